"""Throughput of mixed-storage handles at C2's shape (profiles/mixed_storage_throughput.txt is this script's output).

C2's matrix (100000 x 10000, bench.py's torch_rows: fp32 draws, widened to fp64 on the device) and the README lasso
(lambda = 0.1).  Legs, each a handle of its own on the same device matrix:
  f64        the plain fp64 handle (the code path before mixed storage)
  mixed-off  storage = float32, POGS_AMD_MIXED_PASS=0: rounded matrix, both copies, every pass on the fp64 copy
  mixed-on   storage = float32, the one-pass iteration's hot launches on the float copy
  mixed-full the same with POGS_AMD_MIXED_FULL=1: the full (two dots, two accumulators) form from the first iteration,
             for the question whether the lean form still pays once the tile is float
  f32        the fp32 handle
Per leg: set-up seconds, device memory the handle took, iterations of a converged solve, and -- from `rounds` alternating
runs of begin_run + iterate(steps) -- iterations per second and the average pass time (options.profile, every 8th
launch).  Usage: python scripts/mixed_storage_throughput.py [m n] [--steps K] [--rounds R]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import pogs_amd
from pogs_amd import graph as G

ap = argparse.ArgumentParser()
ap.add_argument("m", nargs="?", type=int, default=100000)
ap.add_argument("n", nargs="?", type=int, default=10000)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
m, n = args.m, args.n
dev = torch.device("cuda:0")

gen = torch.Generator(device=dev)
gen.manual_seed(1234)
x_true = torch.randn(n, generator=gen, device=dev) * (torch.rand(n, generator=gen, device=dev) < 0.1)
gen.manual_seed(1000)
A32 = torch.randn((m, n), generator=gen, device=dev, dtype=torch.float32)
b = (A32 @ x_true + 0.1 * torch.randn(m, generator=gen, device=dev)).double().cpu().numpy()
A64 = A32.double()
f, g = G.lasso_functions(b, 0.1, n)
torch.cuda.synchronize()

LEGS = [   # name, dtype, storage, environment at create
    ("f64", np.float64, None, {}),
    ("mixed-off", np.float64, np.float32, {"POGS_AMD_MIXED_PASS": "0"}),
    ("mixed-on", np.float64, np.float32, {}),
    ("mixed-full", np.float64, np.float32, {"POGS_AMD_MIXED_FULL": "1"}),
    ("f32", np.float32, None, {}),
]


def create(dtype, storage, env):
    for k in ("POGS_AMD_MIXED_PASS", "POGS_AMD_MIXED_FULL"):
        os.environ.pop(k, None)
    os.environ.update(env)
    A = A64 if dtype == np.float64 else A32
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.time()
    s = pogs_amd.Solver(A.data_ptr(), dtype=dtype, shape=(m, n), device_ptr=True, profile=8, storage=storage)
    t1 = time.time()
    free1 = torch.cuda.mem_get_info()[0]
    for k in env:
        os.environ.pop(k, None)
    return s, t1 - t0, (free0 - free1) / 2.0 ** 30


handles = {}
print("# %d x %d, lasso lambda 0.1; %d rounds of %d iterations after %d of warm-up" % (m, n, args.rounds, args.steps, args.warmup))
print("%-11s %9s %11s %7s %7s %6s %7s %9s" % ("leg", "set-up s", "memory GiB", "status", "iters", "exact", "misses", "optval"))
for name, dtype, storage, env in LEGS:
    s, setup_s, gib = create(dtype, storage, env)
    r = s.solve(f, g)
    st = s.stats()
    handles[name] = s
    print("%-11s %9.3f %11.2f %7d %7d %6d %7d %9.6g" % (name, setup_s, gib, r["status"], r["iterations"], st["exact_iters"],
                                                       st["spec_misses"], r["optval"]))
    sys.stdout.flush()

rates = {name: [] for name in handles}
passes = {name: [] for name in handles}
bytes_per = {}
for rnd in range(args.rounds):
    for name, s in handles.items():
        s.begin_run(f, g)
        s.iterate(args.warmup)
        s.reset_stats()
        sec, _ = s.iterate(args.steps)
        st = s.stats()
        rates[name].append(args.steps / sec)
        passes[name].append(st["stream_ms"] / max(1, st["stream_launches"]))
        bytes_per[name] = st["stream_bytes"] / max(1, st["stream_launches"])
print()
print("%-11s %9s %19s %9s %10s %9s" % ("leg", "it/s", "(min .. max)", "pass ms", "GB / pass", "TB/s"))
for name in handles:
    r, p = np.asarray(rates[name]), np.asarray(passes[name])
    print("%-11s %9.1f %8.1f .. %-8.1f %9.4f %10.3f %9.2f" % (name, np.median(r), r.min(), r.max(), np.median(p), bytes_per[name] / 1e9,
                                                         bytes_per[name] / (np.median(p) * 1e-3) / 1e12))
base = np.median(rates["f64"])
print()
for name in ("mixed-off", "mixed-on", "mixed-full", "f32"):
    print("it/s ratio %-10s / f64 = %.3f" % (name, np.median(rates[name]) / base))
for s in handles.values():
    s.close()
