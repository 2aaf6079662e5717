"""Throughput of mixed-storage SPARSE handles (profiles/sparse_mixed_throughput.txt is this script's output).

A lasso (lambda = 0.1, bench.py's c4 value) on a CSR matrix with a fixed number of N(0, 1) non-zeros per row, made on
the device in fp64 (columns uniform, sorted inside a row; an index may repeat, the products add such entries up) and
handed over as the device-CSR tuple.  Default: C4's shape, 2 000 000 x 500 000 with 50 per row (1e8 non-zeros), CGLS.
`--direct` takes the direct projector (give a short side <= 16384, e.g. 2000000 2000: the shape of
profiles/sparse_direct_throughput.txt).  Legs, each a handle of its own on the same device arrays, in one process:
  f64        the plain fp64 handle (the code path before mixed storage)
  mixed-off  values = float32, POGS_AMD_MIXED_PASS=0: rounded values, tiled values kept as doubles, the existing kernel
  mixed-on   values = float32: the tiled values as floats, every solo product on the float-value kernel
  f32        the fp32 handle (the values rounded to float before anything else)
  f64-b      a second plain fp64 handle, created last: the same code on other device addresses -- what two handles of
             one kind differ by, next to what the rounds of one handle differ by
Per leg: set-up seconds, device memory the handle took, and of a converged solve iterations, cg_iters, status, optval;
then `rounds` alternating rounds of whole solves: iterations per second of the loop (min .. max over the rounds) and,
from options.profile (every 8th launch), the HIP-event time per product and the TB/s of its algorithmic bytes.
The stored formats (bytes per stored element of each tiled copy) come from the info words of PogsAmdSparseCgCheck on
a CGLS handle.  Usage: python scripts/sparse_mixed_throughput.py [m n] [--per-row K] [--direct] [--rounds R]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import pogs_amd
from pogs_amd import _lib
from pogs_amd import graph as G

ap = argparse.ArgumentParser()
ap.add_argument("m", nargs="?", type=int, default=2000000)
ap.add_argument("n", nargs="?", type=int, default=500000)
ap.add_argument("--per-row", type=int, default=50)
ap.add_argument("--direct", action="store_true")
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
m, n, k = args.m, args.n, args.per_row
dev = torch.device("cuda:0")
projector = _lib.PROJ_DIRECT if args.direct else _lib.PROJ_CGLS

gen = torch.Generator(device=dev)
gen.manual_seed(1234)
x_true = torch.randn(n, generator=gen, device=dev, dtype=torch.float64) * (torch.rand(n, generator=gen, device=dev) < 0.05)
cols = torch.sort(torch.randint(0, n, (m, k), generator=gen, device=dev, dtype=torch.int32), dim=1).values.contiguous()
vals64 = torch.randn((m, k), generator=gen, device=dev, dtype=torch.float64)
b = ((vals64 * x_true[cols.long()]).sum(1) + 0.1 * torch.randn(m, generator=gen, device=dev, dtype=torch.float64)).cpu().numpy()
ptr = (torch.arange(m + 1, device=dev, dtype=torch.int64) * k).to(torch.int32)
vals32 = vals64.float()
nnz = m * k
assert nnz < 2 ** 31 and not torch.equal(vals32.double(), vals64)
f, g = G.lasso_functions(b, 0.1, n)
torch.cuda.synchronize()

LEGS = [   # name, dtype, values, environment at create
    ("f64", np.float64, None, {}),
    ("mixed-off", np.float64, np.float32, {"POGS_AMD_MIXED_PASS": "0"}),
    ("mixed-on", np.float64, np.float32, {}),
    ("f32", np.float32, None, {}),
    ("f64-b", np.float64, None, {}),
]


def create(dtype, values, env, proj=projector):
    os.environ.pop("POGS_AMD_MIXED_PASS", None)
    os.environ.update(env)
    v = vals64 if dtype == np.float64 else vals32
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.time()
    s = pogs_amd.Solver((v.data_ptr(), ptr.data_ptr(), cols.data_ptr(), nnz), dtype=dtype, shape=(m, n), device_ptr=True,
                        profile=8, projector=proj, values=values)
    t1 = time.time()
    free1 = torch.cuda.mem_get_info()[0]
    for key in env:
        os.environ.pop(key, None)
    return s, t1 - t0, (free0 - free1) / 2.0 ** 30


def stored_formats():
    """bytes per stored element of both tiled copies, fp64 values against float values, from a CGLS handle's info words"""
    s, _, _ = create(np.float64, None, {}, _lib.PROJ_CGLS)
    zx, zy = np.zeros(n), np.zeros(m)
    info = _lib.sparse_cg_check(s._h, zx, zy, zx, zy, zx, zx, zy, 1e-8, max_steps=1, loop=_lib.CG_HOST_COLD)["info"]
    s.close()
    b8 = b4 = 0.0
    for name, i in zip(("A", "A^T"), info):
        if not i["tiled"]:
            print("# copy %-3s is not tiled (%s)" % (name, _lib.SPMV_WHY.get(i["why"], i["why"])))
            continue
        ids = 1 if i["two"] else 2
        el = i["units"] * 64
        print("# copy %-3s %s, %d x %d tiles of %d rows, %d column groups, %.3f stored elements per non-zero: %d B per "
              "element in fp64, %d B with float values" % (name, "two id slots" if i["two"] else "row tags", i["nrr"], i["ncb"],
                                                           i["rr_rows"], i["ncg"], el / nnz, 8 + 2 + ids, 4 + 2 + ids))
        b8 += el * (8 + 2 + ids)
        b4 += el * (4 + 2 + ids)
    return b8 / b4 if b4 else float("nan")


print("# %d x %d, %d non-zeros per row (%.3g in all), lasso lambda 0.1, projector %s; %d rounds of whole solves" % (
    m, n, k, nnz, "DIRECT" if args.direct else "CGLS", args.rounds))
byte_ratio = stored_formats()
print("# byte ratio of the stored formats, fp64 values / float values: %.3f" % byte_ratio)
handles = {}
print("%-10s %9s %11s %7s %7s %9s %14s" % ("leg", "set-up s", "memory GiB", "status", "iters", "cg_iters", "optval"))
for name, dtype, values, env in LEGS:
    s, setup_s, gib = create(dtype, values, env)
    r = s.solve(f, g)
    st = s.stats()
    handles[name] = (s, r["iterations"], st["cg_iters"])
    print("%-10s %9.3f %11.2f %7d %7d %9d %14.9g" % (name, setup_s, gib, r["status"], r["iterations"], st["cg_iters"], r["optval"]))
    sys.stdout.flush()

rates = {name: [] for name in handles}
prods = {name: [] for name in handles}
bytes_per = {}
for rnd in range(args.rounds):
    for name, (s, _, _) in handles.items():
        s.reset_stats()
        s.solve(f, g)
        st = s.stats()
        rates[name].append(st["iterations"] / st["t_loop_s"])
        prods[name].append(st["stream_ms"] / max(1, st["stream_launches"]))
        bytes_per[name] = st["stream_bytes"] / max(1, st["stream_launches"])
print()
print("%-10s %9s %19s %11s %10s %9s" % ("leg", "it/s", "(min .. max)", "product ms", "GB / prod.", "TB/s"))
for name in handles:
    r, p = np.asarray(rates[name]), np.asarray(prods[name])
    print("%-10s %9.1f %8.1f .. %-8.1f %11.4f %10.3f %9.2f" % (name, np.median(r), r.min(), r.max(), np.median(p),
                                                           bytes_per[name] / 1e9, bytes_per[name] / (np.median(p) * 1e-3) / 1e12))
base = np.asarray(rates["f64"])
print()
print("run-to-run spread of f64 over the rounds: max / min = %.3f" % (base.max() / base.min()))
for name in ("f64-b", "mixed-off", "mixed-on", "f32"):
    print("it/s ratio %-9s / f64 = %.3f    product-time ratio f64 / %-9s = %.3f" % (
        name, np.median(rates[name]) / np.median(base), name, np.median(prods["f64"]) / np.median(prods[name])))
same = handles["mixed-on"][1:] == handles["mixed-off"][1:]
print("iterations and cg_iters of mixed-on %s those of mixed-off; f64: %d / %d, mixed: %d / %d" % (
    "equal" if same else "DIFFER FROM", handles["f64"][1], handles["f64"][2], handles["mixed-on"][1], handles["mixed-on"][2]))
for s, _, _ in handles.values():
    s.close()
