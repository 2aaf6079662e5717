"""Batched sparse-solve throughput on C4's matrix (synth.csr_lasso(2000000, 500000, 50, seed=4), fp32 lasso): for
K = 1, 2, 4, 8, 16 lambda values around C4's lambda = 0.1, problem-iterations per second of one Solver.solve_batch
call against K solo Solver.solve calls on the same handle; the multi-vector products with A / A^T per batch iteration;
and the products timed with HIP events (profile=1; PogsAmdStats.reserved[5..7]), in ms and in GB/s on their
algorithmic bytes (nnz (value + index) + row pointers + K operand and K result vectors), as a fraction of the
device's measured read ceiling (PogsAmdReadBandwidth).
    python scripts/sparse_batch_throughput.py [--ks 1,2,4,8,16] [--no-solo] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pogs_amd  # noqa: E402
from pogs_amd import _lib, synth  # noqa: E402

LAMBDAS = np.geomspace(0.06, 0.16, 16)   # 16 values around C4's 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--no-solo", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ks = [int(v) for v in a.ks.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t0 = time.perf_counter()
    A, b, _ = synth.csr_lasso(2000000, 500000, 50, seed=4, dtype=np.float32)
    m, n = A.shape
    ceil_gbs, pattern = _lib.read_bandwidth(nbytes=4 << 30, reps=10)
    say("C4 batched sparse lasso path: m %d, n %d, nnz %d, fp32; read ceiling %.0f GB/s (%s); data built in %.1f s"
        % (m, n, A.nnz, ceil_gbs, pattern, time.perf_counter() - t0))
    say("%3s %9s %12s %10s %12s %9s %7s %8s %8s %9s %7s %6s  %s" % (
        "K", "batch_s", "prob_it/s", "solo_s", "solo_it/s", "speedup", "b_iter", "prod/it", "cg_step", "prod_ms",
        "GB/s", "ceil", "iterations"))
    with pogs_amd.Solver(A, dtype=np.float32, profile=True) as s:
        fgs = [pogs_amd.graph.lasso_functions(b, float(lam), n) for lam in LAMBDAS]
        s.solve(*fgs[0])                              # warm-up: code objects loaded, pool filled
        s.solve_batch([fgs[0][0]], [fgs[0][1]])
        for k in ks:
            fs, gs = [fg[0] for fg in fgs[:k]], [fg[1] for fg in fgs[:k]]
            tb = time.perf_counter()
            res = s.solve_batch(fs, gs)
            tb = time.perf_counter() - tb
            st = s.stats()
            prob_it = st["batch_problem_iters"]
            prod_ms = st["batch_pass_ms"] / max(st["batch_pass_launches"], 1)
            gbs = st["batch_pass_bytes"] / max(st["batch_pass_ms"], 1e-12) / 1e6
            its = [r["iterations"] + 1 for r in res]
            if a.no_solo:
                ts, solo_rate, spd = float("nan"), float("nan"), float("nan")
            else:
                ts = time.perf_counter()
                solo_its = 0
                for f, g in zip(fs, gs):
                    solo_its += s.solve(f, g)["iterations"] + 1
                ts = time.perf_counter() - ts
                solo_rate = solo_its / ts
                spd = (prob_it / tb) / solo_rate
            say("%3d %9.3f %12.1f %10.3f %12.1f %8.2fx %7d %8.2f %8d %9.3f %7.0f %6.3f  %s" % (
                k, tb, prob_it / tb, ts, solo_rate, spd, st["iterations"], st["matvecs"] / max(st["iterations"], 1),
                st["cg_iters"], prod_ms, gbs, gbs / ceil_gbs, ",".join(str(v) for v in its)))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
