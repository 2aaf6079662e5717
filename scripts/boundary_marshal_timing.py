"""Host cost of the Python boundary's marshalling, with the library call replaced by a function returning 0 (no GPU):
    ManySolver.solve     k = 1024 problems of 64 x 32 on a bare handle, per-element b, every other field a scalar
    Solver.solve_batch   k = 16 problems on a bare 20000 x 2000 handle, the same functions
Compares two checkouts: --rounds rounds, in each a fresh process per checkout (the checkouts alternating) that calls
once to warm up and times the next call.  Prints every figure, then min / median / max per checkout and workload.
    python scripts/boundary_marshal_timing.py --against OTHER_ROOT [--rounds 20] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np

    from pogs_amd import graph

    for name in ("PogsAmdManySolveFn", "PogsAmdSolveBatchFn"):
        setattr(graph.lib, name, lambda *a: 0)
    rng = np.random.default_rng(0)

    def timed(call):
        call()
        t0 = time.perf_counter()
        call()
        return time.perf_counter() - t0

    k, m, n = 1024, 64, 32
    many = object.__new__(graph.ManySolver)
    many.k, many.m, many.n, many.dtype, many._h = k, m, n, np.dtype(np.float64), ctypes.c_void_p(1)
    pairs = [graph.lasso_functions(rng.standard_normal(m), 0.1, n) for _ in range(k)]
    fs, gs = [p[0] for p in pairs], [p[1] for p in pairs]
    t_many = timed(lambda: many.solve(fs, gs))
    many._h = ctypes.c_void_p()
    k, m, n = 16, 20000, 2000
    solo = object.__new__(graph.Solver)
    solo.m, solo.n, solo.dtype, solo.sparse, solo._h = m, n, np.dtype(np.float64), False, ctypes.c_void_p()
    pairs = [graph.lasso_functions(rng.standard_normal(m), 0.1, n) for _ in range(k)]
    fs, gs = [p[0] for p in pairs], [p[1] for p in pairs]
    t_batch = timed(lambda: solo.solve_batch(fs, gs))
    print("%.9f %.9f" % (t_many, t_batch))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", help="the other checkout's root")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    if not args.against:
        ap.error("--against OTHER_ROOT is required")
    trees = [("other", args.against), ("this", ROOT)]
    got = {name: ([], []) for name, _ in trees}
    for _ in range(args.rounds):
        for name, tree in trees:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree], check=True,
                                 capture_output=True, text=True).stdout.split()
            got[name][0].append(float(out[-2]))
            got[name][1].append(float(out[-1]))
    lines = []
    for w, title in enumerate(("ManySolver.solve k=1024 64x32", "solve_batch k=16 20000x2000")):
        for name, _ in trees:
            v = got[name][w]
            lines.append("%-30s %-5s ms: %s" % (title, name, " ".join("%.3f" % (1e3 * t) for t in v)))
            lines.append("%-30s %-5s min %.3f  median %.3f  max %.3f ms" % (title, name, 1e3 * min(v),
                                                                             1e3 * statistics.median(v), 1e3 * max(v)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
