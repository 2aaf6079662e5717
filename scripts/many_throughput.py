"""Many-problem throughput (pogs_amd.solve_many / PogsAmdSolveManyFn): problems solved per second at C1's shape
(500 x 300 lasso, the README recipe with one seed per problem) in fp64 and fp32 for k = 1, 16, 256, 1024, and at
1000 x 500 fp32 for k = 256.  For each: the many-problem call with its setup and loop time (its verbose summary), the
same problems as a loop of one-shot solve_lasso calls in the same process (warm pool; at most --solo-max of them are
timed and the rate is per problem), and for C1 fp64 the CPU oracle.  The loop's achieved bandwidth counts
(2 m n + min(m, n)^2) sizeof(T) bytes per problem-iteration (A read twice, W's triangle twice) against the measured
read ceiling.
    python scripts/many_throughput.py [--out FILE] [--solo-max 64] [--oracle-max 8] [--one SHAPE]"""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pogs_amd  # noqa: E402
from pogs_amd import _lib  # noqa: E402

SUMMARY = re.compile(r"setup ([0-9.e+-]+) s, loop ([0-9.e+-]+) s, total ([0-9.e+-]+) s; (\d+) launches")


def problems(k, m, n, seed0=0):
    A = np.empty((k, m, n))
    B = np.empty((k, m))
    for j in range(k):
        rs = np.random.RandomState(seed0 + j)
        A[j] = rs.randn(m, n)
        B[j] = rs.randn(m)
    return A, B


def many_call(A, B, lam, dtype):
    """solve_many with verbose=1; returns (result, wall s, setup s, loop s, launches) from its summary line."""
    k, m, n = A.shape
    fgs = [pogs_amd.graph.lasso_functions(B[j], lam, n) for j in range(k)]
    sys.stdout.flush()
    fd = os.dup(1)
    with tempfile.TemporaryFile(mode="w+") as tmp:
        os.dup2(tmp.fileno(), 1)
        try:
            t0 = time.perf_counter()
            res = pogs_amd.solve_many(A, [p[0] for p in fgs], [p[1] for p in fgs], dtype=dtype, verbose=1)
            wall = time.perf_counter() - t0
        finally:
            sys.stdout.flush()
            os.dup2(fd, 1)
            os.close(fd)
        tmp.seek(0)
        text = tmp.read()
    mt = SUMMARY.search(text)
    setup, loop, _, launches = (float(mt.group(1)), float(mt.group(2)), float(mt.group(3)), int(mt.group(4)))
    return res, wall, setup, loop, launches, text.strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--solo-max", type=int, default=64)
    ap.add_argument("--oracle-max", type=int, default=8)
    ap.add_argument("--one", default=None, help="m,n,k,f32|f64: one many-problem call only (for a kernel trace)")
    a = ap.parse_args()
    if a.one:
        m, n, k, t = a.one.split(",")
        A, B = problems(int(k), int(m), int(n))
        dt = np.float32 if t == "f32" else np.float64
        many_call(A, B, 0.1, dt)
        r = many_call(A, B, 0.1, dt)
        print(r[5])
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ceil_gbs, _ = _lib.read_bandwidth(nbytes=4 << 30, reps=10)
    say("many-problem throughput: lasso (README recipe, one seed per problem); read ceiling %.0f GB/s measured"
        % ceil_gbs)
    say("%-22s %5s | %10s %9s %9s %8s %7s %7s | %10s %7s | %s" % (
        "shape", "k", "many p/s", "setup s", "loop s", "GB/s", "of ceil", "launch", "solo p/s", "gain", "iters"))
    cases = [((500, 300), np.float64, k) for k in (1, 16, 256, 1024)] + \
            [((500, 300), np.float32, k) for k in (1, 16, 256, 1024)] + [((1000, 500), np.float32, 256)]
    data = {}
    for (m, n), dt, k in cases:
        if (m, n) not in data or data[(m, n)][0].shape[0] < k:
            data[(m, n)] = problems(1024 if (m, n) == (500, 300) else 256, m, n)
        A, B = data[(m, n)]
        A, B = A[:k], B[:k]
        many_call(A[:1], B[:1], 0.1, dt)      # warm: code objects, pool
        res, wall, setup, loop, launches, _ = many_call(A, B, 0.1, dt)
        its = res["iterations"].astype(np.int64) + 1
        isz = np.dtype(dt).itemsize
        gbs = float(its.sum()) * (2.0 * m * n + min(m, n) ** 2) * isz / loop / 1e9
        ns = min(k, a.solo_max)
        pogs_amd.solve_lasso(A[0], B[0], 0.1, dtype=dt)   # warm
        t0 = time.perf_counter()
        for j in range(ns):
            pogs_amd.solve_lasso(A[j], B[j], 0.1, dtype=dt)
        solo_ps = ns / (time.perf_counter() - t0)
        say("%-22s %5d | %10.1f %9.4f %9.4f %8.0f %7.3f %7d | %10.1f %6.1fx | %d..%d, status 0: %d/%d" % (
            "%dx%d %s" % (m, n, "fp64" if dt == np.float64 else "fp32"), k, k / wall, setup, loop, gbs, gbs / ceil_gbs,
            launches, solo_ps, (k / wall) / solo_ps, its.min() - 1, its.max() - 1, int((res["status"] == 0).sum()), k))
    import oracle_binding as ob
    from helpers import soa

    threads = ob.oracle_set_threads()
    A, B = data[(500, 300)]
    no = min(a.oracle_max, A.shape[0])
    t0 = time.perf_counter()
    for j in range(no):
        f, g = pogs_amd.graph.lasso_functions(B[j], 0.1, 300)
        ob.oracle_solve(A[j], soa(f), soa(g), dtype=np.float64)
    say("oracle (CPU restatement, %d threads), 500x300 fp64: %.1f problems/s over %d problems"
        % (threads, no / (time.perf_counter() - t0), no))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
