"""Re-solve throughput of the persistent many-problem handle (pogs_amd.ManySolver / PogsAmdManyCreate): README-recipe
lassos at C1's shape (500 x 300, one seed per problem), k = 1024, fp64 and fp32, ten lambda from 0.5 lambda_max down
(lambda_max = max|A^T b| per problem), solved three ways:
    one-shot    ten solve_many calls (each sets the problems up again and starts cold)
    handle cold one ManySolver, ten cold solves
    handle last one ManySolver, one cold solve, then nine start="last" solves (own last x, l and rho)
For each: total seconds, problems/s, total problem-iterations, setup and loop time; then the two ratios against the
one-shot leg.
    python scripts/many_resolve_throughput.py [--out FILE] [--k 1024] [--steps 10]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import pogs_amd  # noqa: E402
from many_throughput import SUMMARY, problems  # noqa: E402


def captured(fn):
    """fn() with the process's stdout (the library's summary line included) captured: (result, text)."""
    import tempfile

    sys.stdout.flush()
    fd = os.dup(1)
    with tempfile.TemporaryFile(mode="w+") as tmp:
        os.dup2(tmp.fileno(), 1)
        try:
            res = fn()
        finally:
            sys.stdout.flush()
            os.dup2(fd, 1)
            os.close(fd)
        tmp.seek(0)
        return res, tmp.read()


def functions(A, B, fracs):
    """Per step the (fs, gs) of the k lassos at lambda = frac * max|A_j^T b_j|."""
    k, m, n = A.shape
    lam_max = np.abs(np.einsum("kmn,km->kn", A, B)).max(axis=1)
    steps = []
    for fr in fracs:
        fgs = [pogs_amd.graph.lasso_functions(B[j], fr * lam_max[j], n) for j in range(k)]
        steps.append(([p[0] for p in fgs], [p[1] for p in fgs]))
    return steps


def leg_one_shot(A, steps, dt):
    t0 = time.perf_counter()
    setup = loop = 0.0
    iters = 0
    for fs, gs in steps:
        res, text = captured(lambda: pogs_amd.solve_many(A, fs, gs, dtype=dt, verbose=1))
        mt = SUMMARY.search(text)
        setup += float(mt.group(1))
        loop += float(mt.group(2))
        iters += int(np.sum(res["iterations"] + 1))
        assert np.all(res["status"] == 0)
    return time.perf_counter() - t0, iters, setup, loop, res


def leg_handle(A, steps, dt, chained):
    t0 = time.perf_counter()
    loop = 0.0
    iters = 0
    with pogs_amd.ManySolver(A, dtype=dt) as s:
        for i, (fs, gs) in enumerate(steps):
            res = s.solve(fs, gs, start="last" if chained and i > 0 else "cold")
            info = s.info()
            loop += info["loop_s"]
            iters += info["problem_iters"]
            assert np.all(res["status"] == 0)
        setup = info["setup_s"]
    return time.perf_counter() - t0, iters, setup, loop, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    m, n, k = 500, 300, a.k
    fracs = np.geomspace(0.5, 0.05, a.steps)
    say("many-problem re-solves: %d lassos of %d x %d (README recipe, one seed per problem), %d lambda from %.2f to "
        "%.3f lambda_max" % (k, m, n, a.steps, fracs[0], fracs[-1]))
    say("%-6s %-12s | %9s %11s %14s %9s %9s | %s" % ("dtype", "way", "total s", "problems/s", "problem-iters",
                                                     "setup s", "loop s", "against one-shot"))
    A64, B = problems(k, m, n)
    for dt in (np.float64, np.float32):
        A = A64.astype(dt)
        steps = functions(A64, B, fracs)
        captured(lambda: pogs_amd.solve_many(A[:1], steps[0][0][:1], steps[0][1][:1], dtype=dt))   # warm: code, pool
        rows = [("one-shot",) + leg_one_shot(A, steps, dt), ("handle cold",) + leg_handle(A, steps, dt, False),
                ("handle last",) + leg_handle(A, steps, dt, True)]
        base_t, base_it = rows[0][1], rows[0][2]
        # the cold handle is the one-shot call, byte for byte; the chain ends at the same solutions to the tolerance
        assert rows[0][5]["x"].tobytes() == rows[1][5]["x"].tobytes()
        err = np.linalg.norm(rows[2][5]["x"] - rows[0][5]["x"], axis=1) / np.linalg.norm(rows[0][5]["x"], axis=1)
        for name, t, iters, setup, loop, _ in rows:
            say("%-6s %-12s | %9.3f %11.1f %14d %9.3f %9.3f | %.2fx faster, %.2fx fewer iterations" % (
                "fp64" if dt == np.float64 else "fp32", name, t, k * a.steps / t, iters, setup, loop, base_t / t,
                base_it / max(iters, 1)))
        say("       last step, chained against one-shot: relative x difference median %.1e, max %.1e"
            % (np.median(err), err.max()))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
