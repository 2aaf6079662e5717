"""A regularisation path as cold batches against the warm chain (Solver.solve_chain), on one handle: C2's shape and
recipe (100000 x 10000 fp32 lasso, synth.dense_lasso_rows), --count lambda values log-spaced from 0.5 to 0.02
lambda_max (64 by default).  `cold` is Solver.solve_batch over all of them, every problem from zero; `chain` cuts the
sorted list into --slots segments and starts each problem but the first of its segment from its neighbour's x, l and
final rho.  Reported per leg: wall time, batch iterations (passes of the loop, summed over the batches),
problem-iterations, multi-vector passes over A (`matvecs`), and how far the chain's x lies from the cold one's.
--sparse runs the same on C4's matrix (synth.csr_lasso(2000000, 500000, 50, seed=4), fp32, CGLS projector).
    python scripts/batch_path_throughput.py [--count 64] [--slots 16] [--sparse] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pogs_amd  # noqa: E402
from pogs_amd import _lib, synth  # noqa: E402


class Counting(pogs_amd.Solver):
    """A Solver that adds up the stats of its batched calls (each call's stats replace the last one's)."""

    def reset_counts(self):
        self.batches, self.batch_iters, self.prob_iters, self.passes = 0, 0, 0, 0

    def solve_batch(self, fs, gs, **kw):
        out = []
        for lo in range(0, len(fs), _lib.BATCH_MAX):    # one library call at a time, so that every call is counted
            kw_lo = dict(kw)
            for key in ("x0", "l0", "warm", "rho"):
                if isinstance(kw.get(key), (list, tuple, np.ndarray)):
                    kw_lo[key] = kw[key][lo:lo + _lib.BATCH_MAX]
            out += super().solve_batch(fs[lo:lo + _lib.BATCH_MAX], gs[lo:lo + _lib.BATCH_MAX], **kw_lo)
            st = self.stats()
            self.batches += 1
            self.batch_iters += st["iterations"]
            self.prob_iters += st["batch_problem_iters"]
            self.passes += st["matvecs"]
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--slots", type=int, default=_lib.BATCH_MAX)
    ap.add_argument("--sparse", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t0 = time.perf_counter()
    if a.sparse:
        A, b, _ = synth.csr_lasso(2000000, 500000, 50, seed=4, dtype=np.float32)
        label = "C4 (sparse, CGLS)"
    else:
        A, b, _ = synth.dense_lasso_rows(100000, 10000, seed=0)
        label = "C2 (dense)"
    m, n = A.shape
    lmax = float(np.max(np.abs(A.T @ np.asarray(b, np.float32))))
    lambdas = lmax * np.geomspace(0.5, 0.02, a.count)
    say("%s lasso path: m %d, n %d, fp32; %d lambdas from 0.5 to 0.02 lambda_max (%.4g); data built in %.1f s"
        % (label, m, n, a.count, lmax, time.perf_counter() - t0))
    say("%-22s %9s %8s %11s %11s %8s  %s" % ("leg", "wall_s", "batches", "batch_iter", "prob_iter", "matvecs",
                                             "iterations of each lambda"))
    fgs = [pogs_amd.graph.lasso_functions(b, float(lam), n) for lam in lambdas]
    fs, gs = [fg[0] for fg in fgs], [fg[1] for fg in fgs]
    with Counting(A, dtype=np.float32) as s:
        s.reset_counts()
        s.solve_batch(fs[:1], gs[:1], max_iter=3)   # warm-up: code objects loaded, pool filled
        legs = {}
        for leg in ("cold", "chain"):
            s.reset_counts()
            t = time.perf_counter()
            if leg == "cold":
                res = s.solve_batch(fs, gs)
            else:
                res = s.solve_chain(fs, gs, slots=a.slots)
            t = time.perf_counter() - t
            legs[leg] = (t, s.prob_iters, res)
            name = "cold (solve_batch)" if leg == "cold" else "chain (slots %d)" % a.slots
            say("%-22s %9.3f %8d %11d %11d %8d  %s" % (name, t, s.batches, s.batch_iters, s.prob_iters, s.passes,
                                                       ",".join(str(r["iterations"] + 1) for r in res)))
    (tc, pc, rc), (tw, pw, rw) = legs["cold"], legs["chain"]
    dx = max(float(np.linalg.norm(c["x"] - w["x"]) / max(np.linalg.norm(c["x"]), 1e-30)) for c, w in zip(rc, rw))
    say("status: cold %s, chain %s; largest |x_chain - x_cold| / |x_cold| %.2e"
        % (sorted({r["status"] for r in rc}), sorted({r["status"] for r in rw}), dx))
    say("chain against cold: %.2fx fewer problem-iterations, %.2fx the wall time" % (pc / max(pw, 1), tw / tc))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
