"""The dense CGLS projector against its one-pass, device-resident form, at C3's shape (200000 x 5000 logistic, fp32,
synth.dense_logistic_rows with logit_std 2, lambda 0.01): one handle per projector value (PROJ_CGLS, PROJ_CGLS_FUSED)
in one process, solved in turn --rounds times.  Every solve runs under its own time limit (--limit seconds: a solve
that exceeds it ends the process with status 124, nothing more is started).  Per projector and round: iterations,
it/s (iterations over the loop time), matvecs / iterations (passes over A per ADMM iteration), cg_iters / iterations.
Then one more solve each on handles created with profile=1 (not part of the timing: an event record costs the stream a
few microseconds): the mean HIP-event time of a launch that reads A -- for PROJ_CGLS the DOT-only and ACC-only passes,
for PROJ_CGLS_FUSED mostly the DOT + ACC pass of a CG step.  The last lines compare the two: the ratio of passes per
iteration, the ratio of it/s, and whether the second reaches 0.85 of the first.
    python scripts/dense_cgls_throughput.py [--m 200000] [--n 5000] [--rounds 3] [--limit 120] [--no-profile] [--out FILE]"""
import argparse
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pogs_amd  # noqa: E402
from pogs_amd import _lib, synth  # noqa: E402


def limited(seconds, what, fn):
    """fn() under a time limit of its own: past it the process ends (a solve cannot be interrupted from inside)"""
    def expired():
        print("time limit of %.0f s exceeded by %s: ending the process" % (seconds, what), flush=True)
        os._exit(124)

    timer = threading.Timer(seconds, expired)
    timer.daemon = True
    timer.start()
    try:
        return fn()
    finally:
        timer.cancel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t0 = time.perf_counter()
    A, b, _ = synth.dense_logistic_rows(a.m, a.n, seed=0, logit_std=2.0)
    f, g = pogs_amd.graph.logistic_functions(b, 0.01, a.n)
    say("dense logistic, m %d, n %d, fp32, lambda 0.01; data built in %.1f s" % (a.m, a.n, time.perf_counter() - t0))
    names = {"cgls": _lib.PROJ_CGLS, "cgls-fused": _lib.PROJ_CGLS_FUSED}
    solvers = {}
    for name, proj in names.items():
        solvers[name] = limited(a.limit, "the set-up of " + name,
                                lambda: pogs_amd.Solver(A, dtype=np.float32, projector=proj))
        limited(a.limit, "the warm-up of " + name, lambda: solvers[name].solve(f, g, max_iter=3))   # code objects loaded
    say("%-11s %5s %10s %8s %9s %12s %12s" % ("projector", "round", "iterations", "status", "it/s", "matvecs/iter",
                                             "cg_iters/iter"))
    best = {}
    for rnd in range(a.rounds):
        for name, s in solvers.items():
            s.reset_stats()
            res = limited(a.limit, "%s, round %d" % (name, rnd), lambda: s.solve(f, g))
            st = s.stats()
            it = st["iterations"]
            its = it / st["t_loop_s"]
            say("%-11s %5d %10d %8d %9.1f %12.2f %12.2f" % (name, rnd, it, res["status"], its, st["matvecs"] / it,
                                                          st["cg_iters"] / it))
            if name not in best or its > best[name][0]:
                best[name] = (its, st["matvecs"] / it, it)
    for s in solvers.values():
        s.close()
    if not a.no_profile:
        for name, proj in names.items():
            with limited(a.limit, "the profiled set-up of " + name,
                         lambda: pogs_amd.Solver(A, dtype=np.float32, projector=proj, profile=True)) as s:
                limited(a.limit, "the profiled warm-up of " + name, lambda: s.solve(f, g, max_iter=3))
                s.reset_stats()
                limited(a.limit, "the profiled solve of " + name, lambda: s.solve(f, g))
                st = s.stats()
                say("%-11s profiled: %d launches that read A in %d iterations, %.1f us each, %.0f GB/s; loop %.3f s, of "
                    "which those launches %.3f s" % (name, st["stream_launches"], st["iterations"],
                                                    1e3 * st["stream_ms"] / max(st["stream_launches"], 1),
                                                    st["stream_bytes"] / max(st["stream_ms"], 1e-9) / 1e6, st["t_loop_s"],
                                                    1e-3 * st["stream_ms"]))
    (i0, p0, n0), (i1, p1, n1) = best["cgls"], best["cgls-fused"]
    say("passes per iteration: cgls %.2f, cgls-fused %.2f, ratio %.3f" % (p0, p1, p0 / p1))
    say("it/s (best round): cgls %.1f, cgls-fused %.1f, ratio %.3f; 0.85 x the ratio of passes = %.3f: %s"
        % (i0, i1, i1 / i0, 0.85 * p0 / p1, "reached" if i1 / i0 >= 0.85 * p0 / p1 else "NOT reached"))
    say("iterations: cgls %d, cgls-fused %d (%.1f %% apart)" % (n0, n1, 100.0 * abs(n1 - n0) / n0))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
