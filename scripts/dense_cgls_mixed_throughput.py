"""Mixed storage with the one-pass CGLS projector against the plain fp64 PROJ_CGLS_FUSED handle, in fp64, on a dense
logistic problem (synth.dense_logistic_rows with logit_std 2, lambda 0.01; default C3's shape, 200000 x 5000; a wide
shape a user would run: --m 20000 --n 10000): three handles in one process -- the plain handle, the mixed handle
(storage=float32) and the mixed handle created with POGS_AMD_MIXED_PASS=0 (same rounded matrix, every pass on the fp64
copy) -- warmed up once each and then solved in turn --rounds times.  Every step runs under its own time limit
(--limit seconds: past it the process ends with status 124 and nothing more is started).  Per handle and round:
iterations, it/s (iterations over the loop time), matvecs / iterations, cg_iters / iterations; then the spread between
the rounds.  Then, not part of the timing, handles created with profile=1 and POGS_AMD_CG_TIME_FORM=1, 2, 3, which
brackets ONE form of the loop's recurring launches with HIP events: the mean time per launch of the start's A^T r (ACC),
of L1 (DOT + ACC) and of the y-sync product (DOT), float copy against fp64 copy.
    python scripts/dense_cgls_mixed_throughput.py [--m 200000] [--n 5000] [--rounds 3] [--limit 180] [--no-profile] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import pogs_amd  # noqa: E402
from pogs_amd import _lib, synth  # noqa: E402
from dense_cgls_throughput import limited  # noqa: E402

FORMS = {1: "start A^T r (ACC)", 2: "L1 (DOT + ACC)", 3: "y-sync (DOT)"}


def create(A, kind, **kw):
    """kind: plain | mixed | mixed-off (POGS_AMD_MIXED_PASS is read at create)"""
    os.environ.pop("POGS_AMD_MIXED_PASS", None)
    if kind == "mixed-off":
        os.environ["POGS_AMD_MIXED_PASS"] = "0"
    try:
        return pogs_amd.Solver(A, dtype=np.float64, projector=_lib.PROJ_CGLS_FUSED,
                               storage=None if kind == "plain" else np.float32, **kw)
    finally:
        os.environ.pop("POGS_AMD_MIXED_PASS", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=180.0)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # (kept current: a step that runs into its limit ends the process)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    t0 = time.perf_counter()
    A, b, _ = synth.dense_logistic_rows(a.m, a.n, seed=0, logit_std=2.0)
    A = A.astype(np.float64)
    f, g = pogs_amd.graph.logistic_functions(b, 0.01, a.n)
    say("dense logistic, m %d, n %d, fp64, lambda 0.01; data built in %.1f s" % (a.m, a.n, time.perf_counter() - t0))
    kinds = ("plain", "mixed", "mixed-off")
    solvers = {}
    for kind in kinds:
        solvers[kind] = limited(a.limit, "the set-up of " + kind, lambda: create(A, kind))
        limited(a.limit, "the warm-up of " + kind, lambda: solvers[kind].solve(f, g, max_iter=3))   # code objects loaded
    say("%-10s %5s %10s %7s %9s %12s %13s" % ("handle", "round", "iterations", "status", "it/s", "matvecs/iter", "cg_iters/iter"))
    rates = {k: [] for k in kinds}
    last = {}
    for rnd in range(a.rounds):
        for kind in kinds:
            s = solvers[kind]
            s.reset_stats()
            res = limited(a.limit, "%s, round %d" % (kind, rnd), lambda: s.solve(f, g))
            st = s.stats()
            it = st["iterations"]
            rates[kind].append(it / st["t_loop_s"])
            last[kind] = (it, st["cg_iters"], res["x"])
            say("%-10s %5d %10d %7d %9.1f %12.2f %13.2f" % (kind, rnd, it, res["status"], rates[kind][-1], st["matvecs"] / it,
                                                            st["cg_iters"] / it))
    for s in solvers.values():
        s.close()
    for kind in kinds:
        r = rates[kind]
        say("%-10s it/s: best %.1f, worst %.1f, spread %.1f %%; iterations %d, CG steps %d"
            % (kind, max(r), min(r), 100.0 * (max(r) - min(r)) / max(r), last[kind][0], last[kind][1]))
    bp, bm, bo = (max(rates[k]) for k in kinds)
    say("it/s, best round: mixed / plain %.3f, mixed / mixed-off %.3f, mixed-off / plain %.3f" % (bm / bp, bm / bo, bo / bp))
    nx = np.linalg.norm(last["plain"][2])
    say("relative distance in x: mixed - plain %.2e, mixed - mixed-off %.2e"
        % (np.linalg.norm(last["mixed"][2] - last["plain"][2]) / nx, np.linalg.norm(last["mixed"][2] - last["mixed-off"][2]) / nx))
    if not a.no_profile:
        mean = {}
        for kind in ("plain", "mixed"):
            for form, what in FORMS.items():
                os.environ["POGS_AMD_CG_TIME_FORM"] = str(form)
                try:
                    with limited(a.limit, "the profiled set-up of " + kind, lambda: create(A, kind, profile=True)) as s:
                        limited(a.limit, "the profiled warm-up of " + kind, lambda: s.solve(f, g, max_iter=3))
                        s.reset_stats()
                        limited(a.limit, "the profiled solve of " + kind, lambda: s.solve(f, g))
                        st = s.stats()
                finally:
                    os.environ.pop("POGS_AMD_CG_TIME_FORM", None)
                mean[(kind, form)] = (st["stream_ms"], st["stream_launches"], st["stream_bytes"])
        for form, what in FORMS.items():
            row = []
            for kind in ("plain", "mixed"):
                row.append(mean[(kind, form)])
            say("%-18s plain: %6d timed launches, %.1f us each, %.0f GB/s | mixed: %6d, %.1f us each, %.0f GB/s | time ratio %.3f"
                % (what, row[0][1], 1e3 * row[0][0] / max(row[0][1], 1), row[0][2] / max(row[0][0], 1e-9) / 1e6,
                   row[1][1], 1e3 * row[1][0] / max(row[1][1], 1), row[1][2] / max(row[1][0], 1e-9) / 1e6,
                   (row[1][0] / max(row[1][1], 1)) / (row[0][0] / max(row[0][1], 1))))


if __name__ == "__main__":
    main()
