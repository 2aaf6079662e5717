"""Ragged many-problem throughput (pogs_amd.solve_many_ragged / PogsAmdSolveManyRaggedFn): 1024 lassos with n = 300
and m_j drawn uniformly from [310, 700] (the README recipe from RandomState(j): m_j = randint(310, 701), A = randn(m_j,
300), b = randn(m_j), lambda = 0.1), in fp64 and fp32.
  (a) the ragged call against a loop of one solve_many call per problem (what a caller with unequal shapes had);
  (b) the same 1024 problems all at 500 x 300 (seed j) through the ragged entry against solve_many: the same kernels
      on the same data, so the expectation is parity (the bytes are compared too);
  (c) with --parent ROOT (a built checkout of the parent commit): solve_many at k = 1024 on C1's shape in fresh
      processes of both builds, alternating (scripts/many_throughput.py --one 500,300,1024,f64, its second call's
      summary line): the medians of the total time, against the spread of the parent's own runs.
Wall times are host clocks around calls that end with the results on the host.
    python scripts/many_ragged_throughput.py [--out FILE] [--k 1024] [--loop-max 1024] [--reps 3] [--parent ROOT]
                                             [--parts abc]"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pogs_amd  # noqa: E402

TOTAL = re.compile(r"iterations (\d+)\.\.(\d+); setup ([0-9.e+-]+) s, loop ([0-9.e+-]+) s, total ([0-9.e+-]+) s")


def ragged_problems(k, n=300, lo=310, hi=700):
    mats, bs = [], []
    for j in range(k):
        rs = np.random.RandomState(j)
        m = int(rs.randint(lo, hi + 1))
        mats.append(rs.randn(m, n))
        bs.append(rs.randn(m))
    return mats, bs


def uniform_problems(k, m=500, n=300):
    mats, bs = [], []
    for j in range(k):
        rs = np.random.RandomState(j)
        mats.append(rs.randn(m, n))
        bs.append(rs.randn(m))
    return mats, bs


def functions(mats, bs, lam=0.1):
    fgs = [pogs_amd.graph.lasso_functions(b, lam, A.shape[1]) for A, b in zip(mats, bs)]
    return [p[0] for p in fgs], [p[1] for p in fgs]


def timed(call, reps):
    """(last result, sorted wall times) of reps calls."""
    times, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = call()
        times.append(time.perf_counter() - t0)
    return res, sorted(times)


def alternating(call_a, call_b, reps):
    ta, tb, ra, rb = [], [], None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        ra = call_a()
        ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        rb = call_b()
        tb.append(time.perf_counter() - t0)
    return ra, rb, sorted(ta), sorted(tb)


def one_shot_total(root):
    """The total time of solve_many at k = 1024 on C1's shape in a fresh process of the build at `root`."""
    root = os.path.abspath(root)
    out = subprocess.run([sys.executable, os.path.join(root, "scripts", "many_throughput.py"), "--one",
                          "500,300,1024,f64"], cwd=root, capture_output=True, text=True, check=True).stdout
    mt = TOTAL.search(out)
    if mt is None:
        raise RuntimeError("no summary line in the output of %s:\n%s" % (root, out))
    return float(mt.group(5)), "iterations %s..%s; setup %s s, loop %s s, total %s s" % mt.groups()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "many_ragged_throughput.txt"))
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--loop-max", type=int, default=1024, help="problems timed in the loop of (a)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for (c)")
    ap.add_argument("--parent-runs", type=int, default=5)
    ap.add_argument("--parts", default="abc", help="which of (a), (b), (c) to run")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    k = a.k
    med = lambda t: t[len(t) // 2]   # noqa: E731
    ab = "a" in a.parts or "b" in a.parts
    rag_mats, rag_bs = ragged_problems(k if ab else 0)
    uni_mats, uni_bs = uniform_problems(k if ab else 0)
    if ab:
        ms = np.array([A.shape[0] for A in rag_mats])
        say("ragged many-problem throughput: %d lassos (README recipe, seed j), n = 300, m_j in [%d, %d] (mean %.1f); "
            "medians of %d calls" % (k, ms.min(), ms.max(), ms.mean(), a.reps))
    for dt in (np.float64, np.float32) if ab else ():
        name = "fp64" if dt == np.float64 else "fp32"
        # (a)
        # both entries get their matrices packed and in the solve's dtype, as solve_many gets its (k, m, n) array
        fs, gs = functions(rag_mats, rag_bs)
        flat = np.concatenate([A.ravel() for A in rag_mats]).astype(dt)
        shapes = [A.shape for A in rag_mats]
        pogs_amd.solve_many_ragged(rag_mats[:2], fs[:2], gs[:2], dtype=dt)            # warm: code objects, pool
        res, t_rag = timed(lambda: pogs_amd.solve_many_ragged(flat, fs, gs, dtype=dt, shapes=shapes), a.reps)
        nl = min(k, a.loop_max)
        pogs_amd.solve_many(rag_mats[0][None], fs[:1], gs[:1], dtype=dt)
        t0 = time.perf_counter()
        loop = [pogs_amd.solve_many(rag_mats[j][None], fs[j:j + 1], gs[j:j + 1], dtype=dt) for j in range(nl)]
        t_loop = time.perf_counter() - t0
        same = all(res[j]["x"].tobytes() == loop[j]["x"][0].tobytes() and res[j]["iterations"] == loop[j]["iterations"][0]
                   for j in range(nl))
        its = np.array([r["iterations"] for r in res])
        ok = sum(r["status"] == 0 for r in res)
        say("(a) %s ragged call: %.4f s (min %.4f, max %.4f), %.1f problems/s; iterations %d..%d, status 0: %d/%d"
            % (name, med(t_rag), t_rag[0], t_rag[-1], k / med(t_rag), its.min(), its.max(), ok, k))
        say("    %s loop of solve_many(k = 1) over %d problems: %.3f s, %.1f problems/s; ragged / loop = %.1fx; "
            "x and iterations byte-identical: %s" % (name, nl, t_loop, nl / t_loop, (k / med(t_rag)) / (nl / t_loop),
                                                     same))
        # (b)
        fs, gs = functions(uni_mats, uni_bs)
        stack = np.stack(uni_mats).astype(dt)
        flat, shapes = stack.reshape(-1), [A.shape for A in uni_mats]
        r_rag, r_uni, t_r, t_u = alternating(lambda: pogs_amd.solve_many_ragged(flat, fs, gs, dtype=dt, shapes=shapes),
                                             lambda: pogs_amd.solve_many(stack, fs, gs, dtype=dt), a.reps)
        same = all(r_rag[j]["x"].tobytes() == r_uni["x"][j].tobytes() for j in range(k))
        say("(b) %s 500 x 300, k = %d: ragged entry %.4f s (min %.4f, max %.4f), solve_many %.4f s (min %.4f, max %.4f);"
            " solve_many / ragged = %.3f; x byte-identical: %s"
            % (name, k, med(t_r), t_r[0], t_r[-1], med(t_u), t_u[0], t_u[-1], med(t_u) / med(t_r), same))
    # (c)
    if "c" not in a.parts:
        pass
    elif a.parent:
        say("(c) solve_many, k = 1024, 500 x 300 fp64, fresh processes, parent commit and this change alternating "
            "(scripts/many_throughput.py --one 500,300,1024,f64, second call):")
        tp, tc = [], []
        for r in range(a.parent_runs):
            t, text = one_shot_total(a.parent)
            tp.append(t)
            say("    parent %d: %s" % (r + 1, text))
            t, text = one_shot_total(ROOT)
            tc.append(t)
            say("    change %d: %s" % (r + 1, text))
        tp.sort()
        tc.sort()
        spread = tp[-1] - tp[0]
        diff = abs(med(tc) - med(tp))
        say("    parent total s: median %.4f, min %.4f, max %.4f (spread %.4f); change: median %.4f, min %.4f, max %.4f; "
            "medians differ by %.4f s: %s the parent's spread"
            % (med(tp), tp[0], tp[-1], spread, med(tc), tc[0], tc[-1], diff, "within" if diff <= spread else "OUTSIDE"))
    else:
        say("(c) not measured: no --parent checkout given")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
