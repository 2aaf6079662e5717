"""Kernel times of the batched passes over A: the fp64 kernels against their float-storage forms
(profiles/mixed_batch_kernel_times.txt is this script's output).

The passes are run through the diagnostic entries (PogsAmdBatchRowsCheck / PogsAmdBatchColsCheck on a matrix of doubles,
PogsAmdBatchRowsMixedCheck / PogsAmdBatchColsMixedCheck on the same values as floats), each `--reps` times in turn, at
K = 16 and K = 8 problems.  An entry uploads its matrix before the launch, so every launch streams it from HBM.  The
entries time nothing themselves: run the script under the profiler's kernel trace and hand the trace to --summarize,
    rocprofv3 --kernel-trace --output-format csv -d OUT -o t -- python scripts/batch_mixed_kernel_times.py
    python scripts/batch_mixed_kernel_times.py --summarize OUT/**/t_kernel_trace.csv [--out FILE]
which prints, per kernel and K, the dispatch times and the float / fp64 ratio with the spread of the fp64 dispatches
next to it.  Default shape 40000 x 10000 (1.6 GB of floats, 3.2 GB of doubles: C2's row length, far beyond the caches)."""
import argparse
import csv
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (16, 8)
LEGS = (("rows fp64", "batch_rows_kernel<double"), ("rows float", "batch_rows_mixed_kernel"),
        ("cols fp64", "batch_cols_kernel<double"), ("cols float", "batch_cols_mixed_kernel"))


def run(m, n, reps):
    from pogs_amd import _lib

    rng = np.random.default_rng(0)
    M32 = rng.standard_normal((m, n), dtype=np.float32)
    M64 = M32.astype(np.float64)
    for k in KS:
        X, U = rng.standard_normal((k, n)), rng.standard_normal((k, m))
        Y, Z = np.zeros((k, m)), np.zeros((k, n))
        act = list(range(k))
        for _ in range(reps):
            y64 = _lib.batch_rows_check(0, M64, n, X, Y, act)
            y32 = _lib.batch_rows_mixed_check(M32, n, X, Y, act)
            z64, _, _ = _lib.batch_cols_check(M64, n, U, Z, act)
            z32, _, _ = _lib.batch_cols_mixed_check(M32, n, U, Z, act)
            assert np.array_equal(y64.view(np.uint8), y32.view(np.uint8)), "row dots differ in a bit"
            assert np.array_equal(z64.view(np.uint8), z32.view(np.uint8)), "column sums differ in a bit"
    print("ran %d x %d, K in %s, %d reps each" % (m, n, KS, reps))


def short(name):
    return re.search(r"batch_\w+(<[^>]*>)?", name).group(0)


def summarize(path, m, n, reps, out):
    times = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            times.setdefault(row["Kernel_Name"], []).append(
                (int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6))
    lines = ["batched passes over A by kernel, %d x %d, %d dispatches each (ms; GB/s of the matrix alone)" % (m, n, reps),
             "%-11s %3s %9s %9s %9s %8s  %s" % ("pass", "K", "median", "min", "max", "GB/s", "kernel")]
    med = {}
    for leg, key in LEGS:
        for name in sorted(nm for nm in times if key in nm and "reduce" not in nm):
            ms = [t for _, t in sorted(times[name])]
            for q, k in enumerate(KS):
                part = np.asarray(ms[q * reps:(q + 1) * reps])
                if part.size == 0:
                    continue
                size = m * n * (8 if "fp64" in leg else 4)
                med[(leg, k, name)] = (np.median(part), (part.max() - part.min()) / part.min())
                lines.append("%-11s %3d %9.4f %9.4f %9.4f %8.0f  %s" % (leg, k, np.median(part), part.min(), part.max(),
                                                                       size / np.median(part) / 1e6, short(name)))
    lines.append("")
    lines.append("float / fp64 kernel time (spread = (max - min) / min of the fp64 dispatches)")
    for side in ("rows", "cols"):
        for k in KS:
            base = [v for (leg, kk, _), v in med.items() if leg == side + " fp64" and kk == k]
            for (leg, kk, name), v in med.items():
                if leg == side + " float" and kk == k and base:
                    ratio, spread = v[0] / base[0][0], base[0][1]
                    lines.append("%s K %2d  %.3f  (spread %.3f)  %s  %s" % (
                        side, k, ratio, spread, "faster by more than the spread" if ratio < 1 - spread else
                        "not faster beyond the spread", short(name)))
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("m", nargs="?", type=int, default=40000)
    ap.add_argument("n", nargs="?", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize, a.m, a.n, a.reps, a.out)
    else:
        run(a.m, a.n, a.reps)
