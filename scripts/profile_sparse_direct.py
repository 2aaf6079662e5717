"""Measures the sparse solver's direct projector next to its CGLS projector and writes profiles/sparse_direct_throughput.txt.

For fp32 and a matrix of M x K with NNZ non-zeros per row (default 2e6 x {2000, 10000}, 50 per row), per K:
  * the set-up of a direct handle, split into Gram / Cholesky / inverse (HIP events), next to the CGLS handle's set-up;
  * iterations/s of a lasso on the direct handle and on a CGLS handle of the same matrix (PogsAmdBeginRun +
    PogsAmdIterate: the loop alone, no set-up, no epilogue);
  * problem-iterations/s of a batch of 8 lassos on both handles.
Then rho_W = max |W (I + A_eq^T A_eq) W^T - I| of one factor at the cap (K = 16384), the products taken in fp64 on the GPU
with torch, and, with --accuracy, the ratios the tests of tests/test_gpu_sparse_direct.py print (pytest -s).

    python scripts/profile_sparse_direct.py [--rows 2000000] [--ks 2000,10000] [--cap-rows 200000] [--accuracy] [--out FILE]
"""
import argparse
import os
import subprocess
import sys
import time

os.environ.setdefault("POGS_AMD_TORCH_PRELOAD", "1")
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402


def matrix(m, n, per_row, seed):
    """CSR of m x n with per_row entries in every row (sorted columns; a column drawn twice stays two entries, which the
    engine adds up), built without a COO detour: 1e8 entries in seconds"""
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.integers(0, n, size=(m, per_row), dtype=np.int32), axis=1)
    vals = rng.standard_normal((m, per_row), dtype=np.float32)
    ptr = np.arange(0, (m + 1) * per_row, per_row, dtype=np.int64)
    A = sp.csr_matrix((vals.ravel(), cols.ravel(), ptr), shape=(m, n))
    x_true = (rng.standard_normal(n) * (rng.random(n) < 0.05)).astype(np.float32)
    b = A @ x_true + 0.1 * rng.standard_normal(m).astype(np.float32)
    return A, b


def measure(A, b, projector, name, iters, batch_iters, lines):
    import pogs_amd
    from pogs_amd import graph

    m, n = A.shape
    t0 = time.time()
    with pogs_amd.Solver(A, dtype=np.float32, projector=projector) as s:
        t_create = time.time() - t0
        st = s.stats()
        lines.append("  %-6s set-up: create %.2f s (host + upload included), equilibration %.1f ms, norm estimate %.1f ms, "
                     "Gram %.1f ms, Cholesky %.1f ms, inverse + transpose %.1f ms"
                     % (name, t_create, st["equil_ms"], st["normest_ms"], st["gram_ms"], st["chol_ms"], st["trtri_ms"]))
        f, g = graph.lasso_functions(b, 0.1, n)
        s.begin_run(f, g, max_iter=100000)
        s.iterate(10)
        s.reset_stats()
        sec, _ = s.iterate(iters)
        st = s.stats()
        rate = iters / sec
        lines.append("  %-6s solo lasso: %d iterations in %.3f s = %.1f iterations/s (%.2f CG steps and %.2f SpMVs per iteration)"
                     % (name, iters, sec, rate, st["cg_iters"] / iters, st["matvecs"] / iters))
        fgs = [graph.lasso_functions(b, 0.05 * 1.3 ** j, n) for j in range(8)]
        t0 = time.time()
        s.solve_batch([fg[0] for fg in fgs], [fg[1] for fg in fgs], max_iter=batch_iters)
        sec_b = time.time() - t0
        st = s.stats()
        brate = st["batch_problem_iters"] / sec_b
        lines.append("  %-6s batch of 8: %d problem-iterations in %.3f s (whole call) = %.1f problem-iterations/s = %.2f x its solo "
                     "rate (%d products, %d CG steps)"
                     % (name, st["batch_problem_iters"], sec_b, brate, brate / rate, st["matvecs"], st["cg_iters"]))
    return rate, brate


def cap_factor(rows, per_row, lines):
    """rho_W of the factor of a rows x 16384 matrix: H = I + A_eq^T A_eq and W H W^T in fp64 on the GPU"""
    import ctypes

    import torch

    import pogs_amd
    from pogs_amd import _lib

    K = _lib.SPARSE_DIRECT_MAX
    A, _ = matrix(rows, K, per_row, seed=5)
    with pogs_amd.Solver(A, dtype=np.float32, projector=_lib.PROJ_DIRECT) as s:
        st = s.stats()
        vals = np.zeros(A.nnz, np.float32)
        assert _lib.lib.PogsAmdGetEquil(s._h, vals.ctypes.data_as(ctypes.c_void_p), None, None, None) == 0
        W, _ = s.factor()
    lines.append("  %d x %d, %d per row: Gram %.1f ms, Cholesky %.1f ms, inverse + transpose %.1f ms"
                 % (rows, K, per_row, st["gram_ms"], st["chol_ms"], st["trtri_ms"]))
    dev = torch.device("cuda:0")
    H = torch.eye(K, dtype=torch.float64, device=dev)
    chunk = 16384
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
        lo, hi = A.indptr[r0], A.indptr[r1]
        D = torch.zeros((r1 - r0, K), dtype=torch.float64, device=dev)
        rr = torch.from_numpy(np.repeat(np.arange(r1 - r0), np.diff(A.indptr[r0:r1 + 1]))).to(dev)
        cc = torch.from_numpy(A.indices[lo:hi].astype(np.int64)).to(dev)
        vv = torch.from_numpy(vals[lo:hi].astype(np.float64)).to(dev)
        D.index_put_((rr, cc), vv, accumulate=True)
        H += D.T @ D
    W64 = torch.from_numpy(W).to(dev).to(torch.float64)
    R = W64 @ H @ W64.T - torch.eye(K, dtype=torch.float64, device=dev)
    lines.append("  finite: %s; rho_W = max |W H W^T - I| = %.3e; max |W| %.3e, min / max diagonal of W %.3e / %.3e"
                 % (bool(np.all(np.isfinite(W))), float(R.abs().max()), float(np.abs(W).max()), float(np.diag(W).min()),
                    float(np.diag(W).max())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000000)
    ap.add_argument("--per-row", type=int, default=50)
    ap.add_argument("--ks", default="2000,10000")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--batch-iters", type=int, default=30)
    ap.add_argument("--cap-rows", type=int, default=200000, help="0: skip the factor at the cap")
    ap.add_argument("--accuracy", action="store_true", help="also run the accuracy tests and keep the lines they print")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_direct_throughput.txt"))
    a = ap.parse_args()
    lines = ["Sparse direct projector next to CGLS, fp32 (scripts/profile_sparse_direct.py)", ""]
    if a.accuracy:   # in a process of its own, before this one opens the device
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider", "-m", "gpu",
                            os.path.join(ROOT, "tests", "test_gpu_sparse_direct.py"), "-k",
                            "gram_of_real or factor or projection or follows"], capture_output=True, text=True, cwd=ROOT)
        lines.append("Accuracy (tests/test_gpu_sparse_direct.py, pytest -s; exit %d):" % r.returncode)
        lines += ["  " + ln[ln.index(":") + 2:] for ln in r.stdout.splitlines()
                  if "sparse_direct: " in ln or "factor_accuracy: " in ln]
        lines.append("")
    from pogs_amd import _lib

    for K in (int(k) for k in a.ks.split(",") if k):
        A, b = matrix(a.rows, K, a.per_row, seed=K)
        lines.append("%d x %d, %d non-zeros per row:" % (a.rows, K, a.per_row))
        rd, bd = measure(A, b, _lib.PROJ_DIRECT, "direct", a.iters, a.batch_iters, lines)
        rc, bc = measure(A, b, _lib.PROJ_CGLS, "CGLS", a.iters, a.batch_iters, lines)
        lines.append("  direct / CGLS: solo %.2f x, batch of 8 %.2f x" % (rd / rc, bd / bc))
        lines.append("")
        del A, b
    if a.cap_rows:
        lines.append("The factor at the cap:")
        cap_factor(a.cap_rows, a.per_row, lines)
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
