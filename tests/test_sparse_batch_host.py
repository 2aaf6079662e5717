"""CPU tests of the batched sparse-solve boundary (include/pogs_amd.h: PogsAmdSolveBatchSparseFn): the header compiles as
C99 with a call of it, the library exports it, and Solver.solve_batch checks lengths before any library call and
routes a sparse handle to the sparse entry point (a dense one to PogsAmdSolveBatchFn)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from pogs_amd import _lib, graph

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

SNIPPET = r"""
#include "pogs_amd.h"
int call_sparse_batch(PogsAmdSolver *s, const PogsAmdFn *f, const PogsAmdFn *g, double *x, unsigned int *it,
                      int *st) {
  double rho[POGS_AMD_BATCH_MAX];
  for (int j = 0; j < POGS_AMD_BATCH_MAX; ++j) rho[j] = 1.0;
  return PogsAmdSolveBatchSparseFn(s, 2, f, g, rho, 1e-4, 1e-4, 2500u, 0u, 1, 1, x, NULL, NULL, NULL, NULL, it, st);
}
"""


def test_header_compiles_as_c99_with_a_sparse_batch_call(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "sparse_batch_call.c"
    src.write_text(SNIPPET)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_library_exports_the_sparse_batch_entry():
    assert "PogsAmdSolveBatchSparseFn" in _lib.ABI_SYMBOLS
    assert getattr(_lib.lib, "PogsAmdSolveBatchSparseFn") is not None
    assert _lib.lib.PogsAmdSolveBatchSparseFn.argtypes == _lib.lib.PogsAmdSolveBatchFn.argtypes


def _fake_solver(m, n, sparse):
    # a handle-less Solver: enough for the argument checks, which come before any library call
    s = object.__new__(graph.Solver)
    s._h = ctypes.c_void_p()
    s.m, s.n, s.dtype, s.sparse = m, n, np.float64, sparse
    return s


def test_sparse_length_mismatches_raise_before_the_library(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")

    monkeypatch.setattr(graph.lib, "PogsAmdSolveBatchSparseFn", boom)
    monkeypatch.setattr(graph.lib, "PogsAmdSolveBatchFn", boom)
    s = _fake_solver(20, 10, sparse=True)
    b = np.ones(20)
    f, g = graph.lasso_functions(b, 0.1, 10)
    with pytest.raises(ValueError):
        s.solve_batch([f, f], [g])                              # f / g counts
    with pytest.raises(ValueError):
        s.solve_batch([f, f], [g, g], rho=[1.0, 2.0, 3.0])     # rho count
    fs, gs = graph.lasso_functions(np.ones(19), 0.1, 10)
    with pytest.raises(ValueError):
        s.solve_batch([f, fs], [g, g])                          # f length
    f2, g2 = graph.lasso_functions(b, 0.1, 11)
    with pytest.raises(ValueError):
        s.solve_batch([f, f2], [g, g2])                         # g length


class _Recorder:
    """Stands in for a batch entry point: records k and the rho values, fills status / iterations, returns 0."""

    def __init__(self):
        self.calls = []

    def __call__(self, h, k, fa, ga, rho, abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop, x, y, l, mu,
                 optval, final_iter, status):
        rhos = list(np.ctypeslib.as_array(ctypes.cast(rho, ctypes.POINTER(ctypes.c_double)), shape=(k,)))
        self.calls.append((k, rhos))
        it = np.ctypeslib.as_array(ctypes.cast(final_iter, ctypes.POINTER(ctypes.c_uint)), shape=(k,))
        it[:] = 7
        return 0


@pytest.mark.parametrize("sparse", [True, False])
def test_solve_batch_routes_by_handle_type(monkeypatch, sparse):
    sp_rec, dn_rec = _Recorder(), _Recorder()
    monkeypatch.setattr(graph.lib, "PogsAmdSolveBatchSparseFn", sp_rec)
    monkeypatch.setattr(graph.lib, "PogsAmdSolveBatchFn", dn_rec)
    m, n = 30, 12
    s = _fake_solver(m, n, sparse=sparse)
    b = np.linspace(-1.0, 1.0, m)
    lambdas = [0.01 * (j + 1) for j in range(21)]
    fgs = [graph.lasso_functions(b, lam, n) for lam in lambdas]
    res = s.solve_batch([fg[0] for fg in fgs], [fg[1] for fg in fgs], rho=[1.0 + j for j in range(21)])
    called, idle = (sp_rec, dn_rec) if sparse else (dn_rec, sp_rec)
    assert idle.calls == []
    assert [c[0] for c in called.calls] == [16, 5]          # split into batches of BATCH_MAX
    assert called.calls[0][1] == [1.0 + j for j in range(16)]
    assert called.calls[1][1] == [17.0, 18.0, 19.0, 20.0, 21.0]
    assert len(res) == 21 and all(r["iterations"] == 7 and r["x"].shape == (n,) for r in res)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sp_batch_spmv_check_refusals(dtype):
    ptr, ind, val = np.array([0, 2, 2, 3]), np.array([0, 4, 1]), np.array([1, 2, 3], dtype)
    X, Y = np.ones((2, 5), dtype), np.zeros((2, 3), dtype)
    bad = {
        "k must be in": lambda: _lib.sp_batch_spmv_check(ptr, ind, val, 5, np.ones((17, 5), dtype),
                                                         np.zeros((17, 3), dtype), [0]),
        "nact must be in": lambda: _lib.sp_batch_spmv_check(ptr, ind, val, 5, X, Y, [0, 1, 1]),
        "act entry repeats": lambda: _lib.sp_batch_spmv_check(ptr, ind, val, 5, X, Y, [1, 1]),
        "act entry out of range": lambda: _lib.sp_batch_spmv_check(ptr, ind, val, 5, X, Y, [2]),
        "must not decrease": lambda: _lib.sp_batch_spmv_check(np.array([0, 2, 1, 3]), ind, val, 5, X, Y, [0]),
        "ptr\\[0\\] must be 0": lambda: _lib.sp_batch_spmv_check(np.array([1, 2, 2, 3]), ind, val, 5, X, Y, [0]),
        "column index out of range": lambda: _lib.sp_batch_spmv_check(ptr, np.array([0, 5, 1]), val, 5, X, Y, [0]),
        "ldx must be": lambda: _lib.sp_batch_spmv_check(ptr, ind, val, 5, X[:, :4], Y, [0]),
        "ldy must be": lambda: _lib.sp_batch_spmv_check(ptr, ind, val, 5, X, Y[:, :2], [0]),
        "ldin must be": lambda: _lib.sp_batch_spmv_check(ptr, ind, val, 5, X, Y, [0], beta=1.0,
                                                         yin=np.zeros((2, 2), dtype)),
        "num_cu must be": lambda: _lib.sp_batch_spmv_check(ptr, ind, val, 5, X, Y, [0], num_cu=-1),
    }
    for msg, call in bad.items():
        with pytest.raises(RuntimeError, match=msg):
            call()
        assert msg.replace("\\", "") in _lib.last_error()
    try:
        Yo, _, geom = _lib.sp_batch_spmv_check(ptr, ind, val, 5, X, Y, [1])
    except RuntimeError as e:        # no device here: the call got past every argument check
        assert "HIP error" in str(e), str(e)
    else:
        assert list(Yo[1]) == [3, 0, 3] and np.all(Yo[0] == 0) and geom[0] == 4
