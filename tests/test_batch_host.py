"""CPU tests of the batched-solve boundary (include/pogs_amd.h: PogsAmdSolveBatchFn): the header compiles as C99 with a
call of it, the library exports it, the Python layer has its entry points and checks lengths before any library call."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import pogs_amd
from pogs_amd import _lib, graph

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

SNIPPET = r"""
#include "pogs_amd.h"
int call_batch(PogsAmdSolver *s, const PogsAmdFn *f, const PogsAmdFn *g, double *x, unsigned int *it, int *st) {
  double rho[POGS_AMD_BATCH_MAX];
  for (int j = 0; j < POGS_AMD_BATCH_MAX; ++j) rho[j] = 1.0;
  return PogsAmdSolveBatchFn(s, 2, f, g, rho, 1e-4, 1e-4, 2500u, 0u, 1, 1, x, NULL, NULL, NULL, NULL, it, st);
}
"""


def test_header_compiles_as_c99_with_a_batch_call(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "batch_call.c"
    src.write_text(SNIPPET)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_library_exports_the_batch_entry():
    assert "PogsAmdSolveBatchFn" in _lib.ABI_SYMBOLS
    assert getattr(_lib.lib, "PogsAmdSolveBatchFn") is not None
    assert _lib.BATCH_MAX == 16


def test_python_entry_points_exist():
    assert callable(getattr(pogs_amd.Solver, "solve_batch"))
    assert callable(pogs_amd.solve_lasso_path)
    assert callable(pogs_amd.solve_logistic_path)
    assert "solve_lasso_path" in pogs_amd.__all__ and "solve_logistic_path" in pogs_amd.__all__


def _fake_solver(m, n):
    # a handle-less Solver: enough for the argument checks, which come before any library call
    s = object.__new__(graph.Solver)
    s._h = ctypes.c_void_p()
    s.m, s.n, s.dtype, s.sparse = m, n, np.float64, False
    return s


def test_length_mismatches_raise_before_the_library(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")

    monkeypatch.setattr(graph.lib, "PogsAmdSolveBatchFn", boom)
    s = _fake_solver(20, 10)
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


def _valid_call_runs_or_lacks_a_device(call):
    """After refusals the entry still works: on a GPU box the valid call runs; without one it gets as far as the
    device and fails there, not at an argument check."""
    try:
        return call()
    except RuntimeError as e:
        assert "HIP error" in str(e), str(e)
        return None


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_rows_check_refusals(dtype):
    V = 16 // np.dtype(dtype).itemsize
    M, X, Y = np.zeros((8, 8), dtype), np.zeros((3, 8), dtype), np.zeros((3, 8), dtype)
    bad = {
        "k must be in": lambda: _lib.batch_rows_check(0, M, 8, np.zeros((17, 8), dtype), np.zeros((17, 8), dtype), [0]),
        "nact must be in": lambda: _lib.batch_rows_check(0, M, 8, X, Y, [0, 1, 2, 0]),
        "act entry repeats": lambda: _lib.batch_rows_check(0, M, 8, X, Y, [1, 1]),
        "act entry out of range": lambda: _lib.batch_rows_check(0, M, 8, X, Y, [3]),
        "ldm must be": lambda: _lib.batch_rows_check(0, M, 8 + 1, X, Y, [0]),
        "ldx must be": lambda: _lib.batch_rows_check(0, M, 8, X[:, :8 - V], Y, [0]),
        "ldy must be": lambda: _lib.batch_rows_check(0, M, 8, X, Y[:, :7], [0]),
        "unknown tri": lambda: _lib.batch_rows_check(3, M, 8, X, Y, [0]),
        "triangle needs rows == cols": lambda: _lib.batch_rows_check(1, M[:5], 8, X, Y, [0]),
    }
    for msg, call in bad.items():
        with pytest.raises(RuntimeError, match=msg):
            call()
        assert msg in _lib.last_error()
    M[:] = 1
    X[:] = 2
    out = _valid_call_runs_or_lacks_a_device(lambda: _lib.batch_rows_check(0, M, 8, X, Y, [2, 0]))
    if out is not None:
        assert np.all(out[[0, 2]] == 16) and np.all(out[1] == 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_cols_check_refusals(dtype):
    M, U, Z = np.zeros((6, 8), dtype), np.zeros((2, 6), dtype), np.zeros((2, 8), dtype)
    bad = {
        "k must be in": lambda: _lib.batch_cols_check(M, 8, np.zeros((17, 6), dtype), np.zeros((17, 8), dtype), [0]),
        "nact must be in": lambda: _lib.batch_cols_check(M, 8, U, Z, [0, 1, 0]),
        "act entry repeats": lambda: _lib.batch_cols_check(M, 8, U, Z, [0, 0]),
        "act entry out of range": lambda: _lib.batch_cols_check(M, 8, U, Z, [-1]),
        "ldm must be": lambda: _lib.batch_cols_check(M, 9, U, Z, [0]),
        "ldu must be": lambda: _lib.batch_cols_check(M, 8, U[:, :5], Z, [0]),
        "ldz must be": lambda: _lib.batch_cols_check(M, 8, U, Z[:, :7], [0]),
    }
    for msg, call in bad.items():
        with pytest.raises(RuntimeError, match=msg):
            call()
        assert msg in _lib.last_error()
    M[:] = 1
    U[:] = 3
    out = _valid_call_runs_or_lacks_a_device(lambda: _lib.batch_cols_check(M, 7, U, Z, [1]))
    if out is not None:
        Zo, nrb, rpb = out
        assert np.all(Zo[1, :7] == 18) and Zo[1, 7] == 0 and np.all(Zo[0] == 0) and (nrb, rpb) == (1, 16)
