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
