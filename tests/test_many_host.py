"""CPU tests of the many-problem boundary (include/pogs_amd.h: PogsAmdSolveManyFn): the header compiles as C99 with a
call of it, the library exports it, and pogs_amd.solve_many checks counts and shapes before any library call."""
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
int call_many(const double *A, const PogsAmdFn *f, const PogsAmdFn *g, double *x, unsigned int *it, int *st) {
  PogsAmdOptions opt = {-1, POGS_AMD_PROJ_DIRECT, 0, {0, 0, 0, 0, 0}};
  double rho[3] = {1.0, 1.0, 1.0};
  size_t m = POGS_AMD_MANY_MIN_DIM_MAX, n = POGS_AMD_MANY_MAX_DIM_MAX;
  return PogsAmdSolveManyFn(POGS_AMD_F64, ROW_MAJ, 3, m, n, A, POGS_AMD_HOST, &opt, f, g, rho, 1e-4, 1e-4, 2500u, 0u,
                            1, 1, x, NULL, NULL, NULL, NULL, it, st);
}
"""


def test_header_compiles_as_c99_with_a_many_call(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "many_call.c"
    src.write_text(SNIPPET)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_library_exports_the_many_entry():
    assert "PogsAmdSolveManyFn" in _lib.ABI_SYMBOLS
    assert getattr(_lib.lib, "PogsAmdSolveManyFn") is not None
    assert (_lib.MANY_MIN_DIM_MAX, _lib.MANY_MAX_DIM_MAX) == (512, 16384)
    assert callable(pogs_amd.solve_many) and "solve_many" in pogs_amd.__all__


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")

    monkeypatch.setattr(graph.lib, "PogsAmdSolveManyFn", boom)


def test_counts_and_shapes_raise_before_the_library(no_library):
    k, m, n = 3, 20, 10
    A = np.ones((k, m, n))
    f, g = graph.lasso_functions(np.ones(m), 0.1, n)
    with pytest.raises(ValueError):
        pogs_amd.solve_many(A, [f] * 2, [g] * 3)                          # f count
    with pytest.raises(ValueError):
        pogs_amd.solve_many(A, [f] * 3, [g] * 4)                          # g count
    with pytest.raises(ValueError):
        pogs_amd.solve_many(A, [f] * 3, [g] * 3, rho=[1.0, 2.0])         # rho count
    fs, _ = graph.lasso_functions(np.ones(m + 1), 0.1, n)
    with pytest.raises(ValueError):
        pogs_amd.solve_many(A, [f, fs, f], [g] * 3)                       # f length
    _, g2 = graph.lasso_functions(np.ones(m), 0.1, n - 1)
    with pytest.raises(ValueError):
        pogs_amd.solve_many(A, [f] * 3, [g, g, g2])                       # g length
    with pytest.raises(ValueError):
        pogs_amd.solve_many(np.ones((m, n)), [f], [g])                    # not (k, m, n)
    with pytest.raises(ValueError):
        pogs_amd.solve_many([np.ones((m, n)), np.ones((m, n + 1))], [f, f], [g, g])   # unequal matrices
    with pytest.raises(ValueError):
        pogs_amd.solve_many([], [], [])                                   # no matrices
    with pytest.raises(ValueError):
        pogs_amd.solve_many(A, [f] * 3, [g] * 3, dtype=np.int32)          # dtype


def test_many_setup_check_refusals():
    A = np.ones((2, 6, 4))
    bad = {
        "k must be >= 1": lambda: _lib.many_setup_check(np.ones((0, 6, 4))),
        "unknown ord": lambda: _lib.many_setup_check(A, ord=7),
        "m and n must be >= 1": lambda: _lib.many_setup_check(np.ones((1, 0, 4))),
        "MIN_DIM_MAX": lambda: _lib.many_setup_check(np.ones((1, 513, 513), np.float32)),
        "MAX_DIM_MAX": lambda: _lib.many_setup_check(np.ones((1, 16385, 1), np.float32)),
    }
    for msg, call in bad.items():
        with pytest.raises(RuntimeError, match=msg):
            call()
        assert msg in _lib.last_error()
    rng = np.random.default_rng(0)
    try:
        out = _lib.many_setup_check(rng.standard_normal((2, 6, 4)))
    except RuntimeError as e:        # no device here: the call got past every argument check
        assert "HIP error" in str(e), str(e)
    else:
        assert np.all(np.isfinite(out["W"])) and np.all(out["nrmA"] > 0)
