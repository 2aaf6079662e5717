"""CPU tests of the persistent many-problem handle's boundary (include/pogs_amd.h: PogsAmdManyCreate, PogsAmdManySolveFn,
PogsAmdManyGetInfo, PogsAmdManyDestroy): the header compiles as C99 with a create / solve / info / destroy call, the
library exports the four symbols, pogs_amd.ManySolver.solve checks its arguments before any library call, and
PogsAmdManyCreate refuses bad arguments with the one-shot call's messages before any device work."""
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
int call_handle(const double *A, const PogsAmdFn *f, const PogsAmdFn *g, const double *x0, const double *l0, double *x,
                unsigned int *it, int *st, double *rho_final) {
  PogsAmdOptions opt = {-1, POGS_AMD_PROJ_DIRECT, 0, {0, 0, 0, 0, 0}};
  PogsAmdMany *h = NULL;
  PogsAmdManyInfo info;
  size_t m = POGS_AMD_MANY_MAX_DIM_MAX, n = POGS_AMD_MANY_MIN_DIM_MAX;
  int rc = PogsAmdManyCreate(&h, POGS_AMD_F64, ROW_MAJ, 3, m, n, A, POGS_AMD_HOST, &opt);
  if (rc != 0) return rc;
  rc = PogsAmdManySolveFn(h, f, g, NULL, POGS_AMD_MANY_COLD, NULL, NULL, 1e-4, 1e-4, 2500u, 0u, 1, 1, x, NULL, NULL,
                          NULL, NULL, it, st, rho_final);
  if (rc == 0)
    rc = PogsAmdManySolveFn(h, f, g, rho_final, POGS_AMD_MANY_WARM_GIVEN, x0, l0, 1e-4, 1e-4, 2500u, 0u, 1, 1, x, NULL,
                            NULL, NULL, NULL, it, st, NULL);
  if (rc == 0)
    rc = PogsAmdManySolveFn(h, f, g, NULL, POGS_AMD_MANY_WARM_LAST, NULL, NULL, 1e-4, 1e-4, 2500u, 0u, 1, 1, x, NULL,
                            NULL, NULL, NULL, it, st, rho_final);
  if (rc == 0) rc = PogsAmdManyGetInfo(h, &info);
  if (rc == 0 && (info.k != 3 || info.m != m || info.resident_bytes == 0 || info.problem_iters == 0)) rc = 1;
  PogsAmdManyDestroy(h);
  return rc;
}
"""


def test_header_compiles_as_c99_with_a_handle_life_cycle(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "many_handle_call.c"
    src.write_text(SNIPPET)
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), str(src)], check=True)


def test_library_exports_the_handle_entries():
    for name in ("PogsAmdManyCreate", "PogsAmdManySolveFn", "PogsAmdManyGetInfo", "PogsAmdManyDestroy"):
        assert name in _lib.ABI_SYMBOLS
        assert getattr(_lib.lib, name) is not None
    assert (_lib.MANY_COLD, _lib.MANY_WARM_GIVEN, _lib.MANY_WARM_LAST) == (0, 1, 2)
    assert "ManySolver" in pogs_amd.__all__ and pogs_amd.ManySolver is graph.ManySolver
    assert ctypes.sizeof(_lib.PogsAmdManyInfo) % 8 == 0


def _bare_solver(k, m, n, dtype=np.float64):
    """A ManySolver as its constructor leaves it, without the library: the handle is a non-NULL dummy that no call
    may reach."""
    s = object.__new__(graph.ManySolver)
    s.k, s.m, s.n, s.dtype = k, m, n, np.dtype(dtype)
    s._h = ctypes.c_void_p(1)
    return s


def test_solve_arguments_raise_before_the_library(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")

    monkeypatch.setattr(graph.lib, "PogsAmdManySolveFn", boom)
    monkeypatch.setattr(graph.lib, "PogsAmdManyDestroy", lambda h: None)
    k, m, n = 3, 20, 10
    s = _bare_solver(k, m, n)
    f, g = graph.lasso_functions(np.ones(m), 0.1, n)
    fl, _ = graph.lasso_functions(np.ones(m + 1), 0.1, n)
    _, gs = graph.lasso_functions(np.ones(m), 0.1, n - 1)
    x0, l0 = np.zeros((k, n)), np.zeros((k, m))
    bad = [
        dict(fs=[f] * 2, gs=[g] * 3),                                        # f count
        dict(fs=[f] * 3, gs=[g] * 4),                                        # g count
        dict(fs=[f, fl, f], gs=[g] * 3),                                     # f length
        dict(fs=[f] * 3, gs=[g, g, gs]),                                     # g length
        dict(fs=[f] * 3, gs=[g] * 3, rho=[1.0, 2.0]),                        # rho count
        dict(fs=[f] * 3, gs=[g] * 3, start="hot"),                           # start value
        dict(fs=[f] * 3, gs=[g] * 3, start=1),                               # start is a name, not the enum
        dict(fs=[f] * 3, gs=[g] * 3, start="warm"),                          # warm without x0, l0
        dict(fs=[f] * 3, gs=[g] * 3, start="warm", x0=x0),                   # warm with x0 alone
        dict(fs=[f] * 3, gs=[g] * 3, start="warm", l0=l0),                   # warm with l0 alone
        dict(fs=[f] * 3, gs=[g] * 3, start="warm", x0=x0[:2], l0=l0),        # x0 shape
        dict(fs=[f] * 3, gs=[g] * 3, start="warm", x0=x0, l0=l0[:, :5]),     # l0 shape
        dict(fs=[f] * 3, gs=[g] * 3, start="cold", x0=x0, l0=l0),            # stray x0 / l0
        dict(fs=[f] * 3, gs=[g] * 3, start="last", x0=x0),                   # stray x0
        dict(fs=[f] * 3, gs=[g] * 3, l0=l0),                                 # stray l0, default start
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            s.solve(**kw)
    # and a valid call does reach the library
    with pytest.raises(AssertionError, match="the library was called"):
        s.solve([f] * 3, [g] * 3, start="warm", x0=x0, l0=l0, rho=[1.0, 2.0, 3.0])
    s._h = ctypes.c_void_p()
    with pytest.raises(ValueError):
        s.solve([f] * 3, [g] * 3)                                            # a closed handle


def _raw_create(k, m, n, dtype_code=1, ord_=1, mem=0, projector=1, a_null=False):
    A = np.ones(4)
    h = ctypes.c_void_p(12345)
    opt = _lib.PogsAmdOptions(device=-1, projector=projector)
    rc = _lib.lib.PogsAmdManyCreate(ctypes.byref(h), dtype_code, ord_, k, m, n, None if a_null else A.ctypes.data, mem,
                                    ctypes.byref(opt))
    return rc, _lib.last_error(), h


def _one_shot_message(k, m, n, dtype_code=1, ord_=1, mem=0, projector=1, a_null=False):
    A = np.ones(4)
    cnt = max(k, 1)
    fa, ga = (_lib.PogsAmdFn * cnt)(), (_lib.PogsAmdFn * cnt)()
    for j in range(cnt):
        fa[j].h0, ga[j].h0 = 15, 15
    x, it, st = np.zeros(4), np.zeros(cnt, np.uint32), np.zeros(cnt, np.int32)
    opt = _lib.PogsAmdOptions(device=-1, projector=projector)
    rc = _lib.lib.PogsAmdSolveManyFn(dtype_code, ord_, k, m, n, None if a_null else A.ctypes.data, mem,
                                     ctypes.byref(opt), fa, ga, None, 1e-4, 1e-4, 10, 0, 1, 1, x.ctypes.data, None, None,
                                     None, None, it.ctypes.data, st.ctypes.data)
    assert rc == 6
    return _lib.last_error()


def _text(msg):
    """A refusal's message without the source position the library appends."""
    return msg.rsplit(" at ", 1)[0]


@pytest.mark.parametrize("kw,needle", [
    (dict(k=0, m=6, n=4), "k must be >= 1"),
    (dict(k=-2, m=6, n=4), "k must be >= 1"),
    (dict(k=1, m=6, n=4, ord_=7), "unknown ord"),
    (dict(k=1, m=6, n=4, dtype_code=7), "unknown dtype"),
    (dict(k=1, m=6, n=4, mem=5), "unknown mem"),
    (dict(k=1, m=6, n=4, a_null=True), "null A"),
    (dict(k=1, m=0, n=4), "m and n must be >= 1"),
    (dict(k=1, m=513, n=513), "POGS_AMD_MANY_MIN_DIM_MAX"),
    (dict(k=1, m=16385, n=1), "POGS_AMD_MANY_MAX_DIM_MAX"),
    (dict(k=1, m=6, n=4, projector=2), "CGLS refused"),
])
def test_create_refusals_carry_the_one_shot_messages(kw, needle, capfd):
    rc, msg, h = _raw_create(**kw)
    assert rc == 6 and needle in msg, (rc, msg)
    assert "HIP error" not in msg              # refused on the arguments, before any device work
    assert not h.value                         # *out is NULL after a refusal
    assert _text(msg) == _text(_one_shot_message(**kw))
    capfd.readouterr()


def test_null_handles_are_refused_or_ignored(capfd):
    _lib.lib.PogsAmdManyDestroy(None)
    info = _lib.PogsAmdManyInfo()
    assert _lib.lib.PogsAmdManyGetInfo(None, ctypes.byref(info)) == 6
    x, it, st = np.full(4, 7.0), np.full(1, 77, np.uint32), np.full(1, 55, np.int32)
    fa, ga = (_lib.PogsAmdFn * 1)(), (_lib.PogsAmdFn * 1)()
    rc = _lib.lib.PogsAmdManySolveFn(None, fa, ga, None, 0, None, None, 1e-4, 1e-4, 10, 0, 1, 1, x.ctypes.data, None,
                                     None, None, None, it.ctypes.data, st.ctypes.data, None)
    assert rc == 6 and "null handle" in _lib.last_error()
    assert np.all(x == 7.0) and it[0] == 77 and st[0] == 55
    capfd.readouterr()
