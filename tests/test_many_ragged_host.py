"""CPU tests of the ragged many-problem boundary (include/pogs_amd.h: PogsAmdSolveManyRaggedFn,
PogsAmdManyCreateRagged, PogsAmdManyGetShapes): the header compiles as C99 with calls of them, the library exports
them, pogs_amd.solve_many_ragged and ManySolver.from_ragged check counts, lengths and dtypes before any library call,
and the C entries refuse bad arguments before any device work."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import pogs_amd
from helpers import fn_arrays
from pogs_amd import _lib, graph

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

SNIPPET = r"""
#include "pogs_amd.h"
int call_ragged(const double *A, const PogsAmdFn *f, const PogsAmdFn *g, double *x, unsigned int *it, int *st) {
  PogsAmdOptions opt = {-1, POGS_AMD_PROJ_DIRECT, 0, {0, 0, 0, 0, 0}};
  double rho[3] = {1.0, 1.0, 1.0};
  const size_t m[3] = {7, 3, POGS_AMD_MANY_MAX_DIM_MAX}, n[3] = {3, 7, POGS_AMD_MANY_MIN_DIM_MAX};
  size_t ms[3], ns[3];
  PogsAmdMany *h = NULL;
  int rc = PogsAmdSolveManyRaggedFn(POGS_AMD_F64, ROW_MAJ, 3, m, n, A, POGS_AMD_HOST, &opt, f, g, rho, 1e-4, 1e-4, 2500u,
                                    0u, 1, 1, x, NULL, NULL, NULL, NULL, it, st);
  rc += PogsAmdManyCreateRagged(&h, POGS_AMD_F64, COL_MAJ, 3, m, n, A, POGS_AMD_HOST, &opt);
  rc += PogsAmdManyGetShapes(h, ms, ns);
  PogsAmdManyDestroy(h);
  return rc;
}
"""


def test_header_compiles_as_c99_with_the_ragged_calls(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "ragged_call.c"
    src.write_text(SNIPPET)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_library_exports_the_ragged_entries():
    for name in ("PogsAmdSolveManyRaggedFn", "PogsAmdManyCreateRagged", "PogsAmdManyGetShapes"):
        assert name in _lib.ABI_SYMBOLS
        assert getattr(_lib.lib, name) is not None
    assert callable(pogs_amd.solve_many_ragged) and "solve_many_ragged" in pogs_amd.__all__
    assert callable(pogs_amd.ManySolver.from_ragged)


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")

    for name in ("PogsAmdSolveManyRaggedFn", "PogsAmdManyCreateRagged", "PogsAmdSolveManyFn", "PogsAmdManySolveFn"):
        monkeypatch.setattr(graph.lib, name, boom)


def _problem(m, n):
    f, g = graph.lasso_functions(np.ones(m), 0.1, n)
    return np.ones((m, n)), f, g


def test_counts_lengths_and_dtypes_raise_before_the_library(no_library):
    (A0, f0, g0), (A1, f1, g1), (A2, f2, g2) = _problem(7, 3), _problem(3, 7), _problem(5, 5)
    As, fs, gs = [A0, A1, A2], [f0, f1, f2], [g0, g1, g2]
    solve = pogs_amd.solve_many_ragged
    with pytest.raises(ValueError):
        solve(As, fs[:2], gs)                                             # f count
    with pytest.raises(ValueError):
        solve(As, fs, gs + [g0])                                          # g count
    with pytest.raises(ValueError):
        solve(As, fs, gs, rho=[1.0, 2.0])                                 # rho count
    with pytest.raises(ValueError, match="problem 1"):
        solve(As, [f0, f0, f2], gs)                                       # f[1] has problem 0's length
    with pytest.raises(ValueError, match="problem 2"):
        solve(As, fs, [g0, g1, g0])                                       # g[2] has problem 0's length
    with pytest.raises(ValueError):
        solve([A0, np.ones(3), A2], fs, gs)                               # a 1-D member
    with pytest.raises(ValueError):
        solve([A0, np.ones((3, 7, 2)), A2], fs, gs)                       # a 3-D member
    with pytest.raises(ValueError):
        solve([], [], [])                                                 # no matrices
    with pytest.raises(ValueError):
        solve(As, fs, gs, dtype=np.int32)                                 # dtype
    with pytest.raises(ValueError):
        solve(np.ones(21 + 21 + 25), fs, gs, shapes=[(7, 3), (3, 7)])     # packed size against the shapes
    with pytest.raises(ValueError):
        solve(np.ones(21), [f0], [g0], shapes=[(7, 3)], order="K")        # order
    for bad in (lambda: pogs_amd.ManySolver.from_ragged([]),
                lambda: pogs_amd.ManySolver.from_ragged([A0, np.ones(3)]),
                lambda: pogs_amd.ManySolver.from_ragged([A0, np.ones((3, 7, 2))]),
                lambda: pogs_amd.ManySolver.from_ragged(As, dtype=np.int32)):
        with pytest.raises(ValueError):
            bad()


def test_the_list_form_passes_the_members_order(monkeypatch):
    """C-ordered members go row-major; a list of Fortran-ordered members goes column-major, packed in that order, and
    its one-row and one-column members (contiguous both ways) do not decide; a mixed list goes row-major."""
    seen = []

    def capture(*a):
        k = a[2]
        total = sum(a[3][j] * a[4][j] for j in range(k))
        seen.append((a[1], np.ctypeslib.as_array(ctypes.cast(a[5], ctypes.POINTER(ctypes.c_double)), (total,)).copy()))
        return 6

    monkeypatch.setattr(graph.lib, "PogsAmdSolveManyRaggedFn", capture)
    mats = [np.arange(21.0).reshape(7, 3), np.arange(15.0).reshape(3, 5), np.arange(4.0).reshape(1, 4),
            np.arange(4.0).reshape(4, 1)]
    fgs = [graph.lasso_functions(np.ones(a.shape[0]), 0.1, a.shape[1]) for a in mats]
    fs, gs = [p[0] for p in fgs], [p[1] for p in fgs]
    fort = [np.asfortranarray(a) for a in mats]
    assert fort[2].flags.c_contiguous and fort[3].flags.c_contiguous and not fort[0].flags.c_contiguous
    for As in (mats, fort, [fort[0]] + mats[1:]):
        with pytest.raises(RuntimeError):
            pogs_amd.solve_many_ragged(As, fs, gs)
    (o_c, a_c), (o_f, a_f), (o_m, _) = seen
    assert (o_c, o_f, o_m) == (int(graph.Ordering.ROW_MAJ), int(graph.Ordering.COL_MAJ), int(graph.Ordering.ROW_MAJ))
    assert np.array_equal(a_c, np.concatenate([a.ravel() for a in mats]))
    assert np.array_equal(a_f, np.concatenate([a.ravel(order="F") for a in mats]))


def test_solve_many_with_unequal_matrices_still_raises(no_library):
    (A0, f0, g0), (A1, f1, g1) = _problem(7, 3), _problem(3, 7)
    with pytest.raises(ValueError):
        pogs_amd.solve_many([A0, A1], [f0, f1], [g0, g1])


def _raw_ragged(k, ms, ns, A="own", fs="own", gs="own", dtype_code=1, ord_code=1, projector=1, m_null=False,
                n_null=False, x_null=False, it_null=False, st_null=False):
    """PogsAmdSolveManyRaggedFn as given (no Python checks): (return code, last error, x, iterations, status)."""
    cnt = max(len(ms), 1)
    dt = np.float64 if dtype_code == 1 else np.float32
    fgs = [graph.lasso_functions(np.ones(3), 0.1, 3) for _ in ms]     # tiny: never read by a refused call
    fa, ga, keep = fn_arrays([p[0] for p in fgs], [p[1] for p in fgs], dt)
    Abuf = np.ones(64, dt)
    x = np.full(64, 7.0, dt)
    it = np.full(cnt, 77, np.uint32)
    st = np.full(cnt, 55, np.int32)
    marr = (ctypes.c_size_t * cnt)(*ms) if ms else (ctypes.c_size_t * 1)()
    narr = (ctypes.c_size_t * cnt)(*ns) if ns else (ctypes.c_size_t * 1)()
    opt = _lib.PogsAmdOptions(device=-1, projector=projector)
    rc = _lib.lib.PogsAmdSolveManyRaggedFn(
        dtype_code, ord_code, k, None if m_null else marr, None if n_null else narr,
        None if A is None else Abuf.ctypes.data, 0, ctypes.byref(opt), None if fs is None else fa,
        None if gs is None else ga, None, 1e-4, 1e-4, 2500, 0, 1, 1, None if x_null else x.ctypes.data, None, None, None,
        None, None if it_null else it.ctypes.data, None if st_null else st.ctypes.data)
    return rc, _lib.last_error(), x, it, st


def _raw_create(k, ms, ns, A_null=False, dtype_code=1, ord_code=1, projector=1, m_null=False, n_null=False):
    cnt = max(len(ms), 1)
    marr = (ctypes.c_size_t * cnt)(*ms) if ms else (ctypes.c_size_t * 1)()
    narr = (ctypes.c_size_t * cnt)(*ns) if ns else (ctypes.c_size_t * 1)()
    Abuf = np.ones(64)
    h = ctypes.c_void_p(12345)
    opt = _lib.PogsAmdOptions(device=-1, projector=projector)
    rc = _lib.lib.PogsAmdManyCreateRagged(ctypes.byref(h), dtype_code, ord_code, k, None if m_null else marr,
                                          None if n_null else narr, None if A_null else Abuf.ctypes.data, 0,
                                          ctypes.byref(opt))
    return rc, _lib.last_error(), h


REFUSALS = [
    ({"k": 0}, "k must be >= 1"),
    ({"k": -1}, "k must be >= 1"),
    ({"m_null": True}, "null m or n"),
    ({"n_null": True}, "null m or n"),
    ({"dtype_code": 7}, "unknown dtype"),
    ({"ord_code": 7}, "unknown ord"),
    ({"projector": 2}, "direct projector"),
]


@pytest.mark.parametrize("kw,msg", REFUSALS)
def test_c_entries_refuse_before_any_device_work(kw, msg):
    ms, ns = [7, 3, 5], [3, 7, 5]
    kw = dict(kw)
    k = kw.pop("k", 3)
    rc, err, x, it, st = _raw_ragged(k, ms, ns, **kw)
    assert rc == 6 and msg in err, err
    assert np.all(x == 7.0) and np.all(it == 77) and np.all(st == 55)
    rc, err, h = _raw_create(k, ms, ns, **kw)
    assert rc == 6 and msg in err, err
    assert not h.value                                     # *out is NULL after a refused create


def test_c_solve_refuses_null_pointers():
    ms, ns = [7, 3, 5], [3, 7, 5]
    for kw, msg in (({"A": None}, "null A"), ({"fs": None}, "null function descriptions"),
                    ({"gs": None}, "null function descriptions"), ({"x_null": True}, "x, final_iter and status"),
                    ({"it_null": True}, "x, final_iter and status"), ({"st_null": True}, "x, final_iter and status")):
        rc, err, x, it, st = _raw_ragged(3, ms, ns, **kw)
        assert rc == 6 and msg in err, (kw, err)
        assert np.all(x == 7.0) and np.all(it == 77) and np.all(st == 55)
    rc, err, h = _raw_create(3, ms, ns, A_null=True)
    assert rc == 6 and "null A" in err and not h.value


@pytest.mark.parametrize("bad,why", [((513, 513), "MIN_DIM_MAX"), ((16385, 2), "MAX_DIM_MAX"), ((3, 16385), "MAX_DIM_MAX"),
                                     ((0, 4), "m and n must be >= 1")])
def test_a_shape_outside_the_envelope_is_named_by_its_index(bad, why):
    ms, ns = [7, 3, bad[0]], [3, 7, bad[1]]
    for rc, err in (_raw_ragged(3, ms, ns)[:2], _raw_create(3, ms, ns)[:2]):
        assert rc == 6
        assert "problem 2 of 3" in err and why in err, err
        assert "m[2] = %d" % bad[0] in err and "n[2] = %d" % bad[1] in err, err
    rc, err, x, it, st = _raw_ragged(3, ms, ns)
    assert np.all(x == 7.0) and np.all(it == 77) and np.all(st == 55)


def test_get_shapes_refuses_null_arguments():
    one = (ctypes.c_size_t * 1)()
    assert _lib.lib.PogsAmdManyGetShapes(None, one, one) == 6
    assert "null argument" in _lib.last_error()
