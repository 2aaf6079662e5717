"""CPU tests of the boundary of mixed storage with the one-pass CGLS projector (include/pogs_amd.h:
PogsAmdCreateDenseMixed, PogsAmdStreamMixedCheck): the header still compiles as C99 with both entries, the library
exports them, every refusal of both comes before any device work and names its reason (no device is needed to see
them), the Solver wrapper routes storage=float32 with PROJ_CGLS_FUSED to the new entry and everything else to
PogsAmdCreateDense as before, and PogsAmdCreateDense keeps refusing the combination."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import pogs_amd
from pogs_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

SNIPPET = r"""
#include <stddef.h>
#include "pogs_amd.h"
int create_and_check(PogsAmdSolver **out, const double *A, const float *M, double *v, int *info) {
  PogsAmdOptions opt = {-1, POGS_AMD_PROJ_CGLS_FUSED, 0, {0, 0, 0, 0, 0}};
  int rc = PogsAmdCreateDenseMixed(out, ROW_MAJ, 4, 8, A, POGS_AMD_HOST, &opt);
  rc += PogsAmdStreamMixedCheck(POGS_AMD_STREAM_MIXED_DOT_ACC, 4, 8, M, 8, 0, 0, 0, v, NULL, 0.0, v, v, v, NULL, 0, info);
  return rc + (int)POGS_AMD_STREAM_MIXED_ACC + (int)POGS_AMD_STREAM_MIXED_DOT;
}
"""


def test_header_compiles_as_c99_with_both_entries_and_the_library_exports_them(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "dense_mixed_call.c"
    src.write_text(SNIPPET)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    for name in ("PogsAmdCreateDenseMixed", "PogsAmdStreamMixedCheck"):
        assert name in _lib.ABI_SYMBOLS and getattr(_lib.lib, name) is not None
    assert callable(_lib.stream_mixed_check)
    assert (_lib.STREAM_MIXED_ACC, _lib.STREAM_MIXED_DOT_ACC, _lib.STREAM_MIXED_DOT) == (0, 1, 2)


def _create_mixed(m=8, n=4, projector=_lib.PROJ_CGLS_FUSED, storage=_lib.STORE_F32, ord_=_lib.ROW_MAJ, mem=_lib.HOST,
                  null=()):
    """PogsAmdCreateDenseMixed on a buffer that a refused call never reads; (status, handle value, message)"""
    A = np.zeros(16, np.float64)
    h = ctypes.c_void_p(1)
    opt = _lib.PogsAmdOptions(device=-1, projector=projector, profile=0, storage=storage)
    st = _lib.lib.PogsAmdCreateDenseMixed(None if "out" in null else ctypes.byref(h), ord_, m, n,
                                          None if "A" in null else A.ctypes.data, mem,
                                          None if "opt" in null else ctypes.byref(opt))
    return st, (None if "out" in null else h.value), _lib.last_error()


def test_create_dense_mixed_refuses_before_anything_is_built(monkeypatch):
    cases = {
        "null argument: out": dict(null=("out",)),
        "null argument: A and opt are required": dict(null=("A",)),
        "null argument: A and opt are required ": dict(null=("opt",)),
        "unknown ord": dict(ord_=7),
        "unknown mem": dict(mem=7),
        "bad dimensions": dict(m=0),
        "bad dimensions ": dict(n=0),
        "bad dimensions  ": dict(m=1 << 31),
        "opt->projector must be POGS_AMD_PROJ_CGLS_FUSED": dict(projector=_lib.PROJ_DEFAULT),
        "opt->projector must be POGS_AMD_PROJ_CGLS_FUSED ": dict(projector=_lib.PROJ_DIRECT),
        "opt->projector must be POGS_AMD_PROJ_CGLS_FUSED  ": dict(projector=_lib.PROJ_CGLS),
        "the row is too wide for a mixed dense handle": dict(m=20, n=10241),
        "storage: unknown value": dict(storage=2),
        "storage: unknown value ": dict(storage=-1),
    }
    for msg, kw in cases.items():
        st, handle, err = _create_mixed(**kw)
        assert st != 0 and not handle, msg
        assert msg.strip() in err, (msg, err)
    # a windowed row: POGS_AMD_XL_LIMIT (vectors) makes a 200-column row one
    monkeypatch.setenv("POGS_AMD_XL_LIMIT", "16")
    st, handle, err = _create_mixed(m=30, n=200)
    assert st != 0 and not handle and "the row is too wide for a mixed dense handle (windowed" in err, err


def test_create_dense_keeps_refusing_float_storage_with_cgls_fused():
    A = np.zeros(32, np.float64)
    for m, n, msg in ((8, 4, "needs the direct projector (not CGLS or CGLS_FUSED)"), (4, 8, "needs m > n")):
        h = ctypes.c_void_p(1)
        opt = _lib.PogsAmdOptions(device=-1, projector=_lib.PROJ_CGLS_FUSED, profile=0, storage=_lib.STORE_F32)
        st = _lib.lib.PogsAmdCreateDense(ctypes.byref(h), _lib.F64, _lib.ROW_MAJ, m, n, A.ctypes.data, _lib.HOST, ctypes.byref(opt), None)
        assert st != 0 and not h.value and msg in _lib.last_error(), _lib.last_error()


def test_solver_routes_float_storage_with_cgls_fused_to_the_new_entry(monkeypatch):
    calls = []

    def stub(name):
        def f(*a):
            calls.append(name)
            raise AssertionError("stop at " + name)
        return f

    monkeypatch.setattr(_lib.lib, "PogsAmdCreateDense", stub("dense"))
    monkeypatch.setattr(_lib.lib, "PogsAmdCreateDenseMixed", stub("mixed"))
    monkeypatch.setattr(_lib, "check_device_pointer_interop", lambda: None)
    tall, wide = np.ones((8, 4)), np.ones((4, 8))
    want = [
        (dict(A=tall, storage=np.float32, projector=_lib.PROJ_CGLS_FUSED), "mixed"),
        (dict(A=wide, storage=np.float32, projector=_lib.PROJ_CGLS_FUSED), "mixed"),
        (dict(A=wide, storage=_lib.STORE_F32, projector=_lib.PROJ_CGLS_FUSED), "mixed"),
        (dict(A=1 << 20, shape=(4, 8), device_ptr=True, storage=np.float32, projector=_lib.PROJ_CGLS_FUSED), "mixed"),
        (dict(A=tall, storage=np.float32), "dense"),
        (dict(A=tall, storage=np.float32, projector=_lib.PROJ_DIRECT), "dense"),
        (dict(A=tall, storage=np.float32, projector=_lib.PROJ_CGLS), "dense"),
        (dict(A=wide, storage=np.float32), "dense"),
        (dict(A=tall, projector=_lib.PROJ_CGLS_FUSED), "dense"),
        (dict(A=tall, storage=np.float64, projector=_lib.PROJ_CGLS_FUSED), "dense"),
    ]
    for kw, entry in want:
        kw = dict(kw)
        A = kw.pop("A")
        with pytest.raises(AssertionError, match="stop at " + entry):
            pogs_amd.Solver(A, dtype=np.float64, **kw)
    assert calls == [e for _, e in want]
    # a float32 solver with storage=float32 is refused by the wrapper itself, whatever the projector
    with pytest.raises(ValueError, match="storage"):
        pogs_amd.Solver(tall, dtype=np.float32, storage=np.float32, projector=_lib.PROJ_CGLS_FUSED)


def test_wide_float_storage_without_the_projector_keeps_raising_needs_m_gt_n():
    with pytest.raises(RuntimeError, match="needs m > n"):
        pogs_amd.Solver(np.ones((4, 8)), dtype=np.float64, storage=np.float32)
    with pytest.raises(RuntimeError, match="needs the direct projector"):
        pogs_amd.Solver(np.ones((8, 4)), dtype=np.float64, storage=np.float32, projector=_lib.PROJ_CGLS)


def _check(form=_lib.STREAM_MIXED_DOT_ACC, rows=5, n=6, ldm=8, num_cu=1, force=(0, 0), null=(), partials_len=0):
    keep = dict(M=np.zeros((rows, ldm), np.float32), x=np.zeros(n + n % 2), u=np.zeros(rows), q=np.zeros(rows),
                tot=np.zeros(n + n % 2), scalars=np.zeros(2), partials=np.zeros(max(partials_len, 1)), info=np.zeros(8, np.int32))
    p = {k: (None if k in null else v.ctypes.data) for k, v in keep.items()}
    if not partials_len:
        p["partials"] = None
    st = _lib.lib.PogsAmdStreamMixedCheck(form, rows, n, p["M"], ldm, num_cu, force[0], force[1], p["x"], p["u"], 0.0, p["q"],
                                          p["tot"], p["scalars"], p["partials"], partials_len, p["info"])
    return st, _lib.last_error()


def test_the_diagnostic_entry_refuses_before_any_device_work():
    cases = {
        "form must be ACC, DOT_ACC or DOT": dict(form=3),
        "form must be ACC, DOT_ACC or DOT ": dict(form=-1),
        "rows and n must be >= 1": dict(rows=0),
        "rows and n must be >= 1 ": dict(n=0),
        "null argument: M, info": dict(null=("M",)),
        "null argument: M, info ": dict(null=("info",)),
        "ldm must be a multiple of 4": dict(ldm=10),
        "ldm must be a multiple of 4 ": dict(ldm=4),                       # < round_up(6, 4)
        "num_cu must be in [0, 1024]": dict(num_cu=-1),
        "num_cu must be in [0, 1024] ": dict(num_cu=1025),
        "not a one-pass shape of the mixed plan": dict(force=(128, 2)),
        "not a one-pass shape of the mixed plan ": dict(force=(512, 6)),   # a shape of the fp64 plan, not of the mixed one
        "the shape does not hold": dict(n=300, ldm=300, force=(64, 1)),
        "the row fits no one-pass shape of the mixed plan": dict(n=10241, ldm=10244, rows=1),
        "null argument: x, q, scalars": dict(null=("x",)),
        "null argument: x, q, scalars ": dict(form=_lib.STREAM_MIXED_DOT, null=("q",)),
        "null argument: x, q, scalars  ": dict(null=("scalars",)),
        "null argument: u (form ACC)": dict(form=_lib.STREAM_MIXED_ACC, null=("u",)),
        "null argument: tot": dict(null=("tot",)),
        "null argument: tot ": dict(form=_lib.STREAM_MIXED_ACC, null=("tot",)),
        "partials: form DOT forms no column partials": dict(form=_lib.STREAM_MIXED_DOT, partials_len=64),
        "partials_len must be >= grid * round_up(n, 2)": dict(partials_len=5),   # num_cu given: no device is asked
    }
    for msg, kw in cases.items():
        st, err = _check(**kw)
        assert st != 0, msg
        assert msg.strip() in err, (msg, err)
    with pytest.raises(ValueError, match="M: float32"):
        _lib.stream_mixed_check(_lib.STREAM_MIXED_DOT, np.zeros((5, 8)), 6, x=np.zeros(6))
    with pytest.raises(ValueError, match="vector of 6 float64"):
        _lib.stream_mixed_check(_lib.STREAM_MIXED_DOT, np.zeros((5, 8), np.float32), 6, x=np.zeros(7))
