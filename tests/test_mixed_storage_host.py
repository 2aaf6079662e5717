"""CPU tests of the mixed-storage boundary (include/pogs_amd.h: PogsAmdOptions.storage, POGS_AMD_STORE_F32,
PogsAmdDensePassMixedCheck): the header still compiles as C99, the options struct keeps its size with `storage` where
reserved[0] sat (PogsAmdOptStorage), the enum values agree with pogs_amd._lib, the library exports the diagnostic entry, the Solver wrapper
refuses bad storage / dtype combinations before any library call, and PogsAmdCreateDense, PogsAmdCreateSparse and the
diagnostic entry refuse before any device work (no device is needed to see the refusals: they come before the first HIP
call)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pogs_amd
from pogs_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "pogs_amd.h")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "pogs_amd.h"
int create_mixed(PogsAmdSolver **out, const double *A, const PogsAmdDensePassArgs *args) {
  PogsAmdOptions opt = {-1, POGS_AMD_PROJ_DEFAULT, 0, {0, 0, 0, 0, 0}};   /* the initialiser callers have always written */
  PogsAmdOptions zeroed = {0};
  int rc;
  PogsAmdOptStorage(&opt) = POGS_AMD_STORE_F32;
  rc = PogsAmdCreateDense(out, POGS_AMD_F64, ROW_MAJ, 8, 4, A, POGS_AMD_HOST, &opt, NULL);
  rc += PogsAmdCreateDense(out, POGS_AMD_F64, ROW_MAJ, 8, 4, A, POGS_AMD_HOST, &zeroed, NULL);
  rc += PogsAmdDensePassMixedCheck(args);
  return rc + (PogsAmdOptStorage(&zeroed) == POGS_AMD_STORE_SAME ? 0 : 1);
}
"""

LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "pogs_amd.h"
int main(void) {
  PogsAmdOptions probe = {-1, 0, 0, {0, 0, 0, 0, 0}};
  printf("%d %d %d %d %d\n", (int)sizeof(PogsAmdOptions), (int)((char *)&PogsAmdOptStorage(&probe) - (char *)&probe),
         (int)offsetof(PogsAmdOptions, reserved), (int)POGS_AMD_STORE_SAME, (int)POGS_AMD_STORE_F32);
  return 0;
}
"""


def _cc():
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    return cc


def test_header_compiles_as_c99_with_the_storage_field_and_the_entry(tmp_path):
    src = tmp_path / "mixed_call.c"
    src.write_text(SNIPPET)
    subprocess.run([_cc(), "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_options_layout_is_unchanged_and_storage_sits_where_reserved0_sat(tmp_path):
    """8 ints as before: device, projector, profile, then the five that were reserved[5] -- the storage option IS reserved[0]
    (the C declaration stays an array of five: callers brace-initialise it); the ctypes struct names it"""
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT)
    subprocess.run([_cc(), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off_storage, off_reserved, same, f32 = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True,
                                                                                 text=True).stdout.split())
    assert (size, off_storage, off_reserved) == (8 * ctypes.sizeof(ctypes.c_int), 12, 12)
    assert ctypes.sizeof(_lib.PogsAmdOptions) == size
    assert _lib.PogsAmdOptions.storage.offset == off_storage and _lib.PogsAmdOptions.reserved.offset == off_storage + 4
    assert (same, f32) == (_lib.STORE_SAME, _lib.STORE_F32)


def test_enum_values_agree_with_the_header_and_the_entry_is_exported():
    text = open(HEADER).read()
    same = re.search(r"POGS_AMD_STORE_SAME\s*=\s*(\d+)", text)
    f32 = re.search(r"POGS_AMD_STORE_F32\s*=\s*(\d+)", text)
    assert same and f32 and (int(same.group(1)), int(f32.group(1))) == (_lib.STORE_SAME, _lib.STORE_F32) == (0, 1)
    assert (pogs_amd.STORE_SAME, pogs_amd.STORE_F32) == (0, 1)
    assert re.search(r"#define\s+PogsAmdOptStorage\(opt\)\s+\(\(opt\)->reserved\[POGS_AMD_OPT_STORAGE\]\)", text)
    assert re.search(r"#define\s+POGS_AMD_OPT_STORAGE\s+0\b", text)
    assert "PogsAmdDensePassMixedCheck" in _lib.ABI_SYMBOLS
    assert getattr(_lib.lib, "PogsAmdDensePassMixedCheck") is not None and callable(_lib.dense_pass_mixed_check)


def test_wrapper_refuses_bad_storage_before_the_library(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib.lib, "PogsAmdCreateDense", boom)
    monkeypatch.setattr(_lib.lib, "PogsAmdCreateSparse", boom)
    A = np.ones((8, 4))
    for dtype, storage in ((np.float32, np.float32), (np.float32, _lib.STORE_F32), (np.float32, np.float64),
                           (np.float64, np.float16), (np.float64, 2), (np.float64, -1), (np.float64, "narrow"),
                           (np.float64, True), (None, np.int32)):
        with pytest.raises(ValueError, match="storage"):
            pogs_amd.Solver(A, dtype=dtype, storage=storage)
    # the accepted spellings get as far as the library
    for dtype, storage in ((np.float64, np.float32), (np.float64, _lib.STORE_F32), (None, "float32"), (np.float64, None),
                           (np.float64, np.float64), (np.float32, None), (np.float32, _lib.STORE_SAME)):
        with pytest.raises(AssertionError, match="the library was called"):
            pogs_amd.Solver(A, dtype=dtype, storage=storage)


def _create_dense(dtype, m, n, storage, projector=_lib.PROJ_DEFAULT, dist=None):
    """PogsAmdCreateDense on a buffer that a refused call never reads; (status, handle value, message)"""
    A = np.zeros(16, np.float64)
    h = ctypes.c_void_p(1)
    opt = _lib.PogsAmdOptions(device=-1, projector=projector, profile=0, storage=storage)
    st = _lib.lib.PogsAmdCreateDense(ctypes.byref(h), dtype, _lib.ROW_MAJ, m, n, A.ctypes.data, _lib.HOST, ctypes.byref(opt),
                                     ctypes.byref(dist) if dist is not None else None)
    return st, h.value, _lib.last_error()


def test_create_dense_refuses_every_unsupported_combination_before_anything_is_built(monkeypatch):
    shards = _lib.PogsAmdDist(rank=0, world=2, m_global=16)
    cases = {
        "needs dtype POGS_AMD_F64": lambda: _create_dense(_lib.F32, 8, 4, _lib.STORE_F32),
        "needs m > n": lambda: _create_dense(_lib.F64, 4, 8, _lib.STORE_F32),
        "needs m > n ": lambda: _create_dense(_lib.F64, 4, 4, _lib.STORE_F32),
        "needs the direct projector": lambda: _create_dense(_lib.F64, 8, 4, _lib.STORE_F32, projector=_lib.PROJ_CGLS),
        "needs the direct projector ": lambda: _create_dense(_lib.F64, 8, 4, _lib.STORE_F32, projector=_lib.PROJ_CGLS_FUSED),
        "row shards are not supported": lambda: _create_dense(_lib.F64, 8, 4, _lib.STORE_F32, dist=shards),
        "the row is too wide": lambda: _create_dense(_lib.F64, 20000, 10241, _lib.STORE_F32),
        "storage: unknown value": lambda: _create_dense(_lib.F64, 8, 4, 2),
        "storage: unknown value ": lambda: _create_dense(_lib.F64, 8, 4, -1),
    }
    for msg, call in cases.items():
        st, handle, err = call()
        assert st != 0 and not handle, msg
        assert msg.strip() in err, (msg, err)
    # a windowed row: POGS_AMD_XL_LIMIT (vectors) makes a 200-column row one
    monkeypatch.setenv("POGS_AMD_XL_LIMIT", "16")
    st, handle, err = _create_dense(_lib.F64, 300, 200, _lib.STORE_F32)
    assert st != 0 and not handle and "the row is too wide (windowed" in err, err
    with pytest.raises(RuntimeError, match="needs m > n"):
        pogs_amd.Solver(np.ones((4, 8)), dtype=np.float64, storage=np.float32)


def test_create_sparse_refuses_any_storage_before_anything_is_built():
    sp = pytest.importorskip("scipy.sparse")
    A = sp.identity(8, dtype=np.float64, format="csr")
    ptr, ind = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    for storage in (_lib.STORE_F32, 2, -1):
        h = ctypes.c_void_p(1)
        opt = _lib.PogsAmdOptions(device=-1, projector=_lib.PROJ_DEFAULT, profile=0, storage=storage)
        st = _lib.lib.PogsAmdCreateSparse(ctypes.byref(h), _lib.F64, _lib.ROW_MAJ, 8, 8, 8, A.data.ctypes.data, ptr.ctypes.data,
                                          ind.ctypes.data, _lib.HOST, ctypes.byref(opt), None)
        assert st != 0 and not h.value
        assert "a sparse handle stores its matrix in its dtype" in _lib.last_error()
    with pytest.raises(RuntimeError, match="a sparse handle stores its matrix in its dtype"):
        pogs_amd.Solver(A, dtype=np.float64, storage=np.float32)


def _pass_args(rows=5, n=6, ldm=8, dtype=_lib.F64, form=_lib.PASS_ITER_FULL, functor=_lib.PASS_FN_CHEAP, force=(0, 0),
               null=()):
    """a valid argument block of PogsAmdDensePassMixedCheck (REDUCE), with the arrays in `null` left NULL"""
    keep = dict(M=np.zeros((rows, ldm), np.float32), info=np.zeros(8, np.int32), scalars=np.zeros(6))
    for k in ("x0", "x1", "tot0", "tot1"):
        keep[k] = np.zeros(n + n % 2)
    for k in ("ycur", "y12", "ytemp", "ynew", "y12s", "ytemps", "f_a", "f_b", "f_c", "f_d", "f_e"):
        keep[k] = np.zeros(rows)
    keep["f_h"] = np.zeros(rows, np.int32)
    a = _lib.PogsAmdDensePassArgs()
    a.dtype, a.form, a.functor, a.cols = dtype, form, functor, _lib.PASS_COLS_REDUCE
    a.rows, a.n, a.ldm = rows, n, ldm
    a.force_tpb, a.force_nv = force
    a.row_len, a.col_len = rows, n + n % 2
    a.rho = a.alpha = a.zs = 1.0
    for k, v in keep.items():
        if k not in null:
            setattr(a, k, v.ctypes.data)
    return a, keep


def test_the_diagnostic_entry_refuses_before_any_device_work():
    cases = {
        "dtype must be POGS_AMD_F64": dict(dtype=_lib.F32),
        "ldm must be a multiple of 4": dict(ldm=10),
        "ldm must be a multiple of 4 ": dict(ldm=4),                       # < round_up(6, 4)
        "form must be ITER_FULL or ITER_LEAN": dict(form=_lib.PASS_EXACT),
        "functor must be CHEAP or LOGISTIC": dict(functor=_lib.PASS_FN_XSIDE),
        "not a one-pass shape of the mixed plan": dict(force=(128, 2)),
        "not a one-pass shape of the mixed plan ": dict(force=(512, 6)),   # a shape of the fp64 plan, not of the mixed one
        "the shape does not hold": dict(n=300, ldm=300, force=(64, 1)),
        "null argument: M, info": dict(null=("M",)),
        "null argument: x0, x1": dict(null=("x1",)),
        "null argument: ycur, ynew, y12s, ytemps, scalars": dict(null=("ynew",)),
        "null argument: f_h, f_a .. f_e": dict(null=("f_c",)),
        "null argument: tot0, tot1": dict(null=("tot0",)),
    }
    for msg, kw in cases.items():
        a, keep = _pass_args(**kw)
        assert _lib.lib.PogsAmdDensePassMixedCheck(ctypes.byref(a)) != 0, msg
        assert msg.strip() in _lib.last_error(), (msg, _lib.last_error())
    assert _lib.lib.PogsAmdDensePassMixedCheck(None) != 0 and "null argument: args" in _lib.last_error()
    with pytest.raises(ValueError, match="M: float32"):
        _lib.dense_pass_mixed_check(_lib.PASS_ITER_LEAN, np.zeros((5, 8)), 6, dict(x0=np.zeros(6)))
