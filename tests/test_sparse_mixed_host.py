"""CPU tests of the mixed-storage SPARSE boundary (include/pogs_amd.h: PogsAmdCreateSparseMixed, PogsAmdSpmvMixedCheck;
Solver(values=np.float32)): the header compiles as C99 with both entries, both names are in ABI_SYMBOLS and exported,
PogsAmdCreateSparseMixed refuses before anything is built (no device is needed to see a refusal: it comes before the
first HIP call), and the Solver wrapper refuses bad `values` combinations before any library call while the accepted
spellings reach the new entry."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import pogs_amd
from pogs_amd import _lib

sp = pytest.importorskip("scipy.sparse")

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

SNIPPET = r"""
#include <stddef.h>
#include "pogs_amd.h"
int both(PogsAmdSolver **out, const double *val, const int *ptr, const int *ind, const double *x, double *y, int *info) {
  PogsAmdOptions opt = {-1, POGS_AMD_PROJ_DIRECT, 0, {0, 0, 0, 0, 0}};
  double sumsq = 0.0;
  int rc = PogsAmdCreateSparseMixed(out, ROW_MAJ, 8, 8, 8, val, ptr, ind, POGS_AMD_HOST, &opt);
  rc += PogsAmdCreateSparseMixed(out, COL_MAJ, 8, 8, 8, val, ptr, ind, POGS_AMD_DEVICE, NULL);
  rc += PogsAmdSpmvMixedCheck(ROW_MAJ, 8, 8, ptr, ind, val, 0, 0, 0, 0, 1.0, 'n', 0.0, 1.0, 0.0, x, 8, y, 8, &sumsq, info);
  return rc;
}
"""


def test_header_compiles_as_c99_with_both_entries(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "sparse_mixed_call.c"
    src.write_text(SNIPPET)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_both_names_are_listed_and_exported():
    for name in ("PogsAmdCreateSparseMixed", "PogsAmdSpmvMixedCheck"):
        assert name in _lib.ABI_SYMBOLS
        assert getattr(_lib.lib, name) is not None
    assert callable(_lib.spmv_mixed_check)
    text = open(os.path.join(ROOT, "include", "pogs_amd.h")).read()
    assert "int PogsAmdCreateSparseMixed(PogsAmdSolver **out, enum ORD ord," in text
    assert "int PogsAmdSpmvMixedCheck(enum ORD ord," in text


def _identity():
    A = sp.identity(8, dtype=np.float64, format="csr")
    return A, A.indptr.astype(np.int32), A.indices.astype(np.int32)


def _create(m=8, n=8, nnz=8, ord=_lib.ROW_MAJ, mem=_lib.HOST, projector=_lib.PROJ_DEFAULT, storage=0, null=(), opt=True,
            out=True):
    """PogsAmdCreateSparseMixed on an 8 x 8 identity that a refused call never reads; (status, handle value, message)"""
    A, ptr, ind = _identity()
    h = ctypes.c_void_p(1)
    o = _lib.PogsAmdOptions(device=-1, projector=projector, profile=0, storage=storage)
    arg = {"data": A.data.ctypes.data, "ptr": ptr.ctypes.data, "ind": ind.ctypes.data}
    for k in null:
        arg[k] = None
    st = _lib.lib.PogsAmdCreateSparseMixed(ctypes.byref(h) if out else None, ord, m, n, nnz, arg["data"], arg["ptr"], arg["ind"],
                                           mem, ctypes.byref(o) if opt else None)
    return st, h.value, _lib.last_error()


def test_create_sparse_mixed_refuses_before_anything_is_built():
    big = _lib.SPARSE_DIRECT_MAX + 1
    cases = {
        "null argument": dict(null=("data",)),
        "null argument ": dict(null=("ptr",)),
        "null argument  ": dict(null=("ind",)),
        "unknown ord": dict(ord=7),
        "unknown mem": dict(mem=5),
        "unknown mem ": dict(mem=-1),
        "bad dimensions": dict(m=0),
        "bad dimensions ": dict(n=0),
        "bad dimensions  ": dict(m=1 << 31),
        "bad dimensions   ": dict(nnz=1 << 31),
        "POGS_AMD_PROJ_CGLS_FUSED is a dense projector": dict(projector=_lib.PROJ_CGLS_FUSED),
        "needs min(m, n) <= POGS_AMD_SPARSE_DIRECT_MAX": dict(m=big, n=big + 5, projector=_lib.PROJ_DIRECT),
        "storage: unknown value": dict(storage=2),
        "storage: unknown value ": dict(storage=-1),
    }
    for msg, kw in cases.items():
        st, handle, err = _create(**kw)
        assert st != 0 and not handle, (msg, st, handle)
        assert msg.strip() in err, (msg, err)
    st, handle, err = _create(out=False)
    assert st != 0 and "null argument" in err, err
    # the refusals that depend on the options come with the options' values only: a NULL opt passes them (and the
    # unknown ord is still refused first)
    st, handle, err = _create(ord=7, opt=False)
    assert st != 0 and not handle and "unknown ord" in err


def _boom(name):
    def boom(*a):
        raise AssertionError("the library was called: " + name)
    return boom


def test_wrapper_refuses_bad_values_before_the_library(monkeypatch):
    for name in ("PogsAmdCreateDense", "PogsAmdCreateSparse", "PogsAmdCreateSparseMixed"):
        monkeypatch.setattr(_lib.lib, name, _boom(name))
    A, _, _ = _identity()
    D = np.ones((8, 4))
    # any other value
    for values in (np.float16, np.int32, "narrow", 1, True, _lib.STORE_F32, 4):
        with pytest.raises(ValueError, match="values must be"):
            pogs_amd.Solver(A, dtype=np.float64, values=values)
    # float64 values under a float32 solver are not a thing either
    with pytest.raises(ValueError, match="values must be"):
        pogs_amd.Solver(A, dtype=np.float32, values=np.float64)
    # a dense matrix: the message points to storage=
    with pytest.raises(ValueError, match=r"storage=np\.float32"):
        pogs_amd.Solver(D, dtype=np.float64, values=np.float32)
    with pytest.raises(ValueError, match=r"storage=np\.float32"):
        pogs_amd.Solver(12345, dtype=np.float64, shape=(8, 4), device_ptr=True, values=np.float32)
    # dtype float32
    with pytest.raises(ValueError, match="needs dtype=float64"):
        pogs_amd.Solver(A, dtype=np.float32, values=np.float32)
    # row shards
    with pytest.raises(ValueError, match="single-GPU"):
        pogs_amd.Solver(A, dtype=np.float64, values=np.float32, dist=(0, 2, 16, b"\0" * _lib.UNIQUE_ID_BYTES))
    # together with storage=
    for storage in (np.float32, np.float64, _lib.STORE_SAME, _lib.STORE_F32):
        with pytest.raises(ValueError, match="do not combine"):
            pogs_amd.Solver(A, dtype=np.float64, values=np.float32, storage=storage)


def test_accepted_spellings_reach_the_new_entry(monkeypatch):
    monkeypatch.setattr(_lib, "check_device_pointer_interop", lambda: None)
    for name in ("PogsAmdCreateDense", "PogsAmdCreateSparse", "PogsAmdCreateSparseMixed"):
        monkeypatch.setattr(_lib.lib, name, _boom(name))
    A, _, _ = _identity()
    for dtype, values in ((np.float64, np.float32), (None, np.float32), (np.float64, "float32"), (None, np.dtype(np.float32))):
        with pytest.raises(AssertionError, match="the library was called: PogsAmdCreateSparseMixed"):
            pogs_amd.Solver(A, dtype=dtype, values=values)
        with pytest.raises(AssertionError, match="the library was called: PogsAmdCreateSparseMixed"):
            pogs_amd.Solver((4096, 8192, 12288, 8), dtype=dtype, shape=(8, 8), device_ptr=True, values=values)
    for projector in (_lib.PROJ_CGLS, _lib.PROJ_DIRECT):
        with pytest.raises(AssertionError, match="the library was called: PogsAmdCreateSparseMixed"):
            pogs_amd.Solver(A, dtype=np.float64, values=np.float32, projector=projector)
    # None and float64 are the plain handle: the existing entry, as before
    for dtype, values in ((np.float64, None), (np.float64, np.float64), (None, "float64"), (np.float32, None)):
        with pytest.raises(AssertionError, match="the library was called: PogsAmdCreateSparse$"):
            pogs_amd.Solver(A, dtype=dtype, values=values)
    with pytest.raises(AssertionError, match="the library was called: PogsAmdCreateDense"):
        pogs_amd.Solver(np.ones((8, 4)), dtype=np.float64, values=np.float64)


def test_the_new_entry_receives_the_matrix_and_storage_reads_store_f32(monkeypatch):
    seen = {}

    def fake(out, ord, m, n, nnz, data, ptr, ind, mem, opt):
        seen.update(ord=ord, m=m, n=n, nnz=nnz, mem=mem,
                    data=np.ctypeslib.as_array(ctypes.cast(data, ctypes.POINTER(ctypes.c_double)), (nnz,)).copy())
        return 1   # a failed create: no handle is kept

    monkeypatch.setattr(_lib.lib, "PogsAmdCreateSparseMixed", fake)
    A = sp.random(8, 6, density=0.5, format="csr", random_state=3, dtype=np.float64)
    with pytest.raises(RuntimeError, match="solver creation failed"):
        pogs_amd.Solver(A, values=np.float32)
    assert (seen["ord"], seen["m"], seen["n"], seen["nnz"], seen["mem"]) == (_lib.ROW_MAJ, 8, 6, A.nnz, _lib.HOST)
    assert np.array_equal(seen["data"], A.data)   # float64 as given: the library rounds after the equilibration

    monkeypatch.setattr(_lib.lib, "PogsAmdCreateSparseMixed", lambda *a: 0)   # (the handle stays NULL: nothing to destroy)
    s = pogs_amd.Solver(A, values=np.float32)
    assert s.storage == _lib.STORE_F32 and s.sparse and s.dtype == np.float64
