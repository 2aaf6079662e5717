"""CPU tests of the dense fused CGLS projector's boundary (include/pogs_amd.h: POGS_AMD_PROJ_CGLS_FUSED,
PogsAmdDenseCgCheck): the header compiles as C99 with the new value and entry, the enum value agrees with pogs_amd._lib,
the library exports the entry, and the entry and PogsAmdCreateSparse refuse before any device work (no device is
needed to see the refusals: they come before the first HIP call)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from pogs_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "pogs_amd.h")

SNIPPET = r"""
#include "pogs_amd.h"
int call_fused(PogsAmdSolver **out, const float *A, const float *x0, const float *y0, float *x, float *y, double *slots) {
  PogsAmdOptions opt = {-1, POGS_AMD_PROJ_CGLS_FUSED, 0, {0, 0, 0, 0, 0}};
  int enq = 0, steps = 0;
  unsigned long long mv = 0;
  int rc = PogsAmdCreateDense(out, POGS_AMD_F32, ROW_MAJ, 8, 4, A, POGS_AMD_HOST, &opt, NULL);
  rc += PogsAmdDenseCgCheck(*out, x0, y0, x0, y0, 1e-3, 500, 1, 0, x, y, y, x, x, slots, &enq, &steps, &mv);
  return rc;
}
"""


def test_header_compiles_as_c99_with_the_new_value_and_entry(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "fused_call.c"
    src.write_text(SNIPPET)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_enum_value_agrees_with_the_header_and_the_entry_is_exported():
    text = open(HEADER).read()
    val = re.search(r"POGS_AMD_PROJ_CGLS_FUSED\s*=\s*(\d+)", text)
    assert val and int(val.group(1)) == _lib.PROJ_CGLS_FUSED == 3
    assert (_lib.PROJ_DEFAULT, _lib.PROJ_DIRECT, _lib.PROJ_CGLS) == (0, 1, 2)
    assert "PogsAmdDenseCgCheck" in _lib.ABI_SYMBOLS and getattr(_lib.lib, "PogsAmdDenseCgCheck") is not None
    assert callable(_lib.dense_cg_check)


def test_wrapper_checks_shapes_before_the_library(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib.lib, "PogsAmdDenseCgCheck", boom)
    x, y = np.zeros(4, np.float32), np.zeros(8, np.float32)
    with pytest.raises(ValueError):
        _lib.dense_cg_check(None, x, y, x[:3], y, 1e-3)                      # x_warm length
    with pytest.raises(ValueError):
        _lib.dense_cg_check(None, x, y, x, y[:7], 1e-3)                      # y_warm length
    with pytest.raises(ValueError):
        _lib.dense_cg_check(None, x, y.astype(np.float64), x, y, 1e-3)       # two dtypes


def _raw_call(handle, x0, y0, xw, yw, tol, max_steps, ahead, ysync, outs):
    slots = np.zeros(17)
    enq, steps, mv = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_ulonglong(0)
    ptr = lambda v: None if v is None else v.ctypes.data   # noqa: E731
    return _lib.lib.PogsAmdDenseCgCheck(handle, ptr(x0), ptr(y0), ptr(xw), ptr(yw), tol, max_steps, ahead, ysync,
                                        *(ptr(v) for v in outs), slots.ctypes.data, ctypes.addressof(enq),
                                        ctypes.addressof(steps), ctypes.addressof(mv))


def test_the_entry_refuses_before_any_device_work():
    x, y = np.zeros(4, np.float32), np.zeros(8, np.float32)
    outs = [x.copy(), y.copy(), y.copy(), x.copy(), x.copy()]
    cases = {
        "null argument": lambda: _raw_call(None, None, y, x, y, 1e-3, 500, 1, 0, outs),
        "null argument ": lambda: _raw_call(None, x, y, x, y, 1e-3, 500, 1, 0, outs[:4] + [None]),
        "ysync must be 0 or 1": lambda: _raw_call(None, x, y, x, y, 1e-3, 500, 1, 2, outs),
        "ahead must be >= 1": lambda: _raw_call(None, x, y, x, y, 1e-3, 500, 0, 0, outs),
        "max_steps must be >= 1": lambda: _raw_call(None, x, y, x, y, 1e-3, 0, 1, 0, outs),
        "null solver": lambda: _raw_call(None, x, y, x, y, 1e-3, 500, 1, 0, outs),
    }
    for msg, call in cases.items():
        assert call() != 0, msg
        assert msg.strip() in _lib.last_error(), (msg, _lib.last_error())
    with pytest.raises(RuntimeError, match="ahead must be >= 1"):
        _lib.dense_cg_check(None, x, y, x, y, 1e-3, ahead=0)


def test_a_fused_sparse_handle_is_refused_before_anything_is_built():
    """the refusal needs no device: it comes before the handle's context is set up, and *out is NULL"""
    sp = pytest.importorskip("scipy.sparse")
    import pogs_amd

    with pytest.raises(RuntimeError, match="POGS_AMD_PROJ_CGLS_FUSED is a dense projector"):
        pogs_amd.Solver(sp.identity(8, dtype=np.float32, format="csr"), dtype=np.float32, projector=_lib.PROJ_CGLS_FUSED)
    A = sp.identity(8, dtype=np.float32, format="csr")
    h = ctypes.c_void_p(1)
    opt = _lib.PogsAmdOptions(device=-1, projector=_lib.PROJ_CGLS_FUSED, profile=0)
    ptr, ind = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    st = _lib.lib.PogsAmdCreateSparse(ctypes.byref(h), _lib.F32, _lib.ROW_MAJ, 8, 8, 8, A.data.ctypes.data, ptr.ctypes.data,
                                      ind.ctypes.data, _lib.HOST, ctypes.byref(opt), None)
    assert st != 0 and not h.value
    assert "dense projector" in _lib.last_error()
