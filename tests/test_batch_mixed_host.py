"""CPU tests of the diagnostic entries of the float-storage batch kernels (PogsAmdBatchRowsMixedCheck,
PogsAmdBatchColsMixedCheck): their ctypes signatures are the header's, the header compiles as C99 with calls of them, and
the wrappers refuse arrays of the wrong type before the library is called."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from pogs_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRIES = ("PogsAmdBatchRowsMixedCheck", "PogsAmdBatchColsMixedCheck")

SNIPPET = r"""
#include "pogs_amd.h"
int call_mixed(const float *M, const int *act, const double *X, double *Y, const double *U, double *Z) {
  int nrb = 0, rpb = 0;
  int rc = PogsAmdBatchRowsMixedCheck(33, 30, M, 32, POGS_AMD_BATCH_MAX, act, 2, X, 30, Y, 33);
  return rc + PogsAmdBatchColsMixedCheck(33, 30, M, 32, POGS_AMD_BATCH_MAX, act, 2, U, 33, NULL, Z, 30, &nrb, &rpb);
}
"""


def _header_args(name):
    text = open(os.path.join(ROOT, "include", "pogs_amd.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype(arg):
    if "*" in arg:
        return ctypes.POINTER(ctypes.c_int) if re.match(r"int \*(nrb_used|rpb)$", arg) else ctypes.c_void_p
    return {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[arg.rsplit(" ", 1)[0]]


@pytest.mark.parametrize("name", ENTRIES)
def test_ctypes_signatures_match_the_header(name):
    assert name in _lib.ABI_SYMBOLS
    fn = getattr(_lib.lib, name)
    args = _header_args(name)
    assert [_ctype(a) for a in args] == list(fn.argtypes), args
    assert fn.restype is ctypes.c_int
    # the matrix is floats, every vector doubles: fp64 is implied, no dtype argument
    assert args[2] == "const float *M" and not any(a.endswith(" dtype") for a in args)
    assert all(a.startswith(("const double *", "double *")) for a in args if a.split("*")[-1] in ("X", "Y", "U", "Z", "add"))


def test_header_compiles_as_c99_with_calls_of_the_mixed_entries(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "batch_mixed_call.c"
    src.write_text(SNIPPET)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_wrappers_refuse_wrong_dtypes_before_the_library_is_called():
    M, X, Y = np.zeros((4, 4), np.float32), np.zeros((2, 4)), np.zeros((2, 4))
    with pytest.raises(ValueError, match="float32"):
        _lib.batch_rows_mixed_check(M.astype(np.float64), 3, X, Y, [0])
    with pytest.raises(ValueError, match="float32"):
        _lib.batch_rows_mixed_check(M, 3, X.astype(np.float32), Y, [0])
    with pytest.raises(ValueError, match="float32"):
        _lib.batch_cols_mixed_check(M, 3, X, Y, [0], add=Y.astype(np.float32))
    with pytest.raises(ValueError, match="ldz"):
        _lib.batch_cols_mixed_check(M, 3, X, Y, [0], add=np.zeros((2, 6)))
