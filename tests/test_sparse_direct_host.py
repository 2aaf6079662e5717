"""CPU tests of the sparse direct projector's boundary (include/pogs_amd.h: POGS_AMD_SPARSE_DIRECT_MAX,
PogsAmdSparseGramCheck, PogsAmdTriMatvecCheck): the header compiles as C99 with calls of the new entries, the library
exports them, the cap agrees between the header and pogs_amd._lib, the numpy wrappers check shapes before any library
call, and the entries refuse bad arguments before any device work."""
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
int call_direct(PogsAmdSolver **out, const float *val, const int *ptr, const int *ind, float *G, int *info,
                const float *M, const float *x, float *y) {
  PogsAmdOptions opt = {-1, POGS_AMD_PROJ_DIRECT, 0, {0, 0, 0, 0, 0}};
  size_t k = POGS_AMD_SPARSE_DIRECT_MAX;
  int rc = PogsAmdCreateSparse(out, POGS_AMD_F32, ROW_MAJ, 4 * k, k, 8 * k, val, ptr, ind, POGS_AMD_HOST, &opt, NULL);
  rc += PogsAmdSparseGramCheck(POGS_AMD_F32, COL_MAJ, 300, 130, ptr, ind, val, 0, 64, G, 132, info);
  rc += PogsAmdTriMatvecCheck(POGS_AMD_F32, 1, 130, M, 132, x, y);
  return rc;
}
"""


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "direct_call.c"
    src.write_text(SNIPPET)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_library_exports_the_entries_and_the_cap_agrees_with_the_header():
    for sym in ("PogsAmdSparseGramCheck", "PogsAmdTriMatvecCheck"):
        assert sym in _lib.ABI_SYMBOLS and getattr(_lib.lib, sym) is not None
    text = open(HEADER).read()
    cap = re.search(r"#define\s+POGS_AMD_SPARSE_DIRECT_MAX\s+(\d+)", text)
    assert cap and int(cap.group(1)) == _lib.SPARSE_DIRECT_MAX == 16384
    assert (_lib.TRI_LOWER, _lib.TRI_UPPER) == (1, 2)
    assert callable(_lib.sparse_gram_check) and callable(_lib.tri_matvec_check)


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib.lib, "PogsAmdSparseGramCheck", boom)
    monkeypatch.setattr(_lib.lib, "PogsAmdTriMatvecCheck", boom)


def test_wrappers_check_shapes_before_the_library(no_library):
    ptr, ind, val = np.array([0, 1, 2, 3]), np.array([0, 1, 0]), np.ones(3, np.float32)
    G = np.zeros((2, 2), np.float32)
    with pytest.raises(ValueError):
        _lib.sparse_gram_check(ptr[:3], ind, val, (3, 2), G)                       # ptr length
    with pytest.raises(ValueError):
        _lib.sparse_gram_check(ptr, ind, val, (3, 2), np.zeros((3, 3), np.float32))   # G rows != K
    with pytest.raises(ValueError):
        _lib.sparse_gram_check(ptr, ind, val, (3, 2), np.zeros((2, 1), np.float32))   # ldg < K
    with pytest.raises(ValueError):
        _lib.sparse_gram_check(ptr, ind[:2], val, (3, 2), G)                       # fewer indices than ptr[-1]
    with pytest.raises(ValueError):
        _lib.sparse_gram_check(ptr, ind, val.astype(np.float64), (3, 2), G)        # two dtypes
    with pytest.raises(ValueError):
        _lib.sparse_gram_check(ptr, ind, val.astype(np.int32), (3, 2), G.astype(np.int32))   # no float dtype
    M, x = np.zeros((3, 4), np.float32), np.zeros(3, np.float32)
    with pytest.raises(ValueError):
        _lib.tri_matvec_check(1, M, np.zeros(4, np.float32))                       # x length
    with pytest.raises(ValueError):
        _lib.tri_matvec_check(1, np.zeros((3, 2), np.float32), x)                  # ldm < n
    with pytest.raises(ValueError):
        _lib.tri_matvec_check(1, M, x, np.zeros(2, np.float32))                    # y length
    with pytest.raises(ValueError):
        _lib.tri_matvec_check(1, M, x.astype(np.float64))                          # two dtypes


def test_check_entries_refuse_before_any_device_work():
    ptr, ind, val = np.array([0, 1, 2, 3]), np.array([0, 1, 0]), np.ones(3, np.float32)
    G = np.zeros((2, 4), np.float32)
    big = _lib.SPARSE_DIRECT_MAX + 1
    bad = {
        "unknown ord": lambda: _lib.sparse_gram_check(ptr, ind, val, (3, 3), np.zeros((3, 3), np.float32), ord=7),
        "window must be": lambda: _lib.sparse_gram_check(ptr, ind, val, (3, 2), G, window=96),
        "window must be 0": lambda: _lib.sparse_gram_check(ptr, ind, val, (3, 2), G, window=4096),
        "num_cu must be": lambda: _lib.sparse_gram_check(ptr, ind, val, (3, 2), G, num_cu=-1),
        "ptr\\[0\\] must be 0": lambda: _lib.sparse_gram_check(ptr + 1, np.array([0, 1, 0, 1]), np.ones(4, np.float32), (3, 2), G),
        "ptr must end": lambda: _lib.sparse_gram_check(np.zeros(4, np.int32), ind, val, (3, 2), G),
        "SPARSE_DIRECT_MAX": lambda: _lib.sparse_gram_check(np.zeros(big + 1, np.int32), ind, val, (big, big),
                                                            np.zeros((big, big), np.float32)),
        "unknown tri": lambda: _lib.tri_matvec_check(0, np.zeros((3, 4), np.float32), np.zeros(3, np.float32)),
        "ldm must be a multiple": lambda: _lib.tri_matvec_check(1, np.zeros((3, 5), np.float32), np.zeros(3, np.float32)),
    }
    for msg, call in bad.items():
        with pytest.raises(RuntimeError, match=msg):
            call()
    try:
        y = _lib.tri_matvec_check(2, np.triu(np.ones((3, 4), np.float32)), np.ones(3, np.float32))
    except RuntimeError as e:        # no device here: the call got past every argument check
        assert "HIP error" in str(e), str(e)
    else:
        assert np.array_equal(y, [3, 2, 1])


def test_a_direct_sparse_handle_beyond_the_cap_is_refused_before_anything_is_built():
    """the refusal needs no device: it comes before the handle's context is set up"""
    sp = pytest.importorskip("scipy.sparse")
    import pogs_amd

    n = _lib.SPARSE_DIRECT_MAX + 1
    with pytest.raises(RuntimeError, match="POGS_AMD_SPARSE_DIRECT_MAX = 16384"):
        pogs_amd.Solver(sp.identity(n, dtype=np.float32, format="csr"), dtype=np.float32, projector=_lib.PROJ_DIRECT)
    uid = b"POGSLOCAL:0".ljust(128, b"\0")
    with pytest.raises(RuntimeError, match="single-GPU"):
        pogs_amd.Solver(sp.identity(8, dtype=np.float32, format="csr"), dtype=np.float32, projector=_lib.PROJ_DIRECT,
                        dist=(0, 1, 8, uid))
