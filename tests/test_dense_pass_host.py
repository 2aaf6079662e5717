"""CPU tests of the boundary of PogsAmdDensePassCheck (include/pogs_amd.h, Part 3): the header compiles as C99 with a call
of the entry, the library exports it, the numpy wrapper checks lengths and dtypes before any library call, and the entry
refuses bad arguments before any device work, with a message that names the argument."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pogs_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

SNIPPET = r"""
#include <string.h>
#include "pogs_amd.h"
int call_pass(const double *M, const double *x0, double *tot0, int *info) {
  PogsAmdDensePassArgs a;
  memset(&a, 0, sizeof a);
  a.dtype = POGS_AMD_F64; a.form = POGS_AMD_PASS_W_SWEEP; a.functor = POGS_AMD_PASS_FN_CHEAP;
  a.cols = POGS_AMD_PASS_COLS_REDUCE;
  a.rows = 30; a.n = 30; a.M = M; a.ldm = 32; a.row_len = 30; a.col_len = 30;
  a.x0 = x0; a.tot0 = tot0; a.info = info;
  return PogsAmdDensePassCheck(&a);
}
"""


def test_header_compiles_as_c99_with_the_entry(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "pass_call.c"
    src.write_text(SNIPPET)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_library_exports_the_entry_and_the_codes_agree_with_the_header():
    assert "PogsAmdDensePassCheck" in _lib.ABI_SYMBOLS and _lib.lib.PogsAmdDensePassCheck is not None
    text = open(os.path.join(ROOT, "include", "pogs_amd.h")).read()
    for name, val in (("PRE_ACC", 0), ("ITER_FULL", 1), ("ITER_LEAN", 2), ("EXACT", 3), ("W_SWEEP", 4), ("FN_CHEAP", 0),
                      ("FN_LOGISTIC", 1), ("FN_XSIDE", 2), ("COLS_REDUCE", 0), ("COLS_PRE", 1), ("COLS_PRE_ONE", 2),
                      ("COLS_PACK", 3)):
        assert "POGS_AMD_PASS_%s = %d" % (name, val) in text
        assert getattr(_lib, "PASS_" + name) == val
    # the ctypes struct has the fields of the C struct, in its order
    body = text[text.index("typedef struct PogsAmdDensePassArgs {"):text.index("} PogsAmdDensePassArgs;")]
    body = body.split("{", 1)[1]
    import re
    names = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = decl.strip()
        if decl:
            names += [t.strip().lstrip("*").split()[-1].lstrip("*") for t in decl.split(",")]
    assert names == [k for k, _ in _lib.PogsAmdDensePassArgs._fields_]


def _iter_vec(dt, rows=5, n=8, row_len=None, col_len=None):
    row_len, col_len = row_len or rows, col_len or n
    z = lambda k: np.zeros(k, dt)
    vec = dict(x0=z(col_len), x1=z(col_len), ycur=z(row_len), y12=z(row_len), ytemp=z(row_len), ynew=z(row_len),
               y12s=z(row_len), ytemps=z(row_len), tot0=z(col_len), tot1=z(col_len))
    f = dict(h=np.full(row_len, 15, np.int32), a=np.ones(row_len, dt), b=z(row_len), c=np.ones(row_len, dt), d=z(row_len),
             e=z(row_len))
    return np.zeros((rows, n), dt), vec, f


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib.lib, "PogsAmdDensePassCheck", boom)


def test_wrapper_checks_lengths_and_dtypes_before_the_library(no_library):
    M, vec, f = _iter_vec(np.float64)
    call = lambda v, ff=f, MM=M, n=8: _lib.dense_pass_check(_lib.PASS_ITER_FULL, MM, n, v, f=ff)
    with pytest.raises(ValueError, match="row-side"):
        call(dict(vec, ynew=np.zeros(6)))                       # two row lengths
    with pytest.raises(ValueError, match="row-side"):
        call({k: (v[:4] if k in _lib.PASS_ROW_VECTORS else v) for k, v in vec.items()},
             {k: v[:4] for k, v in f.items()})                  # shorter than rows
    with pytest.raises(ValueError, match="row-side"):
        call(vec, {k: v[:4] for k, v in f.items()})             # f of another length
    with pytest.raises(ValueError, match="column-side"):
        call(dict(vec, tot1=np.zeros(10)))                      # two column lengths
    with pytest.raises(ValueError, match="column-side"):
        call(vec, n=9)                                          # shorter than n_pad
    with pytest.raises(ValueError, match="one dtype"):
        call(dict(vec, x0=np.zeros(8, np.float32)))             # mixed dtypes
    with pytest.raises(ValueError, match="one dtype"):
        call(vec, dict(f, a=np.ones(5, np.float32)))
    with pytest.raises(ValueError, match="one dtype"):
        call(vec, MM=M.astype(np.int32))
    with pytest.raises(ValueError, match="dots"):
        call(dict(vec, dots=np.zeros(5)))
    with pytest.raises(ValueError, match="pack"):
        call(dict(vec, pack=np.zeros(8)))
    with pytest.raises(ValueError, match="unknown vectors"):
        call(dict(vec, ynext=np.zeros(5)))
    with pytest.raises(ValueError, match="M"):
        call(vec, MM=np.zeros(8))


def test_entry_refuses_before_any_device_work():
    for dt in (np.float32, np.float64):
        V = 16 // np.dtype(dt).itemsize
        M, vec, f = _iter_vec(dt)
        P = _lib
        bad = {
            "ldm must be a multiple": lambda: P.dense_pass_check(P.PASS_ITER_FULL, np.zeros((5, 8 + V - 1), dt), 8, vec, f=f),
            "unknown form": lambda: P.dense_pass_check(7, M, 8, vec, f=f),
            "unknown functor": lambda: P.dense_pass_check(P.PASS_ITER_FULL, M, 8, vec, f=f, functor=3),
            "unknown cols": lambda: P.dense_pass_check(P.PASS_ITER_FULL, M, 8, vec, f=f, cols=4),
            "num_cu must be": lambda: P.dense_pass_check(P.PASS_ITER_FULL, M, 8, vec, f=f, num_cu=-1),
            "force_tpb, force_nv: not a shape": lambda: P.dense_pass_check(P.PASS_ITER_FULL, M, 8, vec, f=f, force=(256, 7)),
            "force_tpb, force_nv: not a shape of": lambda: P.dense_pass_check(P.PASS_ITER_FULL, M, 8, vec, f=f, force=(0, 2)),
            "force_tpb, force_nv: the shape does not hold n_pad": lambda: P.dense_pass_check(
                P.PASS_ITER_FULL, np.zeros((5, 64 * V + V), dt), 64 * V + 1,
                dict(vec, x0=np.zeros(64 * V + V, dt), x1=np.zeros(64 * V + V, dt), tot0=np.zeros(64 * V + V, dt),
                     tot1=np.zeros(64 * V + V, dt)), f=f, force=(64, 1)),
            "form: the one-pass kernels": lambda: P.dense_pass_check(P.PASS_ITER_FULL, M, 8, vec, f=f, force=(1024, 6)),
            "null argument: x0, x1": lambda: P.dense_pass_check(P.PASS_ITER_FULL, M, 8, {k: v for k, v in vec.items() if k != "x1"}, f=f),
            "null argument: f_h": lambda: P.dense_pass_check(P.PASS_ITER_FULL, M, 8, vec),
            "null argument: tot0, tot1": lambda: P.dense_pass_check(P.PASS_ITER_FULL, M, 8, {k: v for k, v in vec.items() if k != "tot1"}, f=f),
            "null argument: pack": lambda: P.dense_pass_check(P.PASS_ITER_FULL, M, 8, vec, f=f, cols=P.PASS_COLS_PACK),
            "null argument: g_h": lambda: P.dense_pass_check(P.PASS_ITER_FULL, M, 8, vec, f=f, cols=P.PASS_COLS_PRE),
            "functor LOGISTIC: form PRE_ACC": lambda: P.dense_pass_check(P.PASS_PRE_ACC, M, 8, vec, functor=P.PASS_FN_LOGISTIC),
            "form W_SWEEP needs rows == n": lambda: P.dense_pass_check(P.PASS_W_SWEEP, M, 8, vec),
            "functor XSIDE has no lean form": lambda: P.dense_pass_check(P.PASS_ITER_LEAN, M.astype(np.float64), 8,
                                                                        {k: v.astype(np.float64) for k, v in vec.items()},
                                                                        f={k: (v if k == "h" else v.astype(np.float64)) for k, v in f.items()},
                                                                        functor=P.PASS_FN_XSIDE),
        }
        if dt == np.float32:
            bad["form ITER_LEAN is built for fp64 only"] = lambda: P.dense_pass_check(P.PASS_ITER_LEAN, M, 8, vec, f=f)
        else:
            bad["cols PACK: a lean pass"] = lambda: P.dense_pass_check(P.PASS_ITER_LEAN, M, 8, dict(vec, pack=np.zeros(22)), f=f,
                                                                      cols=P.PASS_COLS_PACK)
        for msg, call in bad.items():
            with pytest.raises(RuntimeError, match=msg):
                call()
        try:
            out = P.dense_pass_check(P.PASS_ITER_FULL, M, 8, vec, f=f, num_cu=1)
        except RuntimeError as e:        # no device here: the call got past every argument check
            assert "HIP error" in str(e) or "hip" in str(e).lower(), str(e)
        else:
            assert out["info"]["tpb"] == 64 and out["info"]["nv"] == 1
