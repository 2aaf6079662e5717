"""CPU tests of the boundary of PogsAmdVecCheck (include/pogs_amd.h, Part 3): the header compiles as C99 with a call of
the entry, the library exports it, the op codes agree between the header and the wrapper, the ctypes struct has the C
struct's fields, the numpy wrapper checks lengths and dtypes before any library call, and the entry refuses bad arguments
before any device work, with a message that names the argument."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from pogs_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

SNIPPET = r"""
#include <string.h>
#include "pogs_amd.h"
int call_vec(const double *x, double *y, int *info) {
  PogsAmdVecArgs a;
  memset(&a, 0, sizeof a);
  a.dtype = POGS_AMD_F64; a.op = POGS_AMD_VEC_AXPBY;
  a.n_x = 30; a.len_x = 33; a.s0 = 2.0; a.s1 = 0.0;
  a.x_in[0] = x; a.x_out[0] = y; a.info = info;
  return PogsAmdVecCheck(&a);
}
"""


def test_header_compiles_as_c99_with_the_entry(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "vec_call.c"
    src.write_text(SNIPPET)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_library_exports_the_entry_and_the_codes_agree_with_the_header():
    assert "PogsAmdVecCheck" in _lib.ABI_SYMBOLS and _lib.lib.PogsAmdVecCheck is not None
    text = open(os.path.join(ROOT, "include", "pogs_amd.h")).read()
    for val, name in enumerate(_lib.VEC_OPS):
        assert "POGS_AMD_VEC_%s = %d" % (name, val) in text
        assert getattr(_lib, "VEC_" + name) == val
    assert len(re.findall(r"POGS_AMD_VEC_[A-Z_]+ = \d+", text)) == len(_lib.VEC_OPS)
    assert "#define POGS_AMD_VEC_SCALARS %d" % _lib.VEC_SCALARS in text
    # the slot numbers the wrapper restates are those of the engine's enum
    enum = open(os.path.join(ROOT, "pogs_amd", "csrc", "vec_kernels.h")).read()
    enum = re.sub(r"//[^\n]*", "", enum[enum.index("enum Slot"):enum.index("kNumSlots = ")])
    slots, nxt = {}, 0
    for item in enum.split("{", 1)[1].split(","):
        item = item.strip()
        if item:
            name, _, val = (t.strip() for t in item.partition("="))
            nxt = int(val) if val else nxt
            slots[name] = nxt
            nxt += 1
    assert (slots["kGapY"], slots["kGapX"], slots["kDXprev2"], slots["kCgQ2"], slots["kCgP2"], slots["kCgS2"]) == \
        (_lib.SLOT_GAP_Y, _lib.SLOT_GAP_X, _lib.SLOT_DXPREV2, _lib.SLOT_CG_Q2, _lib.SLOT_CG_P2, _lib.SLOT_CG_S2)
    assert "kNumSlots = %d" % _lib.NUM_SLOTS in open(os.path.join(ROOT, "pogs_amd", "csrc", "vec_kernels.h")).read()
    # the ctypes struct has the fields of the C struct, in its order, arrays with their lengths
    body = text[text.index("typedef struct PogsAmdVecArgs {"):text.index("} PogsAmdVecArgs;")].split("{", 1)[1]
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = decl.strip()
        if decl:
            fields += [t.strip().lstrip("*").split()[-1].lstrip("*") for t in decl.split(",")]
    mine = []
    for k, t in _lib.PogsAmdVecArgs._fields_:
        mine.append("%s[%d]" % (k, t._length_) if hasattr(t, "_length_") else k)
    assert fields == mine
    # ... and their kinds: int, size_t, double, pointer
    kinds = {}
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = decl.strip()
        if decl:
            base = decl.replace("const ", "").split()[0]
            for t in decl.split(","):
                nm = t.strip().split()[-1]
                kinds[nm.lstrip("*").split("[")[0]] = "ptr" if nm.startswith("*") else base
    want = {_lib.c_int: "int", _lib.c_size_t: "size_t", _lib.c_double: "double", _lib.c_void_p: "ptr"}
    for k, t in _lib.PogsAmdVecArgs._fields_:
        assert kinds[k] == want[getattr(t, "_type_", t) if hasattr(t, "_length_") else t], k


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib.lib, "PogsAmdVecCheck", boom)


def test_wrapper_checks_lengths_and_dtypes_before_the_library(no_library):
    P = _lib
    z = np.zeros
    with pytest.raises(ValueError, match="x-side arrays: one dtype"):
        P.vec_check(P.VEC_AXPBY, np.float64, n_x=4, x_in=[z(4, np.float32)], x_out=[z(4)])
    with pytest.raises(ValueError, match="x-side arrays: one length"):
        P.vec_check(P.VEC_AXPBY, np.float64, n_x=4, x_in=[z(4)], x_out=[z(5)])
    with pytest.raises(ValueError, match="y-side arrays: one length"):
        P.vec_check(P.VEC_UNSCALE, np.float64, n_x=4, n_y=4, x_in=[z(4)] * 4, x_out=[z(4)], y_in=[z(4)] * 4, y_out=[z(4), z(3)])
    with pytest.raises(ValueError, match="x-side arrays: one length"):
        P.vec_check(P.VEC_PROBE_UNIFORM, np.float64, n_x=4,
                    g=dict(h=z(4, np.int32), a=z(4), b=z(4), c=z(4), d=z(5), e=z(4)))
    with pytest.raises(ValueError, match="dtype"):
        P.vec_check(P.VEC_AXPBY, np.int32, n_x=4)
    with pytest.raises(ValueError, match="partials: float64"):
        P.vec_check(P.VEC_SUM_JOBS, np.float64, partials=z(4, np.float32), jobs=[[0, 4, 1, 0, 0, 0]])
    with pytest.raises(ValueError, match="scalars: float64, one dimension, 64 long"):
        P.vec_check(P.VEC_SUM_JOBS, np.float64, partials=z(4), jobs=[[0, 4, 1, 0, 0, 0]], scalars=z(52))
    with pytest.raises(ValueError, match="jobs: rows of 6 ints"):
        P.vec_check(P.VEC_SUM_JOBS, np.float64, partials=z(4), jobs=[[0, 4, 1, 0, 0]])
    with pytest.raises(ValueError, match="overlay"):
        P.vec_check(P.VEC_PUBLISH, np.float64, partials=z(4), overlay=(z(3), (0, 8), (2, 2)))


def _fn(dt, n, h=15):
    return dict(h=np.full(n, h, np.int32), a=np.ones(n, dt), b=np.zeros(n, dt), c=np.ones(n, dt), d=np.zeros(n, dt),
                e=np.zeros(n, dt))


def test_entry_refuses_before_any_device_work():
    P = _lib
    for dt in (np.float32, np.float64):
        z = lambda k=8: np.zeros(k, dt)
        g, f = _fn(dt, 8), _fn(dt, 8)
        pre = dict(n_x=8, n_y=8, x_in=[z(), z()], y_in=[z(), z()], x_out=[z(), z()], y_out=[z(), z()], g=g, f=f,
                   partials=np.zeros(6), scalars=np.zeros(64))
        job = [[0, 4, 1, 0, 0, 0]]
        bad = {
            "unknown op": lambda: P.vec_check(15, dt, n_x=8, x_out=[z()]),
            "n_x must be >= 1 and len_x >= n_x": lambda: P.vec_check(P.VEC_SCAL, dt, n_x=9, x_out=[z()]),
            "n_y must be >= 1 and len_y >= n_y": lambda: P.vec_check(P.VEC_ADMM_PRE, dt, **dict(pre, n_y=9)),
            r"null argument: x_in\[1\]": lambda: P.vec_check(P.VEC_SCALE_BY, dt, n_x=8, x_in=[z()], x_out=[z()]),
            r"null argument: x_out\[0\]": lambda: P.vec_check(P.VEC_FILL, dt, n_x=8, x_in=[z()]),
            r"null argument: x_out\[3\]": lambda: P.vec_check(P.VEC_SCALE_OBJECTIVE, dt, n_x=8, x_in=[z()], x_out=[z()] * 3, g=g),
            r"null argument: y_in\[3\]": lambda: P.vec_check(P.VEC_UNSCALE, dt, n_x=8, n_y=8, x_in=[z()] * 4, x_out=[z()],
                                                             y_in=[z()] * 3, y_out=[z()] * 2),
            r"null argument: y_out\[1\]": lambda: P.vec_check(P.VEC_UNSCALE, dt, n_x=8, n_y=8, x_in=[z()] * 4, x_out=[z()],
                                                              y_in=[z()] * 4, y_out=[z()]),
            "null argument: g_h": lambda: P.vec_check(P.VEC_PROBE_UNIFORM, dt, n_x=8, x_in=[z()]),
            "null argument: f_h": lambda: P.vec_check(P.VEC_ADMM_PRE, dt, **dict(pre, f=None)),
            r"mode must be 0 \(multiply\) or 1 \(divide\)": lambda: P.vec_check(P.VEC_SCALE_BY, dt, n_x=8, x_in=[z(), z()],
                                                                              x_out=[z()], mode=2),
            "cheap must be 0 or 1": lambda: P.vec_check(P.VEC_ADMM_PRE, dt, cheap=2, **pre),
            "probe must be 0 or 1": lambda: P.vec_check(P.VEC_ADMM_PRE, dt, probe=-1, **pre),
            "cheap = 1 with a function outside is_cheap_prox": lambda: P.vec_check(P.VEC_ADMM_PRE, dt, cheap=1,
                                                                                  **dict(pre, f=_fn(dt, 8, 8))),
            "u_mask must be in": lambda: P.vec_check(P.VEC_ADMM_PRE, dt, ug=(16, 0, 1, 0, 0), **pre),
            "null argument: partials, scalars": lambda: P.vec_check(P.VEC_ADMM_PRE, dt, **dict(pre, partials=None)),
            "partials_len must hold .blocks_x . blocks_y..3.": lambda: P.vec_check(P.VEC_ADMM_PRE, dt, **dict(pre, partials=np.zeros(5))),
            "partials_len must hold .blocks..2.": lambda: P.vec_check(P.VEC_ADMM_TAIL, dt, n_x=8, x_in=[z()] * 3, x_out=[z()],
                                                                     partials=np.zeros(1)),
            "null argument: partials, scalars, jobs": lambda: P.vec_check(P.VEC_SUM_JOBS, dt, partials=np.zeros(4)),
            "njobs must be in": lambda: P.vec_check(P.VEC_SUM_JOBS, dt, partials=np.zeros(4), jobs=job * 9),
            r"jobs\[0\]: nparts must be >= 1": lambda: P.vec_check(P.VEC_SUM_JOBS, dt, partials=np.zeros(4), jobs=[[0, 0, 1, 0, 0, 0]]),
            r"jobs\[1\]: ns must be in": lambda: P.vec_check(P.VEC_SUM_JOBS, dt, partials=np.zeros(4), jobs=job + [[0, 4, 0, 0, 0, 0]]),
            r"jobs\[0\]: first, stride and offset": lambda: P.vec_check(P.VEC_SUM_JOBS, dt, partials=np.zeros(4), jobs=[[0, 4, 1, -1, 0, 0]]),
            r"jobs\[0\]: the records reach beyond partials_len": lambda: P.vec_check(P.VEC_SUM_JOBS, dt, partials=np.zeros(4),
                                                                                    jobs=[[0, 4, 1, 0, 1, 0]]),
            r"jobs\[0\]: slot .. slot \+ ns leaves": lambda: P.vec_check(P.VEC_SUM_JOBS, dt, partials=np.zeros(8), jobs=[[0, 4, 2, 0, 0, 63]]),
            "partials_len must be in": lambda: P.vec_check(P.VEC_MAX_PARTIALS, dt, partials=np.zeros(0)),
            "null argument: partials, scalars, jobs, cg": lambda: P.vec_check(P.VEC_SUM_CG, dt, partials=np.zeros(4), jobs=job, mode=1),
            "mode must be 1, 2 or 3": lambda: P.vec_check(P.VEC_SUM_CG, dt, partials=np.zeros(4), jobs=job, cg=np.zeros(5), mode=0),
            r"jobs\[0\]: slot": lambda: P.vec_check(P.VEC_SUM_CG, dt, partials=np.zeros(4), jobs=[[0, 4, 1, 0, 0, 52]], cg=np.zeros(5), mode=1),
            "null argument: partials, scalars, pub": lambda: P.vec_check(P.VEC_PUBLISH, dt, jobs=job),
            r"mode must be 0 \(polling\) or 1 \(copying\)": lambda: P.vec_check(P.VEC_PUBLISH, dt, partials=np.zeros(4), jobs=job, mode=2),
            "njobs2 must differ from njobs": lambda: P.vec_check(P.VEC_PUBLISH, dt, partials=np.zeros(4), jobs=job, jobs2=job),
            r"jobs2\[0\]: the records reach": lambda: P.vec_check(P.VEC_PUBLISH, dt, partials=np.zeros(4), jobs2=[[1, 4, 1, 0, 0, 0]]),
            "ov_slot, ov_n: the range leaves": lambda: P.vec_check(P.VEC_PUBLISH, dt, partials=np.zeros(4), jobs=job,
                                                                  overlay=(np.zeros(3), (50, 0), (3, 0))),
        }
        for msg, call in bad.items():
            with pytest.raises(RuntimeError, match=msg):
                call()
        try:
            out = P.vec_check(P.VEC_FILL, dt, n_x=8, x_out=[z()], s0=2.0)
        except RuntimeError as e:        # no device here: the call got past every argument check
            assert "HIP error" in str(e) or "hip" in str(e).lower(), str(e)
        else:
            assert np.all(out["x_out"][0] == 2)
