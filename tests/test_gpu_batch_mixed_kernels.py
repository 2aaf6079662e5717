"""GPU tests of the batched solve's two passes over A for a matrix stored as float32 -- the float copy of a
mixed-storage handle -- on their own (include/pogs_amd.h, Part 3: PogsAmdBatchRowsMixedCheck,
PogsAmdBatchColsMixedCheck): vectors, partial sums and arithmetic are float64.

What is held to what:
  * same bytes: on badly scaled real data the mixed entry returns, bit for bit, what the fp64 entry
    (PogsAmdBatchRowsCheck / PogsAmdBatchColsCheck) returns for the matrix widened to float64, and reports the same
    row-block partition -- every output element is added up in the fp64 kernel's order;
  * exact integers: entries in [-4, 4], every order of summation gives the exact answer: equal to numpy bit for bit;
  * isolation and padding: a problem's bytes are the same alone, in slot 15 of 16 and next to members poisoned with
    Inf / NaN / 1e30; inactive members and output padding keep the sentinel; the float row is NaN from `cols` to `ldm`
    (ldm > round_up(cols, 4)) and no NaN reaches a result;
  * refusals: POGS_ERROR with a message, before any device work.

Shapes: rows cross the 16-row group and the 64-row workgroup; cols cross VEC = 2, the wave step 8, the four waves' 32,
the 32- and 64-column slabs and include round_up(cols, 2) % 4 == 2 (5, 6, 61, 62), where the last float vector of a
row covers two columns no fp64 vector has."""
import ctypes

import numpy as np
import pytest

from helpers import ints, same_bytes, scaled_normal
from pogs_amd import _lib
from test_gpu_batch_kernels import FULL, K, SENTINEL, _check_cols_out, _check_untouched, poison, rup, slot_lists

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 63, 64, 65, 1037)
COLS = (1, 2, 3, 5, 6, 7, 9, 31, 33, 61, 62, 1000)
F64 = np.float64
POGS_ERROR = 6          # include/pogs_amd.h: PogsStatus


def _matrix(rng, rows, cols, data):
    """(M32, Mv): rows x ldm float32 with ldm = round_up(cols, 4) + 4, NaN from `cols` on; Mv its rows x cols values"""
    ldm = rup(cols, 4) + 4
    Mv = (ints(rng, (rows, cols), F64) if data == "int" else scaled_normal(rng, (rows, cols))).astype(np.float32)
    M = np.full((rows, ldm), np.nan, np.float32)
    M[:, :cols] = Mv
    return M, Mv


def _rows_case(rng, rows, cols, data="real"):
    cp = rup(cols, 2)
    M, Mv = _matrix(rng, rows, cols, data)
    X = np.zeros((K, cp + 4), F64)
    Xv = ints(rng, (K, cols), F64) if data == "int" else rng.standard_normal((K, cols))
    X[:, :cols] = Xv                            # X[:, cols:cp] = 0: the contract; beyond: unused
    X[:, cp:] = np.nan
    return M, X, np.full((K, rows + 3), SENTINEL, F64), Mv, Xv


def _cols_case(rng, rows, cols, data="real", add=False):
    cp = rup(cols, 2)
    M, Mv = _matrix(rng, rows, cols, data)
    U = np.full((K, rows + 5), np.nan, F64)
    Uv = ints(rng, (K, rows), F64) if data == "int" else rng.standard_normal((K, rows))
    U[:, :rows] = Uv
    A = None
    if add:
        A = np.full((K, cp + 4), np.nan, F64)
        A[:, :cp] = ints(rng, (K, cp), F64) if data == "int" else rng.standard_normal((K, cp))
    return M, U, np.full((K, cp + 4), SENTINEL, F64), A, Mv, Uv


# ---- same bytes as the fp64 entry on the widened matrix ------------------------------------------------------------

@pytest.mark.parametrize("rows", ROWS)
def test_rows_same_bytes_as_the_fp64_entry(rows):
    rng = np.random.default_rng(100 + rows)
    for cols in COLS:
        M, X, Y0, _, _ = _rows_case(rng, rows, cols)
        act = list(rng.permutation(K)[:11])
        got = _lib.batch_rows_mixed_check(M, cols, X, Y0, act)
        # (the fp64 entry never uses M's columns >= cols either, so the NaN padding is widened along)
        want = _lib.batch_rows_check(FULL, M.astype(F64), cols, X, Y0, act)
        assert np.all(np.isfinite(got[act, :rows])), (rows, cols)
        assert same_bytes(got, want), (rows, cols)
        _check_untouched(got, act, rows)


@pytest.mark.parametrize("rows", ROWS + (4099,))
def test_cols_same_bytes_as_the_fp64_entry(rows):
    rng = np.random.default_rng(200 + rows)
    for cols in ((70,) if rows == 4099 else COLS):
        for add in (False, True):
            M, U, Z0, A, _, _ = _cols_case(rng, rows, cols, add=add)
            act = list(rng.permutation(K)[:13])
            got, nrb, rpb = _lib.batch_cols_mixed_check(M, cols, U, Z0, act, add=A)
            want, nrb64, rpb64 = _lib.batch_cols_check(M.astype(F64), cols, U, Z0, act, add=A)
            assert (nrb, rpb) == (nrb64, rpb64), (rows, cols)
            assert np.all(np.isfinite(got[act, :cols])), (rows, cols, add)
            assert same_bytes(got, want), (rows, cols, add)
            _check_cols_out(got, act, cols, rup(cols, 2))
            if rows == 4099:
                assert nrb > 1 and rows % rpb != 0          # several row blocks, a ragged last one


# ---- exact integers ------------------------------------------------------------------------------------------------

def test_rows_exact_integer_parity():
    rng = np.random.default_rng(3)
    for rows in ROWS:
        for cols in COLS:
            M, X, Y0, Mv, Xv = _rows_case(rng, rows, cols, data="int")
            act = list(rng.permutation(K)[:11])
            Y = _lib.batch_rows_mixed_check(M, cols, X, Y0, act)
            ref = Mv.astype(F64) @ Xv.T
            assert np.array_equal(Y[act, :rows], ref.T[act]), (rows, cols)
            _check_untouched(Y, act, rows)


def test_cols_exact_integer_parity():
    rng = np.random.default_rng(5)
    for rows, cols in [(r, c) for r in ROWS for c in COLS] + [(4099, 70)]:
        add = bool((rows + cols) & 1)
        M, U, Z0, A, Mv, Uv = _cols_case(rng, rows, cols, data="int", add=add)
        act = list(rng.permutation(K)[:13])
        Z, _, _ = _lib.batch_cols_mixed_check(M, cols, U, Z0, act, add=A)
        ref = Uv @ Mv.astype(F64)
        if add:
            ref = ref + A[:, :cols]
        assert np.array_equal(Z[act, :cols], ref[act]), (rows, cols, add)
        _check_cols_out(Z, act, cols, rup(cols, 2))


# ---- isolation and padding -----------------------------------------------------------------------------------------

def test_rows_isolation():
    rng = np.random.default_rng(11)
    rows = cols = 129
    M, X, Y0, Mv, Xv = _rows_case(rng, rows, cols)
    p = 6
    first = None
    for act in slot_lists(rng, p):
        Y = _lib.batch_rows_mixed_check(M, cols, poison(rng, X, act, p, cols), Y0, act)
        _check_untouched(Y, act, rows)
        if first is None:
            first = Y[p].copy()
            assert np.all(np.isfinite(first[:rows]))
            assert same_bytes(first, _lib.batch_rows_check(FULL, M.astype(F64), cols, X, Y0, act)[p])
        assert same_bytes(Y[p], first), act


def test_cols_isolation():
    rng = np.random.default_rng(13)
    rows, cols = 1037, 77
    M, U, Z0, A, Mv, Uv = _cols_case(rng, rows, cols, add=True)
    p = 9
    first = None
    for act in slot_lists(rng, p):
        Ap = poison(rng, A, act, p, rup(cols, 2))
        Z, _, _ = _lib.batch_cols_mixed_check(M, cols, poison(rng, U, act, p, rows), Z0, act, add=Ap)
        _check_cols_out(Z, act, cols, rup(cols, 2))
        if first is None:
            first = Z[p].copy()
            assert np.all(np.isfinite(first[:cols]))
        assert same_bytes(Z[p], first), act


# ---- refusals, then a valid call -----------------------------------------------------------------------------------

def _raw_rows(M, cols, X, Y, act, ldm=None, k=None, nact=None, null=None):
    a = np.ascontiguousarray(act, np.int32)
    ptr = dict(M=M.ctypes.data, act=a.ctypes.data, X=X.ctypes.data, Y=Y.ctypes.data)
    if null:
        ptr[null] = None
    return _lib.lib.PogsAmdBatchRowsMixedCheck(M.shape[0], cols, ptr["M"], M.shape[1] if ldm is None else ldm,
                                               X.shape[0] if k is None else k, ptr["act"], a.size if nact is None else nact,
                                               ptr["X"], X.shape[1], ptr["Y"], Y.shape[1])


def _raw_cols(M, cols, U, Z, act, ldm=None, k=None, nact=None, null=None):
    a = np.ascontiguousarray(act, np.int32)
    nrb, rpb = ctypes.c_int(0), ctypes.c_int(0)
    ptr = dict(M=M.ctypes.data, act=a.ctypes.data, U=U.ctypes.data, Z=Z.ctypes.data, nrb=ctypes.byref(nrb),
               rpb=ctypes.byref(rpb))
    if null:
        ptr[null] = None
    return _lib.lib.PogsAmdBatchColsMixedCheck(M.shape[0], cols, ptr["M"], M.shape[1] if ldm is None else ldm,
                                               U.shape[0] if k is None else k, ptr["act"], a.size if nact is None else nact,
                                               ptr["U"], U.shape[1], None, ptr["Z"], Z.shape[1], ptr["nrb"], ptr["rpb"])


def test_refusals_leave_the_entries_working():
    rng = np.random.default_rng(17)
    rows, cols = 33, 30
    M, X, Y0, Mv, Xv = _rows_case(rng, rows, cols, data="int")
    Mc, U, Z0, _, Mvc, Uv = _cols_case(rng, rows, cols, data="int")
    bad = [dict(ldm=M.shape[1] - 2), dict(ldm=rup(cols, 4) - 4), dict(k=0), dict(k=K + 1), dict(nact=0),
           dict(nact=K + 1), dict(act=[K]), dict(act=[-1]), dict(act=[2, 2])]
    for raw, args, names in ((_raw_rows, (M, cols, X, Y0.copy()), ("M", "act", "X", "Y")),
                             (_raw_cols, (Mc, cols, U, Z0.copy()), ("M", "act", "U", "Z", "nrb", "rpb"))):
        out = args[3]
        for kw in bad + [dict(null=nm) for nm in names]:
            kw = dict(kw)
            act = kw.pop("act", [3, 1])
            assert raw(*args, act, **kw) == POGS_ERROR, kw
            assert _lib.last_error(), kw
            assert np.all(out == SENTINEL), kw                 # nothing was written
        assert raw(*args, [3, 1]) == 0
    Y = _lib.batch_rows_mixed_check(M, cols, X, Y0, [3])
    assert np.array_equal(Y[3, :rows], Mv.astype(F64) @ Xv[3])
    Z, _, _ = _lib.batch_cols_mixed_check(Mc, cols, U, Z0, [3])
    assert np.array_equal(Z[3, :cols], Uv[3] @ Mvc.astype(F64))
    with pytest.raises(ValueError, match="float32"):
        _lib.batch_rows_mixed_check(M.astype(F64), cols, X, Y0, [3])
