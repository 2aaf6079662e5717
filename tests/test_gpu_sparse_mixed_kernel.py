"""The mixed-storage product of the solo sparse solver -- spmv_sell_kernel with float VALUES under fp64 arithmetic
(csrc/sell.h: S = float, T = double) -- through PogsAmdSpmvMixedCheck, against PogsAmdSpmvCheck(dtype F64) and numpy.

What the kernel promises: a float widens to double exactly and the order of every sum is fixed by the tile plan, not by
the value type, so the product over float values is BIT FOR BIT the fp64 kernel's product over the same (rounded)
values.  Every comparison here is therefore an equality of bytes; no tolerance appears.

fp64 geometry (sell.h: SellCfg<double>): column blocks 12288 wide; force_rr_rows = 512 rows per row range.  Shapes, the
smallest that reach each way the kernel can go wrong:

    a     40 x 30                       one tile
    b     1100 x 12300, ~8 per row      three row ranges x two column blocks; the last block is 12 columns wide --
                                        narrower than one batch of x vectors per thread, wider than a 16-byte vector
    b1    1100 x 12289                  the last block one column wide: narrower than a 16-byte vector (thread 0 owns it)
    c     b with force_ncg = 2          the column-group reduction (reduce_parts_kernel over fp64 partials); for
                                        trans = 't' the matrix is handed over transposed (12300 x 1100), so that the copy
                                        the product runs on is again the one with two column blocks
    d     600 x 500                     one row of 400 entries, 30 empty rows, the other rows of length 1 .. 33 in turn:
                                        streams end in every position of a batch

Each shape runs under formats 1 (a row tag per element), 2 (two id slots per batch) and 3 (the plain CSR kernel on the
rounded doubles), trans 'n' and 't', CSR and CSC input, (alpha, beta) in {(1, 0), (-2, 0.5)}, x_nrm2 in {0, 4}; every
run asserts from `info` that it reached the path it names.  Behind y three sentinels must come back untouched (x
carries NaN behind its length)."""
import numpy as np
import pytest
import scipy.sparse as sp

from helpers import ints, same_bytes
from pogs_amd import _lib

gpu = pytest.mark.gpu
SENTINEL = -7.375e-3
BW = 12288   # sell.h: SellCfg<double>::BW
CSR, CSC = _lib.ROW_MAJ, _lib.COL_MAJ
TAGS, TWO, PLAIN = _lib.SPMV_TAGS, _lib.SPMV_TWO, _lib.SPMV_PLAIN
WHY_PINNED = 6


def _random_pattern(m, n, per_row, rng):
    key = np.unique(rng.integers(0, m * n, m * per_row))
    return sp.csr_matrix((np.ones(key.size), (key // n, key % n)), shape=(m, n))


def _lengths_pattern(rng):
    """shape d: 600 x 500, row 7 holds 400 entries, 30 rows are empty, the others hold 1 .. 33 entries in turn"""
    m, n = 600, 500
    empty = set(rng.choice(np.setdiff1d(np.arange(m), [7]), 30, replace=False).tolist())
    rows, cols, turn = [], [], 0
    for r in range(m):
        if r in empty:
            continue
        L = 400 if r == 7 else 1 + turn % 33
        turn += r != 7
        c = np.sort(rng.choice(n, L, replace=False))
        rows.append(np.full(L, r))
        cols.append(c)
    P = sp.csr_matrix((np.ones(sum(c.size for c in cols)), (np.concatenate(rows), np.concatenate(cols))), shape=(m, n))
    lens = np.diff(P.indptr)
    assert lens.max() == 400 and np.sum(lens == 0) == 30 and set(range(1, 34)) <= set(lens.tolist())
    return P


# name -> (pattern builder, kwargs of the entry, what `info` of the product's copy must say for trans = 'n' on a tiled format)
SHAPES = {
    "a": (lambda rng: _random_pattern(40, 30, 6, rng), dict(force_rr_rows=512), dict(nrr=1, ncb=1, ncg=1)),
    "b": (lambda rng: _random_pattern(1100, 12300, 8, rng), dict(force_rr_rows=512), dict(rr_rows=512, nrr=3, ncb=2)),
    "b1": (lambda rng: _random_pattern(1100, 12289, 8, rng), dict(force_rr_rows=512), dict(rr_rows=512, nrr=3, ncb=2)),
    "c": (lambda rng: _random_pattern(1100, 12300, 8, rng), dict(force_rr_rows=512, force_ncg=2),
          dict(rr_rows=512, nrr=3, ncb=2, ncg=2)),
    "d": (_lengths_pattern, dict(force_rr_rows=512), dict(rr_rows=512, nrr=2, ncb=1, ncg=1)),
}
COMBOS = [(ord, trans, fmt, ab, xn) for ord in (CSR, CSC) for trans in "nt" for fmt in (TAGS, TWO, PLAIN)
          for ab in ((1.0, 0.0), (-2.0, 0.5)) for xn in (0.0, 4.0)]


class Case:
    """One shape: its pattern, and for trans = 't' of shape c the transposed pattern (module docstring)"""

    def __init__(self, name):
        build, self.kw, self.want = SHAPES[name]
        self.name = name
        self.rng = np.random.default_rng(sorted(SHAPES).index(name) + 20)
        self.P = build(self.rng).tocsr()
        self.P.sort_indices()
        assert 12300 % BW == 12 and 12289 % BW == 1

    def matrix(self, val, trans):
        """the matrix handed to the entry for a product with `trans`; val: one value per entry of the pattern, CSR order"""
        A = sp.csr_matrix((val, self.P.indices, self.P.indptr), shape=self.P.shape)
        return A.T.tocsr() if (self.name == "c" and trans == "t") else A

    def arrays(self, A, ord):
        B = A if ord == CSR else A.tocsc()
        return B.indptr.astype(np.int32), B.indices.astype(np.int32), np.ascontiguousarray(B.data, np.float64)

    def check_info(self, info, trans, fmt, where):
        if fmt == PLAIN:
            assert (info["tiled"], info["why"]) == (0, WHY_PINNED), (where, info)
            return
        assert info["tiled"] == 1 and info["two"] == (fmt == TWO), (where, info)
        if trans == "n" or self.name == "c":
            for k, v in self.want.items():
                assert info[k] == v, (where, k, info)


def _padded(x, y0):
    return np.concatenate([x, np.full(2, np.nan)]), np.concatenate([y0, np.full(3, SENTINEL)])


def _call(entry, case, A, ord, trans, fmt, ab, xn, x, y0, scale, **extra):
    m, n = A.shape
    nout = m if trans == "n" else n
    ptr, ind, v = case.arrays(A, ord)
    xp, yp = _padded(x, y0)
    y, sumsq, infos = entry(ptr, ind, v, (m, n), xp, yp, trans=trans, ord=ord, num_cu=256, format=fmt, scale=scale,
                            x_nrm2=xn, alpha=ab[0], beta=ab[1], **case.kw, **extra)[:3]
    assert same_bytes(y[nout:], np.full(3, SENTINEL)), (case.name, "wrote behind y")
    return y[:nout], sumsq, infos


@gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_small_integers_give_numpys_product_exactly(name):
    """values and x in -4 .. 4 (exact in float, every partial sum an integer or a half): y and sumsq equal numpy's"""
    case = Case(name)
    val = ints(case.rng, case.P.nnz, np.float64)
    val[val == 0] = 3.0
    for ord, trans, fmt, ab, xn in COMBOS:
        A = case.matrix(val, trans)
        m, n = A.shape
        nin, nout = (n, m) if trans == "n" else (m, n)
        x, y0 = ints(case.rng, nin, np.float64), ints(case.rng, nout, np.float64)
        where = (name, "csr" if ord == CSR else "csc", trans, fmt, ab, xn)
        y, sumsq, infos = _call(_lib.spmv_mixed_check, case, A, ord, trans, fmt, ab, xn, x, y0, 1.0)
        case.check_info(infos[0 if trans == "n" else 1], trans, fmt, where)
        op = A if trans == "n" else A.T
        ref = ab[0] * (op @ (x * (0.5 if xn else 1.0))) + ab[1] * y0
        assert np.array_equal(y, ref), where + (int(np.argmax(y != ref)),)
        assert sumsq == float(np.sum(ref * ref)), where + (sumsq,)


@gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_real_values_give_the_bytes_of_the_fp64_kernel_on_the_rounded_values(name):
    """MixedCheck(v, scale) == SpmvCheck(F64, float32(v scale) as double, scale = 1): y, sumsq and all 16 info words, under
    the same format and forced geometry; MixedCheck(v) == MixedCheck(float32(v) as double) at scale 1; a second call
    returns the same bytes"""
    case = Case(name)
    rng = case.rng
    v = rng.standard_normal(case.P.nnz) * 10.0 ** rng.uniform(-3, 3, case.P.nnz)
    assert np.all(v != v.astype(np.float32)) and np.all((v * 0.37) != (v * 0.37).astype(np.float32))
    for scale in (1.0, 0.37):
        for ord, trans, fmt, ab, xn in COMBOS:
            A = case.matrix(v, trans)
            m, n = A.shape
            nin, nout = (n, m) if trans == "n" else (m, n)
            x, y0 = rng.standard_normal(nin), rng.standard_normal(nout)
            where = (name, scale, "csr" if ord == CSR else "csc", trans, fmt, ab, xn)
            got = _call(_lib.spmv_mixed_check, case, A, ord, trans, fmt, ab, xn, x, y0, scale)
            case.check_info(got[2][0 if trans == "n" else 1], trans, fmt, where)
            rounded = case.matrix((v * scale).astype(np.float32).astype(np.float64), trans)
            want = _call(_lib.spmv_check, case, rounded, ord, trans, fmt, ab, xn, x, y0, 1.0, sq=False)
            assert same_bytes(got[0], want[0]), where + (int(np.argmax(got[0] != want[0])),)
            assert got[1] == want[1], where + (got[1], want[1])
            assert got[2] == want[2], where + (got[2], want[2])
            assert np.all(np.isfinite(got[0])) and np.any(got[0] != 0)
            if scale == 1.0:
                again = _call(_lib.spmv_mixed_check, case, rounded, ord, trans, fmt, ab, xn, x, y0, 1.0)
            else:
                again = _call(_lib.spmv_mixed_check, case, A, ord, trans, fmt, ab, xn, x, y0, scale)
            assert same_bytes(got[0], again[0]) and got[1] == again[1] and got[2] == again[2], where


def test_the_entry_refuses_as_the_fp64_one_does():
    """the shared argument checks (they come before any device work: no GPU is needed), and the float32 arrays the
    wrapper refuses"""
    case = Case("a")
    A = case.matrix(np.ones(case.P.nnz), "n")
    ptr, ind, v = case.arrays(A, CSR)
    x, y = np.ones(30), np.zeros(40)
    for kw, msg in ((dict(trans="x"), "trans must be"), (dict(format=4), "unknown format"),
                    (dict(force_rr_rows=100), "force_rr_rows must be"), (dict(force_ncg=2), "force_ncg must be")):
        with pytest.raises(RuntimeError, match=msg):
            _lib.spmv_mixed_check(ptr, ind, v, A.shape, x, y, **kw)
    with pytest.raises(ValueError, match="float64"):
        _lib.spmv_mixed_check(ptr, ind, v.astype(np.float32), A.shape, x.astype(np.float32), y.astype(np.float32))
