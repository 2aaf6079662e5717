"""The kernels of the dense factorisation (DenseSolver::factor: Gram product, Cholesky, L^-1, transpose) on their own,
through PogsAmdGramCheck, PogsAmdCholCheck and PogsAmdGetFactor (include/pogs_amd.h, Part 3), against references
formed in fp64 (fp32 data) or beyond it (fp64 data: long double sums, helpers.xmatmul).

Gram product.  PogsAmdGramCheck runs the function factor() calls and reports what it chose (`info`); every case below
names the path it must reach and asserts it, so a case that stops reaching its path fails.  num_cu = 256 in every case.

    kdim x k            type   force   path the case must reach
    77 x {1, 3, 127, 128, 129, 255, 257}   both   -    native, one launch (ksplit 1), natural tile order
    1000 x 2048         both   -       native, ksplit 1, natural order (k = 16 tiles)
    100 x 2049          both   -       native, ksplit 1, tile_map (k > 16 tiles)
    4095 x 129          both   -       native, ksplit 1 (one row short of two K ranges)
    4096 x 128          both   -       native, ksplit 2, kchunk 2048
    4097 x 127          both   -       native, ksplit 2, kchunk 2080: the second range is 2017 rows, ends inside a step
    20000 x 65, x 255   both   -       native, ksplit 8, kchunk 2528: rounds of 4, 3 and 1 slabs
    40001 x 3           both   -       native, ksplit 16: rounds of 4, 3, 3, 3, 3
    205000 x 3 (all +4) both   -       native, ksplit 32, kchunk 6432; fp32: kacc 3232 (two-level accumulation)
    8321 x 300          fp32   native  native, ksplit 4 where the fp16 split is the default
    8320 x 300          fp32   -       fp16 split, 128 tile, 4 units of 2080 rows, all full
    8319 x 257          fp32   -       fp16 split, 128 tile, 4 units of 2080, the last one row short
    8321 x 256          fp32   -       fp16 split, 128 tile, 4 units of 2112, the last 1985 rows
    51201 x 257         fp32   -       fp16 split, 128 tile, 8 units of 6432: a second, accumulating launch
    8200 x 2049         fp32   -       fp16 split, 128 tile with its tile_map
    8192 x 4095         fp32   -       fp16 split, 128 tile with its tile_map, the last k below the 256 tile
    8320 x 300, 9001 x 513  fp32  256  fp16 split, 256 tile forced, natural order
    8222 x 4096         fp32   -       fp16 split, 256 tile, natural order (k = 16 tiles)
    20000 x 4097        fp32   -       fp16 split, 256 tile with its tile_map

Not reachable, so not in the list: the fp16 split with ONE unit (it needs kdim >= 8192, and the rows are cut into
4 x launches units of at most 12800: 4 units up to 51200 rows, 8 from there); a leading dimension of the factor that is
not a multiple of the 16-byte vector (factor() rounds it up), i.e. the unpacked branch of the row-sharded all-reduce;
the row-major operand form of the native product (the direct projector stores the K index first in both shapes).

Cholesky and L^-1.  PogsAmdCholCheck runs cholesky_lower, trtri_lower and launch_transpose on four zeroed slabs as
factor() does.  What the solves rely on (stream.h, launch_stream<.., kLower / kUpper>): a pass over W reads the 16-byte
vectors that start at or before the diagonal, one over U those that end at or after it, both up to the padded row
length -- so W must be zero from the diagonal to the end of its vector and in the columns n .. ld, U from the start of
the diagonal's vector to the diagonal.  The tests assert more, which also holds: all of W above and all of U below the
diagonal and every padding column are zero.  L is not read after the inverse; its strict upper triangle keeps what H
held there.  A matrix that is not positive definite is no error here: the one-workgroup diagonal-block kernel takes the
square root of the pivot whatever its sign and no loop bound depends on data, so the column of the first bad pivot and
everything to its right and below comes back NaN (as do the few columns before it that share its 16-row register group,
in the rows below the diagonal block), the columns before those as for a good matrix; the reference's
linalg_cholesky_decomp, gsl_linalg.h:36-55, reports an error at that pivot instead.

Measured error / bar ratios: profiles/factor_accuracy.txt (the tests print them: pytest -s)."""
import os
import threading

import numpy as np
import pytest
import scipy.linalg as sla

from helpers import _w_bars, gamma, hi, ints, same_bytes, scaled_normal, xmatmul
from pogs_amd import _lib

gpu = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
SENTINEL = -7.375e-3
NB = {np.float32: 128, np.float64: 64}       # gemm.h: CholBlock<T>::NB
GROUP = {np.float32: 2, np.float64: 4}       # gemm.hip: kCholGroup


def vec(dt):
    return 16 // np.dtype(dt).itemsize


def rup(v, a):
    return (v + a - 1) // a * a


def tname(dt):
    return "fp32" if dt == np.float32 else "fp64"


def report(line):
    print("factor_accuracy: " + line)


# ---- Gram product ---------------------------------------------------------------------------------------------------

BOTH = (np.float32, np.float64)
F32 = (np.float32,)
NATIVE, T256 = _lib.GRAM_NATIVE, _lib.GRAM_TILE_256
# (kdim, k, dtypes, force, expected info fields)
GRAM_CASES = [(77, k, BOTH, 0, dict(path=0, ksplit=1, tile_map=0)) for k in (1, 3, 127, 128, 129, 255, 257)] + [
    (1000, 2048, BOTH, 0, dict(path=0, ksplit=1, tile_map=0)),
    (100, 2049, BOTH, 0, dict(path=0, ksplit=1, tile_map=1)),
    (4095, 129, BOTH, 0, dict(path=0, ksplit=1)),
    (4096, 128, BOTH, 0, dict(path=0, ksplit=2, kchunk=2048)),
    (4097, 127, BOTH, 0, dict(path=0, ksplit=2, kchunk=2080)),
    (20000, 65, BOTH, 0, dict(path=0, ksplit=8, kchunk=2528)),
    (20000, 255, BOTH, 0, dict(path=0, ksplit=8, kchunk=2528)),
    (40001, 3, BOTH, 0, dict(path=0, ksplit=16)),
    (8321, 300, F32, NATIVE, dict(path=0, ksplit=4)),
    (8320, 300, F32, 0, dict(path=1, tile=128, units=4, unit_rows=2080, tile_map=0)),
    (8319, 257, F32, 0, dict(path=1, tile=128, units=4, unit_rows=2080)),
    (8321, 256, F32, 0, dict(path=1, tile=128, units=4, unit_rows=2112)),
    (51201, 257, F32, 0, dict(path=1, tile=128, units=8, unit_rows=6432)),
    (8200, 2049, F32, 0, dict(path=1, tile=128, units=4, tile_map=1)),
    (8192, 4095, F32, 0, dict(path=1, tile=128, units=4, tile_map=1)),
    (8320, 300, F32, T256, dict(path=1, tile=256, units=4, tile_map=0)),
    (9001, 513, F32, T256, dict(path=1, tile=256, units=4, tile_map=0)),
    (8222, 4096, F32, 0, dict(path=1, tile=256, units=4, tile_map=0)),
    (20000, 4097, F32, 0, dict(path=1, tile=256, units=4, tile_map=1)),
]
ALL_FOUR = (205000, 3)     # the largest kdim, every entry +4: a row counted twice shows as well as one dropped


def _gram_operand(dt, kdim, k, values):
    """P (kdim x lda, lda > k, NaN in the columns >= k, which are never read) and a sentinel-filled G (k x ldg)"""
    lda = rup(k, vec(dt)) + vec(dt)
    P = np.full((kdim, lda), np.nan, dt)
    P[:, :k] = values
    return P, np.full((k, k + 3), SENTINEL, dt)


def _tile_mask(k, tile=128):
    """the lower tiles of a k x k matrix (128: what the Gram phase returns)"""
    t = np.arange(k) // tile
    return t[:, None] >= t[None, :]


def _check_info(info, want, case):
    for key, v in want.items():
        assert info[key] == v, (case, key, info)
    if info["path"] == 1:
        assert info["ksplit"] == 0 and info["kacc"] == 0, (case, info)


def _exact_gram(dt, kdim, k, force, want, values):
    P, G0 = _gram_operand(dt, kdim, k, values)
    G, info = _lib.gram_check(P, k, G0, force=force, num_cu=256)
    _check_info(info, want, (kdim, k, tname(dt), force))
    v = P[:, :k]
    # integer sums below 2^24: the fp32 BLAS product is exact too, and much faster than fp64 at k > 2049
    ref = (v.T @ v) if k > 2049 else (v.astype(np.float64).T @ v.astype(np.float64)).astype(dt)
    mask = _tile_mask(k)
    assert np.array_equal(G[:, :k][mask], ref[mask]), (kdim, k, tname(dt), force, info)
    # untouched: what lies above the diagonal tiles of the launch (the 256 tile writes its diagonal tiles whole, so the
    # 128-tiles above the diagonal inside them hold the first slab's share: as left by the launches, not asserted)
    wrote = _tile_mask(k, info["tile"])
    assert np.all(G[:, :k][~wrote] == np.asarray(SENTINEL, dt)) and np.all(G[:, k:] == np.asarray(SENTINEL, dt))
    return info


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gram_exact_integers_every_path(dtype, monkeypatch):
    """Entries in {-4 .. 4}: every partial sum is an integer below 2^24 and the fp16 split of an entry is (itself, 0), so
    every path returns the lower tiles of P^T P bit for bit; what lies above them comes back untouched.  (force = 0 is
    "as a solve would choose, the environment included": the two variables are cleared so that the table holds under the
    suite's POGS_AMD_GRAM / POGS_AMD_GRAM_TILE sweeps too.)"""
    monkeypatch.delenv("POGS_AMD_GRAM", raising=False)
    monkeypatch.delenv("POGS_AMD_GRAM_TILE", raising=False)
    rng = np.random.default_rng(101)
    seen = []
    for kdim, k, dts, force, want in GRAM_CASES:
        if dtype in dts:
            seen.append(_exact_gram(dtype, kdim, k, force, want, ints(rng, (kdim, k), dtype)))
    kdim, k = ALL_FOUR
    info = _exact_gram(dtype, kdim, k, 0, dict(path=0, ksplit=32, kchunk=6432, kacc=3232 if dtype == np.float32 else 0),
                       np.full((kdim, k), 4, dtype))
    seen.append(info)
    seen.append(_exact_gram(dtype, kdim, k, 0, dict(path=0, ksplit=32), ints(rng, (kdim, k), dtype)))
    # the list as a whole (the table of the module docstring)
    nat = [i for i in seen if i["path"] == 0]
    assert {1, 2} <= {i["ksplit"] for i in nat} and any(i["ksplit"] >= 8 for i in nat)
    assert any(i["tile_map"] for i in nat) and any(not i["tile_map"] for i in nat)
    if dtype == np.float32:
        assert any(i["kacc"] > 0 for i in nat)
        sp = [i for i in seen if i["path"] == 1]
        for tile in (128, 256):
            assert {0, 1} == {i["tile_map"] for i in sp if i["tile"] == tile}, tile
        assert {4, 8} <= {i["units"] for i in sp if i["tile"] == 128}
    else:
        assert all(i["path"] == 0 and i["kacc"] == 0 for i in seen)


def test_refusals_come_before_any_device_work():
    """n = 0, NULL arrays, a bad dtype, bad leading dimensions: POGS_ERROR with the reason, and no GPU is needed to say so."""
    P = np.ones((8, 4), np.float32)
    G = np.zeros((3, 3), np.float32)
    with pytest.raises(RuntimeError, match="kdim and k"):
        _lib.gram_check(P, 0, np.zeros((0, 3), np.float32))
    with pytest.raises(RuntimeError, match="unknown force"):
        _lib.gram_check(P, 3, G, force=7)
    with pytest.raises(RuntimeError, match="num_cu"):
        _lib.gram_check(P, 3, G, num_cu=-1)
    with pytest.raises(RuntimeError, match="lda must be"):
        _lib.gram_check(np.ones((8, 5), np.float32), 3, G)            # lda not a multiple of VEC
    with pytest.raises(RuntimeError, match="ldg must be"):
        _lib.gram_check(P, 4, np.zeros((4, 3), np.float32))
    info = np.zeros(8, np.int32)
    lib = _lib.lib
    assert lib.PogsAmdGramCheck(0, 8, 3, None, 4, 0, 0, G.ctypes.data, 3, info.ctypes.data) != 0
    assert "null argument" in _lib.last_error()
    assert lib.PogsAmdGramCheck(5, 8, 3, P.ctypes.data, 4, 0, 0, G.ctypes.data, 3, info.ctypes.data) != 0
    assert "unknown dtype" in _lib.last_error()
    H = np.eye(3, dtype=np.float32)
    out = np.zeros((3, 3), np.float32)
    p = out.ctypes.data
    assert lib.PogsAmdCholCheck(0, 0, H.ctypes.data, 3, p, p, p, 3) != 0 and "n must be >= 1" in _lib.last_error()
    assert lib.PogsAmdCholCheck(0, 3, None, 3, p, p, p, 3) != 0 and "null argument" in _lib.last_error()
    assert lib.PogsAmdCholCheck(0, 3, H.ctypes.data, 3, p, None, p, 3) != 0 and "null argument" in _lib.last_error()
    assert lib.PogsAmdCholCheck(2, 3, H.ctypes.data, 3, p, p, p, 3) != 0 and "unknown dtype" in _lib.last_error()
    assert lib.PogsAmdCholCheck(0, 3, H.ctypes.data, 2, p, p, p, 3) != 0 and "ldh and ldo" in _lib.last_error()
    assert lib.PogsAmdGetFactor(None, p, p) != 0 and "null solver" in _lib.last_error()


# The bar of the real-data Gram tests, entry (i, j):  beta |P|^T |P|  (+ the fp16 split's small-entry term).
#   native product: a kdim-term dot product in the working type, any order: gamma_kdim, with u = eps and not eps / 2 because
#     the MFMA accumulate truncates (gemm.hip); the slab sums are among the kdim - 1 additions.
#   fp16 split: a scaled entry a s (s = 2^(14 - ex), amax = f 2^ex, f in [0.5, 1)) is stored as h + l, h = fp16(a s),
#     l = fp16(a s - h), and a s = h + l + r.  fp16 has an 11-bit significand, normal numbers down to 2^-14, spacing 2^-24
#     below:  |a s - h| <= 2^-11 |a s|  (a s - h is exact in fp32),  |r| <= 2^-11 |a s - h| <= 2^-22 |a s|  where l is
#     normal, |r| <= 2^-25 where it is not, so |r| <= 2^-22 |a s| + 2^-25.  The kernel forms hh + hl + lh; left out of
#     (h + l + r)(h' + l' + r') are  l l' (<= 2^-22 |a s||b s|),  r (b s) and (a s) r' (<= 2^-22 |a s||b s| + 2^-25 |b s|
#     and likewise), r r' (second order).  Per product, unscaled by s^2 and with 1 / s = 2^(ex - 14) <= 2^-13 amax:
#         3 2^-22 |a||b| + 2^-38 amax (|a| + |b|)   <=   2^-20 |a||b| + 2^-38 amax (|a| + |b|).
#     (One case escapes this by a hair: a s below the normal range whose remainder is exactly half the subnormal spacing
#     has l = +-2^-24 AND |r| = 2^-25, so l l' adds 2^-35 |b s| to the 2^-25 |b s| of r: the small term carries a factor
#     1 + 2^-10 for it.)  The three piece products are exact in fp32 (11 x 11 bits) and are summed there, 3 kdim terms
#     plus one addition per 1024-row chain and per slab, with |h h'| + |h l'| + |l h'| <= (1 + 2^-9) |a s||b s|:
#         beta = (1 + 2^-9) gamma_(3 kdim + kdim / 1024 + 8) (u = eps) + 2^-20.
def _gram_bar(P64abs, kdim, dt, split, amax):
    eps = np.finfo(dt).eps
    absprod = P64abs.T @ P64abs
    if not split:
        return gamma(kdim, dt, u=eps) * absprod
    beta = (1 + 2.0 ** -9) * gamma(3 * kdim + kdim // 1024 + 8, dt, u=eps) + 2.0 ** -20
    colsum = P64abs.sum(axis=0)
    return beta * absprod + _split_small_term(amax, colsum)


def _split_small_term(amax, colsum):
    return 2.0 ** -38 * (1 + 2.0 ** -10) * amax * (colsum[:, None] + colsum[None, :])


def _split_emulated(v):
    """The fp16 split's product in exact arithmetic but for the split itself: float16 casts, piece products summed in fp64
    (gemm.hip: split8_f16, and gram_phase.h for the scale)."""
    amax = float(np.max(np.abs(v)))
    ex = int(np.frexp(amax)[1])
    s = np.float32(2.0 ** (14 - ex))
    a = (v * s).astype(np.float32)
    h = a.astype(np.float16)
    lo = (a - h.astype(np.float32)).astype(np.float16)
    h64, l64 = h.astype(np.float64), lo.astype(np.float64)
    return (h64.T @ h64 + h64.T @ l64 + l64.T @ h64) / float(s) ** 2, amax


# (kdim, k, dtypes, force, path): every path of the table once more on real-valued data
GRAM_REAL = [(1000, 129, BOTH, 0, 0), (4097, 127, BOTH, 0, 0), (20000, 65, BOTH, 0, 0), (205000, 3, BOTH, 0, 0),
             (8321, 300, F32, NATIVE, 0), (8319, 300, F32, 0, 1), (51201, 257, F32, 0, 1), (9001, 300, F32, T256, 1)]


def _gram_real_values(kdim, k, dt, family):
    rng = np.random.default_rng(kdim * 7 + k + (0 if family == "normal" else 1))
    v = rng.standard_normal((kdim, k)) if family == "normal" else scaled_normal(rng, (kdim, k))
    return v.astype(dt)


def _hi_gram(v):
    """P^T P in fp64 for fp32 data (every product exact, a kdim-term sum in fp64), beyond fp64 for fp64 data"""
    return v.astype(np.float64).T @ v.astype(np.float64) if v.dtype == np.float32 else xmatmul(v.T, v)


def test_fp16_split_term_of_the_gram_bar_holds_for_the_emulated_split():
    """The split term of the bar on the test's own inputs, without a GPU: the split emulated in numpy, its three products
    summed in fp64, must sit inside 2^-20 |P|^T |P| + the small-entry term on every entry."""
    for kdim, k, dts, force, path in GRAM_REAL:
        if path != 1:
            continue
        for family in ("normal", "scaled"):
            v = _gram_real_values(kdim, k, np.float32, family)
            emu, amax = _split_emulated(v)
            a = np.abs(v.astype(np.float64))
            bar = 2.0 ** -20 * (a.T @ a) + _split_small_term(amax, a.sum(axis=0))
            ratio = float(np.max(np.abs(emu - _hi_gram(v)) / bar))
            report("gram split emulation %6d x %4d %-6s  max err / split term %.3f" % (kdim, k, family, ratio))
            assert ratio <= 1.0, (kdim, k, family, ratio)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["normal", "scaled"])
def test_gram_real_data_within_the_derived_bar(dtype, family, monkeypatch):
    """|G^ - G_ref| <= beta(kdim) (|P|^T |P|) entry by entry on the lower tiles; an fp64 product that accumulated anything
    in fp32 would miss this by orders of magnitude."""
    monkeypatch.delenv("POGS_AMD_GRAM", raising=False)
    monkeypatch.delenv("POGS_AMD_GRAM_TILE", raising=False)
    for kdim, k, dts, force, path in GRAM_REAL:
        if dtype not in dts:
            continue
        v = _gram_real_values(kdim, k, dtype, family)
        P, G0 = _gram_operand(dtype, kdim, k, v)
        G, info = _lib.gram_check(P, k, G0, force=force, num_cu=256)
        assert info["path"] == path, (kdim, k, info)
        bar = _gram_bar(np.abs(v.astype(np.float64)), kdim, dtype, path == 1, float(np.max(np.abs(v))))
        mask = _tile_mask(k)
        got = G[:, :k]
        assert np.all(np.isfinite(got[mask]))
        ratio = float(np.max((np.abs(hi(got) - _hi_gram(v)) / bar)[mask]))
        report("gram %s %-6s %6d x %4d force %3d path %d tile %3d ksplit %2d kacc %4d units %d  max err / bar %.2e"
               % (tname(dtype), family, kdim, k, force, info["path"], info["tile"], info["ksplit"], info["kacc"],
                  info["units"], ratio))
        assert ratio <= 1.0, (kdim, k, family, info, ratio)
        if path == 0:   # the diagonal tiles are computed whole: the same products in the same order on both sides
            d = min(k, 128)
            assert same_bytes(got[:d, :d], got[:d, :d].T.copy())


# ---- Cholesky, L^-1, transpose ----------------------------------------------------------------------------------------

CHOL_NS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 385, 513, 1000, 1025, 2049]
CHOL_BIG = 4097
R_BAR = {"gaussian": 4.0, "correlated": 32.0}
_cases = {}


def _spd(n, dt, family):
    """H = I + A^T A, ||A||_F^2 = n (1 <= lambda(H) <= 1 + n, the range factor() sees), rounded to the working type"""
    rng = np.random.default_rng(1000 * n + (7 if family == "gaussian" else 11))
    if family == "gaussian":
        A = rng.standard_normal((3 * n, n))
    else:
        A = (0.05 * rng.standard_normal((3 * n, n)) + rng.standard_normal((3 * n, 1))) * np.exp(rng.uniform(-2, 2, (1, n)))
    A *= np.sqrt(n) / np.linalg.norm(A)
    return (np.eye(n) + A.T @ A).astype(dt)


class Ref:
    """LAPACK in the working type and a reference beyond it for one matrix, and the residuals of a factor against them.

    H_hi: the matrix the residuals are taken against -- float64 for fp32 data, long double for fp64 data.  H_work: what
    LAPACK factorises in the working type (the same matrix, rounded).
    fp64 data: nothing here multiplies n x n long double matrices the slow way.  With L0, W0 the fp64 LAPACK factor and
    inverse, E = H - L0 L0^T and F = W0 L0 - I (xmatmul) are of the order of 1e-13, so everything else is a product with
    a small matrix, for which fp64 is plenty:
      W_ref:  H = L0 (I + S) L0^T with S = L0^-1 E L0^-T, so L = L0 (I + Phi), Phi = strict lower of S + half its
              diagonal (to first order; the second order is 1e-26), and L0^-1 = (I + F)^-1 W0:  W = (I - Phi)(I - F) W0.
      rho_W:  W^ H W^T - I = D + D^T + D D^T + W^ E W^T  with D = W^ L0 - I."""

    def __init__(self, H_work, H_hi=None):
        dt = H_work.dtype.type
        n = H_work.shape[0]
        self.dt, self.n = dt, n
        self.H = hi(H_work) if H_hi is None else H_hi
        eye = np.eye(n, dtype=dt)
        self.L_lap = np.linalg.cholesky(H_work)
        self.W_lap = sla.solve_triangular(self.L_lap, eye, lower=True, check_finite=False)
        assert self.L_lap.dtype == dt and self.W_lap.dtype == dt       # LAPACK ran in the working type
        if dt == np.float32:
            self.W_ref = sla.solve_triangular(np.linalg.cholesky(self.H), np.eye(n), lower=True, check_finite=False)
        else:
            H64 = self.H.astype(np.float64)
            self.L0 = np.linalg.cholesky(H64)
            self.W0 = sla.solve_triangular(self.L0, np.eye(n), lower=True, check_finite=False)
            self.E = self.H - xmatmul(self.L0, self.L0.T)
            self.E64 = self.E.astype(np.float64)
            F = xmatmul(self.W0, self.L0) - np.eye(n)
            S = self.W0 @ self.E64 @ self.W0.T
            Phi = np.tril(S, -1) + np.diag(np.diag(S)) / 2
            self.W_ref = self.W0.astype(np.longdouble) - (Phi + F.astype(np.float64)) @ self.W0

    def rho_L(self, L):
        L = np.tril(L)
        prod = hi(L) @ hi(L).T if self.dt == np.float32 else xmatmul(L, L.T)
        return float(np.linalg.norm(np.tril(self.H - prod).astype(np.float64)) / np.linalg.norm(L.astype(np.float64)) ** 2)

    def rho_W(self, W):
        W = np.tril(W)
        if self.dt == np.float32:
            W64 = W.astype(np.float64)
            return float(np.max(np.abs(W64 @ self.H @ W64.T - np.eye(self.n))))
        D = xmatmul(W, self.L0) - np.eye(self.n)
        D64 = D.astype(np.float64)
        return float(np.max(np.abs(D + D.T + D64 @ D64.T + W @ self.E64 @ W.T)))

    def w_diff(self, W):
        return float(np.max(np.abs(hi(np.tril(W)) - self.W_ref)))

    def lapack(self):
        if not hasattr(self, "_lap"):
            self._lap = (self.rho_L(self.L_lap), self.rho_W(self.W_lap), self.w_diff(self.W_lap))
        return self._lap


def _case(n, dt, family):
    """(H, Ref) of a case, made once per module (the references at n > 2049 are the slow part)"""
    key = (n, np.dtype(dt).name, family)
    if key not in _cases:
        H = _spd(n, dt, family)
        _cases[key] = (H, Ref(H))
    return _cases[key]


def restated_block(B):
    """potrf_inv_kernel in numpy: right-looking, one column per step -- the pivot's square root, the column and row j of
    X = L^-1 times the pivot's reciprocal, then a rank-one update of what lies to the right (L) and below (X).  Every
    element is thus a SEQUENTIAL sum of up to NB terms in the working type, where LAPACK's blocked dot products add
    them in a few interleaved partial sums: in fp32 with NB = 128 that alone costs a factor of 2.5 .. 5 against LAPACK."""
    dt = B.dtype.type
    nb = B.shape[0]
    L, X = np.tril(B).copy(), np.eye(nb, dtype=dt)
    for j in range(nb):
        ljj = np.sqrt(L[j, j])
        inv = dt(1) / ljj
        col, xr = L[j + 1:, j] * inv, X[j, :j + 1] * inv
        L[j, j], L[j + 1:, j], X[j, :j + 1] = ljj, col, xr
        L[j + 1:, j + 1:] -= np.tril(np.outer(col, col))
        X[j + 1:, :j + 1] -= np.outer(col, xr)
    return L, X


def restated_factor(H):
    """The algorithm of cholesky_lower + trtri_lower in numpy, every product rounded to the working type: panels of NB
    columns in groups, left-looking inside a group, one trailing update per group; a diagonal block by restated_block; a
    panel is solved by multiplying with the explicit inverse of its diagonal block; the inverse is completed by
    recursive doubling (W_ba = -W_bb (L_ba W_aa))."""
    dt = H.dtype.type
    n, nb_, grp = H.shape[0], NB[dt], GROUP[dt]
    G, W = np.tril(H).copy(), np.zeros_like(H)
    o = 0
    while o < n:
        done = 0
        for j in range(grp):
            oj = o + done
            if oj >= n:
                break
            nb = min(nb_, n - oj)
            if j > 0:
                G[oj:, oj:oj + nb] -= G[oj:, o:oj] @ G[oj:oj + nb, o:oj].T
            Ld, Xd = restated_block(G[oj:oj + nb, oj:oj + nb])
            G[oj:oj + nb, oj:oj + nb], W[oj:oj + nb, oj:oj + nb] = Ld, Xd
            if oj + nb < n:
                G[oj + nb:, oj:oj + nb] = G[oj + nb:, oj:oj + nb] @ Xd.T
            done += nb
        o3 = o + done
        if o3 < n:
            G[o3:, o3:] -= G[o3:, o:o3] @ G[o3:, o:o3].T
        o = o3
    L = np.tril(G)
    sz = nb_
    while sz < n:
        for o in range(0, n, 2 * sz):
            if o + sz >= n:
                break
            a, b = slice(o, o + sz), slice(o + sz, min(o + 2 * sz, n))
            W[b, a] = -(W[b, b] @ (L[b, a] @ W[a, a]))
        sz *= 2
    assert L.dtype == dt and W.dtype == dt
    return L, W


def _ratios(ref, L, W):
    lap = ref.lapack()
    got = (ref.rho_L(L), ref.rho_W(W), ref.w_diff(W))
    return got, lap


def _chol_ns(dt, family):
    """both types and families at every n of CHOL_NS; n = 4097 in fp32 on both families, in fp64 on the Gaussian one (its
    references are ten fp64 products of that size per extended-precision product: the slow part of the file)"""
    return CHOL_NS + ([CHOL_BIG] if dt == np.float32 or family == "gaussian" else [])


def _restated(n, dt, family):
    """(rho_L, rho_W, |W - W_ref|) of the numpy restatement on a case's matrix, once per module"""
    key = (n, np.dtype(dt).name, family)
    if key not in _restated_cache:
        H, ref = _case(n, dt, family)
        L, W = restated_factor(H)
        _restated_cache[key] = (ref.rho_L(L), ref.rho_W(W), ref.w_diff(W))
    return _restated_cache[key]


_restated_cache = {}


def _bars(n, dt, family):
    """The bar of each of the three quantities, as a multiple of LAPACK's: R = 4 (Gaussian) / 32 (correlated) -- what a
    restatement whose diagonal blocks are LAPACK's reaches in rho_L and rho_W (about 2 x LAPACK on the Gaussian family,
    16 x on the correlated one), times 2 for an accumulate that truncates where numpy rounds.  The restatement that also
    factorises the diagonal blocks as the kernel does (restated_block: sequential sums of up to NB terms) exceeds R / 2 at
    many n:
    2.5 - 5.2 x LAPACK in fp32 and 1.4 - 3.4 x in fp64 on the Gaussian family, up to 21 x (rho_L, rho_W) and 51 x
    (|W - W_ref|) in fp32 on the correlated one (profiles/factor_accuracy.txt).  Where it does, R is twice the
    restatement's own ratio at that n, type and family -- taken from the restatement as it runs here, never from the
    kernel."""
    lap = _case(n, dt, family)[1].lapack()
    rst = _restated(n, dt, family)
    return tuple(max(R_BAR[family], 2.0 * r / l_) * l_ if l_ > 0 else 0.0 for r, l_ in zip(rst, lap))


def _fmt(tag, dt, family, n, got, lap):
    x = [g / l_ if l_ else 1.0 for g, l_ in zip(got, lap)]
    return ("%-8s %s %-10s n %4d  rho_L %.2e (x%5.2f LAPACK)  rho_W %.2e (x%5.2f)  |W - W_ref| %.2e (x%5.2f)"
            % (tag, tname(dt), family, n, got[0], x[0], got[1], x[1], got[2], x[2]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["gaussian", "correlated"])
def test_restated_algorithm_against_lapack(dtype, family):
    """Where the bars of the GPU test come from, checked wherever the suite runs: the numpy restatement of the algorithm
    on the very matrices of the GPU test.  It stays inside the worst-case bars (any order of summation does), and its
    ratio to LAPACK, which sets the bar of the kernel wherever it exceeds R / 2 (_bars), is printed per case."""
    for n in _chol_ns(dtype, family):
        ref = _case(n, dtype, family)[1]
        got, lap = _restated(n, dtype, family), ref.lapack()
        report(_fmt("restated", dtype, family, n, got, lap))
        res_bar, w_bar = _w_bars(n, n, dtype, gram=False)
        if dtype == np.float64 or res_bar < 0.5:
            assert got[0] <= gamma(n + 1, dtype) and got[1] <= res_bar and got[2] <= w_bar, (n, got, res_bar, w_bar)
        assert all(np.isfinite(b) for b in _bars(n, dtype, family))


def _structure(n, dt, L, W, U, H):
    ld = rup(n, vec(dt))
    assert L.shape == (n, ld)
    iu = np.triu_indices(n, 1)
    assert np.all(W[:, :n][iu] == 0) and np.all(U[:, :n].T[iu] == 0)
    assert same_bytes(U[:, :n], W[:, :n].T.copy())
    for M in (L, W, U):
        assert np.all(M[:, n:] == 0)                 # the columns n .. ld of the slabs
    assert same_bytes(L[:, :n][iu], H[iu])            # not written: what H held above the diagonal


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["gaussian", "correlated"])
def test_cholesky_and_inverse_against_lapack_in_the_working_type(dtype, family):
    """rho_L, rho_W and |W^ - W_ref| of the kernels' factor at most R times those of numpy.linalg.cholesky /
    scipy.linalg.solve_triangular run in the same type on the same H (R: _bars); the worst-case bars as a backstop;
    structure; and the same bytes from a second run.  The strict upper triangle of the H handed in is NaN: only the lower
    one may be read."""
    for n in _chol_ns(dtype, family):
        H, ref = _case(n, dtype, family)
        Hin = H.copy()
        Hin[np.triu_indices(n, 1)] = np.nan
        ld = rup(n, vec(dtype))
        first = _lib.chol_check(Hin, ldo=ld)
        L, W, U = first
        _structure(n, dtype, L, W, U, Hin)
        L, W = L[:, :n], W[:, :n]
        assert np.all(np.isfinite(np.tril(L))) and np.all(np.isfinite(W))
        got, lap = _ratios(ref, L, W)
        report(_fmt("kernel", dtype, family, n, got, lap))
        for g, bar in zip(got, _bars(n, dtype, family)):
            assert g <= bar or g == 0.0, (n, family, got, lap, _restated(n, dtype, family))
        # the backstop that holds for any order of summation
        res_bar, w_bar = _w_bars(n, n, dtype, gram=False)
        if dtype == np.float64 or res_bar < 0.5:
            assert got[0] <= gamma(n + 1, dtype) and got[1] <= res_bar and got[2] <= w_bar, (n, got, res_bar, w_bar)
        if n in (129, 1000, 2049):
            assert all(same_bytes(a, b) for a, b in zip(_lib.chol_check(Hin, ldo=ld), first)), n


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_cholesky_of_the_identity_and_of_powers_of_four_is_exact(dtype):
    """H = I and H = diag(4^e): L = diag(2^e) and W = diag(2^-e) exactly.  Compared value by value, not as bytes: the
    inverse's off-diagonal blocks are alpha = -1 times an exact zero product, i.e. -0.0."""
    rng = np.random.default_rng(303)
    for n in CHOL_NS:
        for e in (np.zeros(n), rng.integers(-3, 4, n).astype(np.float64)):
            H = np.diag(4.0 ** e).astype(dtype)
            L, W, U = _lib.chol_check(H, ldo=rup(n, vec(dtype)))
            _structure(n, dtype, L, W, U, H)
            assert np.array_equal(L[:, :n], np.diag(2.0 ** e).astype(dtype)), n
            assert np.array_equal(W[:, :n], np.diag(2.0 ** -e).astype(dtype)), n
            assert same_bytes(np.diag(L[:, :n]).copy(), (2.0 ** e).astype(dtype))
            assert same_bytes(np.diag(W[:, :n]).copy(), (2.0 ** -e).astype(dtype))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_matrix_that_is_not_positive_definite_gives_nan_not_a_hang(dtype):
    """A negative pivot at column p = 200 of 300.  The diagonal-block kernel updates its registers in 16-row groups, and a
    row of the pivot's group that lies above the pivot takes part in the pivot's step with a zero coefficient: zero times
    the NaN reciprocal is NaN, so X = L11^-1 is NaN from the first row of that group (p16 = 192) on, and with it the
    columns p16 .. p of the panel below.  Pinned: L's columns before p16 as for the good matrix (same bytes), NaN in L's
    lower triangle from column p on; W's lower triangle NaN in every row from p on, the rows before the pivot's 128-row
    tile as for the good matrix (inside the tile a zero of W's upper part meets a NaN).  No hang, no fault, and the entry
    works afterwards."""
    n, p = 300, 200
    p16 = p - p % 16
    H = _spd(n, dtype, "gaussian")
    good = _lib.chol_check(H)
    bad = H.copy()
    bad[p, p] = -1.0
    L, W, U = _lib.chol_check(bad)
    rows, cols = np.tril_indices(n)
    assert same_bytes(L[:, :p16], good[0][:, :p16])
    assert np.all(np.isnan(L[rows, cols][cols >= p]))
    assert np.all(np.isnan(W[rows, cols][rows >= p]))
    assert same_bytes(W[:p // 128 * 128], good[1][:p // 128 * 128])
    assert same_bytes(U, W.T.copy())
    assert all(same_bytes(a, b) for a, b in zip(_lib.chol_check(H), good))


# ---- the factor a handle holds ----------------------------------------------------------------------------------------

def restated_gram(S, info):
    """The native Gram product's order of summation in numpy (gemm.hip: gemm_body): every K range of `unit_rows` rows is
    ONE chain -- a matrix-core step adds its four rows one after the other to the running sum, in the working type -- and
    the ranges are added in order.  A chain of 3000 terms is what sets this product apart from a BLAS, which keeps
    several interleaved sums."""
    kdim, k = S.shape
    G = np.zeros((k, k), S.dtype)
    tmp = np.empty((k, k), S.dtype)
    for u0 in range(0, kdim, info["unit_rows"]):
        acc = np.zeros((k, k), S.dtype)
        for r in range(u0, min(u0 + info["unit_rows"], kdim)):
            np.multiply.outer(S[r], S[r], out=tmp)
            acc += tmp
        G += acc
    return G


def _handle_check(dt, A_eq_full, Ws, label):
    """Every W of Ws (one per rank) against H = I + A_eq^T A_eq (or A_eq A_eq^T) of the whole equilibrated matrix, formed
    beyond the working precision.  The comparator is the whole pipeline in the working type on the CPU: BLAS Gram + I,
    LAPACK factor and inverse; bar: R = 4 times its rho_W -- and, by the rule of _bars, twice the ratio of the numpy
    restatement of the pipeline (restated_gram where the native product is the live path and K is short enough to restate,
    then restated_factor) where that is more."""
    m, n = A_eq_full.shape
    K = min(m, n)
    S = A_eq_full if m > n else A_eq_full.T                      # K-major: H = I + S^T S
    if dt == np.float32:
        S64 = S.astype(np.float64)
        H_hi = np.eye(K) + S64.T @ S64
    else:
        H_hi = np.eye(K, dtype=np.longdouble) + xmatmul(S.T, S)
    H_work = (S.T @ S + np.eye(K, dtype=dt)).astype(dt)          # the pipeline in the working type: BLAS Gram + I
    assert H_work.dtype == dt
    ref = Ref(H_work, H_hi)
    lap_res, lap_w = ref.rho_W(ref.W_lap), ref.w_diff(ref.W_lap)
    # R = 4 as on the Gaussian family above, and by the same rule (_bars) twice the restatement's ratio where that is more
    H_rst = H_work
    if S.shape[0] <= 4096:
        lda = rup(K, vec(dt))
        Sp = np.zeros((S.shape[0], lda), dt)
        Sp[:, :K] = S
        info = _lib.gram_check(Sp, K, np.zeros((K, K), dt))[1]
        if info["path"] == 0 and info["kacc"] == 0:
            H_rst = restated_gram(np.ascontiguousarray(S), info) + np.eye(K, dtype=dt)
    rst_res = ref.rho_W(restated_factor(H_rst)[1])
    R = max(4.0, 2.0 * rst_res / lap_res)
    res_bar, w_bar = _w_bars(m, n, dt)
    for r, W in enumerate(Ws):
        assert same_bytes(W, Ws[0]), (label, r)
    W = Ws[0]
    assert np.all(W[np.triu_indices(K, 1)] == 0)
    res, wd = ref.rho_W(W), ref.w_diff(W)
    report("handle   %s %-40s rho_W %.2e (x%.2f of the CPU pipeline in %s; restated x%.2f)  |W - W_ref| %.2e (x%.2f)"
           % (tname(dt), label, res, res / lap_res, tname(dt), rst_res / lap_res, wd, wd / lap_w))
    assert res <= R * lap_res, (label, res, lap_res, R)
    if res_bar < 0.5:
        assert res <= res_bar and wd <= w_bar, (label, res, res_bar, wd, w_bar)


def _solver_factor(dt, A, order=None, **kw):
    import pogs_amd

    if order is not None:
        kw["order"] = order
    with pogs_amd.Solver(A, dtype=dt, **kw) as s:
        A_eq = s.equilibrated()[0]
        W, U = s.factor()
    assert same_bytes(U, W.T.copy())
    return A_eq, W


HANDLE_SHAPES = [((3000, 1100), np.float32), ((3000, 1100), np.float64), ((20000, 1500), np.float32),
                 ((1300, 21000), np.float32), ((400, 3000), np.float64)]


@gpu
@pytest.mark.parametrize("shape,dtype", HANDLE_SHAPES)
def test_the_factor_of_a_handle_tall_and_wide(shape, dtype):
    from pogs_amd import synth

    A = synth.dense_lasso(shape[0], shape[1], seed=71, dtype=dtype)[0]
    A_eq, W = _solver_factor(dtype, A)
    _handle_check(dtype, A_eq, [W], "%d x %d" % shape)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_factor_of_a_handle_windowed_and_column_major(dtype, monkeypatch):
    import pogs_amd
    from pogs_amd import synth

    A = synth.dense_lasso(900, 300, seed=73, dtype=dtype)[0]
    A_eq0, W0 = _solver_factor(dtype, A)
    A_eq, W = _solver_factor(dtype, np.asfortranarray(A), order=pogs_amd.Ordering.COL_MAJ)
    assert same_bytes(A_eq, A_eq0) and same_bytes(W, W0)
    _handle_check(dtype, A_eq, [W], "900 x 300 column-major")
    monkeypatch.setenv("POGS_AMD_XL_LIMIT", "40")
    A_eq, W = _solver_factor(dtype, A)
    _handle_check(dtype, A_eq, [W], "900 x 300 windowed")


@gpu
@pytest.mark.parametrize("dtype,bounds", [(np.float64, (0, 1500, 3000)), (np.float32, (0, 700, 2100, 3000)),
                                          (np.float32, (0, 1000, 2000, 3000))])
def test_the_factor_of_row_sharded_handles(dtype, bounds, monkeypatch):
    """Two and three row shards (equal and unequal) through the in-process test communicator: every rank's W is the
    factor of the WHOLE matrix, and all ranks hold the same bytes."""
    import pogs_amd
    from pogs_amd import synth

    monkeypatch.setenv("POGS_AMD_TEST_TRANSPORT", "1")
    m, n = 3000, 1100
    A = synth.dense_lasso(m, n, seed=79, dtype=dtype)[0]
    world = len(bounds) - 1
    uid = (b"POGSLOCAL:" + os.urandom(8).hex().encode()).ljust(128, b"\0")
    out, errors = [None] * world, []

    def work(r):
        try:
            lo, hi_ = bounds[r], bounds[r + 1]
            with pogs_amd.Solver(A[lo:hi_], dtype=dtype, dist=(r, world, m, uid)) as s:
                out[r] = (s.equilibrated()[0], s.factor()[0])
        except Exception as e:  # pragma: no cover - surfaced below
            errors.append((r, e))

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(600)
    assert not errors, errors
    _handle_check(dtype, np.concatenate([o[0] for o in out]), [o[1] for o in out], "3000 x 1100, shards %s" % (bounds,))


@gpu
def test_get_factor_refuses_a_sparse_and_a_cgls_handle_then_serves_a_dense_one():
    import scipy.sparse as sp

    import pogs_amd
    from pogs_amd import synth

    with pogs_amd.Solver(sp.random(60, 20, 0.3, random_state=1, format="csr"), dtype=np.float64) as s:
        with pytest.raises(RuntimeError, match="needs a dense handle"):
            s.factor()
    A = synth.dense_lasso(300, 40, seed=3, dtype=np.float32)[0]
    with pogs_amd.Solver(A, dtype=np.float32, projector=_lib.PROJ_CGLS) as s:
        with pytest.raises(RuntimeError, match="CGLS projector"):
            s.factor()
    with pytest.raises(RuntimeError, match="n must be >= 1"):
        _lib.chol_check(np.zeros((0, 0), np.float32))
    A_eq, W = _solver_factor(np.float32, A)
    _handle_check(np.float32, A_eq, [W], "300 x 40 after refusals")
    H = _spd(65, np.float64, "gaussian")
    L, W, U = _lib.chol_check(H)
    assert np.max(np.abs(np.tril(L) @ np.tril(L).T - H)) < 1e-12 * 65
    G, info = _lib.gram_check(np.ones((8, 4), np.float32), 3, np.zeros((3, 3), np.float32), num_cu=0)
    assert np.array_equal(G, np.full((3, 3), 8, np.float32)) and info["path"] == 0
