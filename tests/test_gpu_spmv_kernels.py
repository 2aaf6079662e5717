"""The product of the solo sparse solver on its own -- both CSR copies (the second transposed on the device), the tiled
lane-stream copies (csrc/sell.h) in both storage formats, the plain CSR kernel, the column-group reduction -- through
PogsAmdSpmvCheck (include/pogs_amd.h, Part 3), which runs the solver's own SparseOperator (csrc/sparse_operator.h: its
build_structure / build_sell, scale, finalize_values and spmv) on HOST arrays without a solver and without the
equilibration, against references formed in fp64 (fp32 data) or long double (fp64 data).

Every case names the path it must reach and asserts it from `info`, so a case that stops reaching its path fails.
num_cu = 256 in every case; BW x RR = 18432 x 16384 (fp32), 12288 x 6144 (fp64): columns per block, rows per range.

Geometry build_sell must choose (format 0, the two environment switches cleared), for the copy A of the shape:

    shape (nnz)                 fp32                               fp64
    below one tile              rr 512, ncb 1, ncg 1               the same
    513 x 700                   nrr 2                              nrr 2
    3000 x 18433 (30 000)       ncb 2, ncg 2                       ncb 2, ncg 2
    3000 x 12289 (30 000)       ncb 1, ncg 1                       ncb 2, ncg 2
    600 x 40000 (6 000)         ncb 3, ncg 3                       ncb 4, ncg 4
    2000 x 600000 (40 000)      ncb 33, ncg 17 (uneven split)      ncb 49, ncg 25
    20000 x 600000 (300 000)    rr 1344, nrr 15, ncg 17            rr 1472, ncg 17 (the second look changes 1920)

Structures (each as CSR and as CSC input, both products, formats 1 = tags, 2 = two id slots, 3 = plain kernel):

    1 x 1, 1 x 700, 700 x 1, one non-empty row, empty rows at both ends of a row range      tiled, rr 512, one block
    row lengths 1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 4095, 4096, 4097 in one tile       tiled; plain: kSpCap = 4096
                                                  and the whole-workgroup long row (4097)
    every row one element (8192^2), rr 4096       format 0 keeps tags on both copies (two slots would pad every batch)
    every row and column two elements (4000^2)    format 0 picks two id slots in fp32 on both copies
    (RR + 1) x 300, every row non-empty, force_rr_rows = RR       rr = RR: 32 rows per stream, a second range of one row
    (RR + 1) x (BW + 1), force_rr_rows = RR, force_ncg = 1, 2     the same height with one and with ncb = 2 groups
    RR x 300, only rows = 0 mod 32 non-empty, force_rr_rows = RR  RR / 32 rows on the 16 streams of one residue, budget of
                                                  one batch: most rows go through the planner's overflow list (reached
                                                  by construction: ~2 entries per row against a budget of 4 per stream;
                                                  `info` has no field that shows it)
    RR x 300, force_rr_rows = RR: 511 rows of 256 entries, 16 per residue but 15 in one, and 200 (fp64: 150)
    single-element rows of one residue            budget 256: 511 streams are full, the single-element rows all overflow
                                                  onto the one empty stream until its 7-bit row count stands at 127;
                                                  the other 73 (23) go over budget to the least loaded streams, which
                                                  makes the tile 260 long instead of 256: tiled, 2080 units of 64
    40 x (2 BW + 1), 40 x (2 BW - 1)              an element in the last column where ncols % BW is 1 and BW - 1, and in
                                                  the first and last column of every block
    600 x 30000, one row of 18000 entries among single-element rows    A falls back to plain, why = padding
    300 x (3 BW + 5), rows shuffled               column blocks out of order: the counted (non-monotone) branch of
                                                  sell_count_kernel and sell_fill_kernel
    64 x (1025 BW + 7), rows shuffled, fp32       more than kSellFillCb = 1024 column blocks: the prefix-count branch
    200 x 300 with an entry 2, 3 and 64 times     repeated entries add up
    a row (and a column) of 65535 / 65536 / 70000 entries on 7 columns of one block, sorted and not:
                                                  65535: the plan is made, why = padding (512 x 65536 stored elements
                                                  against 4 nnz + 2^22); 65536 and 70000: why = row count over 16 bits.
                                                  All of them return the exact product through the plain kernel.

Checks: exact integers (entries, x in -4 .. 4, scale 1 / 0.5, (alpha, beta) = (1, 0) / (-2, 0.5), sq, x_nrm2 = 4: every
partial sum is an integer multiple of a power of two below 2^24 units, so y equals the fp64 reference cast to the type
and sumsq the fp64 sum of y^2, on every path); scale = 0.5 gives exactly half of scale = 1 (a stale element of the
refill shows); tags and two id slots give the same bytes on real data, and every path the same bytes from a second run;
real data within  gamma_(L_i + ncb + ncg + 4) (|A| |x|)_i  per entry (u = eps / 2: an fma chain of L_i terms rounds once
per term, one addition per tile partial and per group, the x scale and alpha), plus the reference's own L_i eps_hi;
3 sentinels behind y come back unchanged and x carries NaN behind its length.

Device transpose and scans (t_ptr / t_ind / t_val against the transpose with sorted indices, array_equal): row counts of
the built copy 1, 8191, 8192, 8193, 32768 (the last single-kernel scan), 32769, 40961; segment lengths 1, 2, 3, 255, 256,
257, 2047, 2048 (the last LDS sort), 2049, 4097, 5000; repeated entries ordered by the value's bit pattern as unsigned.

Not reachable at test size, so not in the list: the planner's range bits (23- and 22-bit stream offsets: a stream of
millions of elements); more than 127 x 16 rows of ONE residue in a tile (a tile holds at most RR / 32 = 512 of them: a
stream's row count runs out through the overflow placement instead, the case above); a row of 65535 entries that stays
tiled (the padding rule needs 7.3 million non-zeros next to it).

The real-data test prints its largest error / bar ratio per structure (pytest -s); no measured number enters an
assertion."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import gamma, hi, ints, same_bytes, scaled_normal
from pogs_amd import _lib

gpu = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
SENTINEL = -7.375e-3
BW = {np.float32: 18432, np.float64: 12288}    # sell.h: SellCfg<T>::BW
RR = {np.float32: 16384, np.float64: 6144}     # sell.h: SellCfg<T>::RR
CSR, CSC = _lib.ROW_MAJ, _lib.COL_MAJ
TAGS, TWO, PLAIN = _lib.SPMV_TAGS, _lib.SPMV_TWO, _lib.SPMV_PLAIN
WHY_PADDING, WHY_COUNT, WHY_PINNED = 4, 5, 6


def tname(dt):
    return "fp32" if dt == np.float32 else "fp64"


def report(line):
    print("spmv_accuracy: " + line)


class Structure:
    """rows[k], cols[k]: the entries of an m x n matrix in the order they are handed over inside a row (CSR input) or a
    column (CSC input); entries may repeat."""

    def __init__(self, name, m, n, rows, cols):
        self.name, self.m, self.n = name, int(m), int(n)
        self.rows, self.cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        assert self.rows.size == self.cols.size and self.rows.size > 0
        assert 0 <= self.rows.min() and self.rows.max() < m and 0 <= self.cols.min() and self.cols.max() < n
        self.nnz = self.rows.size
        self._by = {}

    def arrays(self, ord, val):
        """(ptr, ind, val) of the matrix as CSR (rows in given order) or CSC"""
        if ord not in self._by:
            major, minor, nmaj = (self.rows, self.cols, self.m) if ord == CSR else (self.cols, self.rows, self.n)
            perm = np.argsort(major, kind="stable")
            ptr = np.zeros(nmaj + 1, np.int32)
            ptr[1:] = np.cumsum(np.bincount(major, minlength=nmaj))
            self._by[ord] = (ptr, minor[perm].astype(np.int32), perm)
        ptr, ind, perm = self._by[ord]
        return ptr, ind, val[perm]


def product(S, val, x, trans, dt_hi):
    """(op(A) x, |op(A)| |x|, entries per row of op(A)) with every product and sum in dt_hi"""
    ptr, ind, v = S.arrays(CSR if trans == "n" else CSC, val)
    v, xg = v.astype(dt_hi), x.astype(dt_hi)[ind]
    ne = np.diff(ptr) > 0
    out, absout = np.zeros(ptr.size - 1, dt_hi), np.zeros(ptr.size - 1, dt_hi)
    out[ne] = np.add.reduceat(v * xg, ptr[:-1][ne])
    absout[ne] = np.add.reduceat(np.abs(v * xg), ptr[:-1][ne])
    return out, absout, np.diff(ptr)


def run(S, val, x, y0, dt, ord=CSR, trans="n", fmt=0, **kw):
    """the entry on S with x padded by NaN and y0 by sentinels; returns (y, sumsq, info of the product's copy, both infos)"""
    nin, nout = (S.n, S.m) if trans == "n" else (S.m, S.n)
    assert x.size == nin and y0.size == nout
    xp = np.concatenate([x, np.full(2, np.nan, dt)]).astype(dt)
    yp = np.concatenate([y0, np.full(3, SENTINEL, dt)]).astype(dt)
    ptr, ind, v = S.arrays(ord, val)
    out = _lib.spmv_check(ptr, ind, v.astype(dt), (S.m, S.n), xp, yp, trans=trans, ord=ord, num_cu=256, format=fmt, **kw)
    y, sumsq, infos = out[0], out[1], out[2]
    assert same_bytes(y[nout:], np.full(3, SENTINEL, dt)), (S.name, "wrote behind y")
    return (y[:nout], sumsq, infos[0 if trans == "n" else 1], infos) + tuple(out[3:])


def want_info(info, want, case):
    for key, v in want.items():
        assert info[key] == v, (case, key, info)


# (scale, alpha, beta, sq, x_nrm2): all 16 combinations of the issue's values, cycled over the runs of a structure
PARAMS = [(sc, al, be, sq, xn) for sq in (0, 1) for xn in (0.0, 4.0) for (al, be) in ((1.0, 0.0), (-2.0, 0.5))
          for sc in (1.0, 0.5)]


def exact_reference(S, val, x, y0, trans, scale, alpha, beta, sq, x_nrm2, dt):
    v = val.astype(np.float64) * scale
    v = v * v if sq else v
    xs = 1.0 / np.sqrt(x_nrm2) if x_nrm2 else 1.0
    dot = product(S, v, x.astype(np.float64) * xs, trans, np.float64)[0]
    y = alpha * dot + (beta * y0.astype(np.float64) if beta else 0.0)
    assert np.array_equal(y.astype(dt).astype(np.float64), y), "the case is not exact in the type"
    return y.astype(dt), float(np.sum(y * y))


def exact_runs(S, dt, rng, runs, start=0, val=None):
    """runs: (ord, trans, fmt, want-or-None, kwargs); every run takes the next PARAMS entry.  Returns the infos seen."""
    val = ints(rng, S.nnz, dt) if val is None else val
    seen = []
    for i, (ord, trans, fmt, want, kw) in enumerate(runs):
        scale, alpha, beta, sq, x_nrm2 = PARAMS[(start + i) % len(PARAMS)]
        nin, nout = (S.n, S.m) if trans == "n" else (S.m, S.n)
        x, y0 = ints(rng, nin, dt), ints(rng, nout, dt)
        y, sumsq, info, infos = run(S, val, x, y0, dt, ord, trans, fmt, scale=scale, alpha=alpha, beta=beta, sq=sq,
                                    x_nrm2=x_nrm2, **kw)
        case = (S.name, tname(dt), "csr" if ord == CSR else "csc", trans, fmt, PARAMS[(start + i) % len(PARAMS)], info)
        if fmt == PLAIN:
            want_info(info, dict(tiled=0, why=WHY_PINNED), case)
        elif want is not None:
            want_info(info, want, case)
            if info["tiled"] and fmt in (TAGS, TWO):
                assert info["two"] == (fmt == TWO), case
        ref, ref_sumsq = exact_reference(S, val, x, y0, trans, scale, alpha, beta, sq, x_nrm2, dt)
        assert np.array_equal(y, ref), case + (int(np.argmax(y != ref)),)
        assert sumsq == ref_sumsq, case + (sumsq, ref_sumsq)
        seen.append(info)
    return seen


def all_paths(want=None, want_t=None, **kw):
    """CSR and CSC input, both products, the three pinned formats; want_t: what the copy A^T must report where that
    differs from A's"""
    return [(ord, trans, fmt, want if trans == "n" or want_t is None else want_t, kw)
            for ord in (CSR, CSC) for trans in "nt" for fmt in (TAGS, TWO, PLAIN)]


# ---- structures -----------------------------------------------------------------------------------------------------

def random_structure(name, m, n, nnz, rng, every_row=False):
    """about nnz distinct entries, rows and columns sorted; every_row: no empty row"""
    key = np.unique(rng.integers(0, m * n, nnz))
    rows, cols = key // n, key % n
    if every_row:
        rows, cols = np.concatenate([rows, np.arange(m)]), np.concatenate([cols, rng.integers(0, n, m)])
        key = np.unique(rows * n + cols)
        rows, cols = key // n, key % n
    return Structure(name, m, n, rows, cols)


def shuffled(S, rng):
    perm = rng.permutation(S.nnz)
    return Structure(S.name + " shuffled", S.m, S.n, S.rows[perm], S.cols[perm])


def row_lengths_structure(rng, n=5000):
    lengths = [1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 4095, 4096, 4097]
    rows, cols = [], []
    for r, ln in enumerate(lengths):
        rows.append(np.full(ln, 2 * r + 1))          # an empty row between any two
        cols.append(np.sort(rng.choice(n, ln, replace=False)))
    return Structure("row lengths", 2 * len(lengths) + 1, n, np.concatenate(rows), np.concatenate(cols))


def small_structures(rng):
    one_row = Structure("one non-empty row", 600, 300, np.full(40, 77), np.sort(rng.choice(300, 40, replace=False)))
    base = random_structure("empty rows at the range ends", 1100, 400, 6000, rng)
    keep = ~np.isin(base.rows, np.r_[0:4, 508:516, 1020:1031, 1099])
    ends = Structure(base.name, 1100, 400, base.rows[keep], base.cols[keep])
    return [Structure("1 x 1", 1, 1, [0], [0]), Structure("1 x 700", 1, 700, np.zeros(700, int), np.arange(700)),
            Structure("700 x 1", 700, 1, np.arange(700), np.zeros(700, int)), one_row, ends]


ONE_TILE = dict(tiled=1, rr_rows=512, ncb=1, ncg=1)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_shapes_and_row_lengths_exact_on_every_path(dtype, monkeypatch):
    """The single cases and the row lengths around the planner's classes, the batch of 4 and kSpCap, on every path."""
    monkeypatch.delenv("POGS_AMD_SELL_FORMAT", raising=False)
    monkeypatch.delenv("POGS_AMD_SPMV", raising=False)
    rng = np.random.default_rng(11)
    for S in small_structures(rng):
        seen = exact_runs(S, dtype, rng, all_paths(ONE_TILE) + [(CSR, "n", 0, ONE_TILE, {}), (CSC, "t", 0, ONE_TILE, {})])
        if S.m == 1100:
            assert all(i["nrr"] == 3 for i in seen[:2]), seen[:2]     # A: 512 + 512 + 76 rows
    S = random_structure("513 x 700", 513, 700, 3000, rng)
    exact_runs(S, dtype, rng, [(o, "n", 0, dict(tiled=1, rr_rows=512, nrr=2, ncb=1, ncg=1), {}) for o in (CSR, CSC)] +
               all_paths(dict(tiled=1)), start=3)
    S = row_lengths_structure(rng)
    exact_runs(S, dtype, rng, all_paths(ONE_TILE), start=5)
    exact_runs(shuffled(S, rng), dtype, rng, all_paths(ONE_TILE), start=9)   # one block: shuffled rows stay monotone


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_format_choice_follows_the_padding(dtype, monkeypatch):
    """format 0: single-element rows keep the tags (the two-slot planner pads nearly every batch); two elements per
    (row, tile) take the two id slots in fp32 (7 against 8 bytes per stored element, no padding)."""
    monkeypatch.delenv("POGS_AMD_SELL_FORMAT", raising=False)
    monkeypatch.delenv("POGS_AMD_SPMV", raising=False)
    rng = np.random.default_rng(12)
    # 8192 rows in two ranges of 4096 (forced on the product's copy: at 512 rows a stream holds one row and both layouts
    # are one batch long): 8 single-element rows per stream are 2 batches with tags, 4 with two ends per batch
    S = Structure("single-element rows", 8192, 8192, np.arange(8192), rng.permutation(8192))
    auto = [(o, t, 0, dict(tiled=1, two=0, rr_rows=4096, nrr=2), dict(force_rr_rows=4096)) for o in (CSR, CSC) for t in "nt"]
    exact_runs(S, dtype, rng, auto + all_paths(dict(tiled=1)))
    p = rng.permutation(4000)
    r = np.arange(4000)
    S = Structure("two per row and column", 4000, 4000, np.repeat(r, 2), np.sort(np.stack([p, np.roll(p, -1)], 1), 1).ravel())
    auto = [(o, t, 0, dict(tiled=1, two=1) if dtype == np.float32 else dict(tiled=1), {}) for o in (CSR, CSC) for t in "nt"]
    exact_runs(S, dtype, rng, auto + all_paths(dict(tiled=1)), start=7)


# the table of the module docstring: (m, n, nnz, fp32 geometry of A, fp64 geometry of A)
TABLE = [
    (3000, 18433, 30000, dict(ncb=2, ncg=2), dict(ncb=2, ncg=2)),
    (3000, 12289, 30000, dict(ncb=1, ncg=1), dict(ncb=2, ncg=2)),
    (600, 40000, 6000, dict(ncb=3, ncg=3), dict(ncb=4, ncg=4)),
    (2000, 600000, 40000, dict(rr_rows=512, ncb=33, ncg=17), dict(rr_rows=512, ncb=49, ncg=25)),
    (20000, 600000, 300000, dict(rr_rows=1344, nrr=15, ncb=33, ncg=17), dict(rr_rows=1472, nrr=14, ncb=49, ncg=17)),
]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_geometry_table_and_column_groups_exact(dtype, monkeypatch):
    """What build_sell chooses at num_cu = 256 for the shapes of the table, and the grouped product (partial sums per
    column group, reduce_parts_kernel) exact in both formats; an uneven split of 33 blocks over 17 groups among them."""
    monkeypatch.delenv("POGS_AMD_SELL_FORMAT", raising=False)
    monkeypatch.delenv("POGS_AMD_SPMV", raising=False)
    rng = np.random.default_rng(13)
    for k, (m, n, nnz, g32, g64) in enumerate(TABLE):
        S = random_structure("%d x %d" % (m, n), m, n, nnz, rng)
        want = dict(tiled=1, **(g32 if dtype == np.float32 else g64))
        runs = [(o, "n", 0, want, {}) for o in (CSR, CSC)] + [(CSR, "n", TAGS, want, {}), (CSC, "n", TWO, want, {}),
                                                             (CSR, "t", 0, dict(tiled=1), {}), (CSC, "t", TAGS, None, {}),
                                                             (CSR, "t", TWO, None, {}), (CSR, "n", PLAIN, None, {}),
                                                             (CSC, "t", PLAIN, None, {})]
        exact_runs(S, dtype, rng, runs, start=3 * k)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_lds_limit_height_forced_groups_and_overflow_list(dtype):
    """force_rr_rows = RR: row ranges of the LDS-limit height (32 rows per stream) with a second range of one row, with
    one and with two column groups; and RR / 32 rows of one residue on their 16 streams (the overflow list places most)."""
    rng = np.random.default_rng(14)
    rr, bw = RR[dtype], BW[dtype]
    S = random_structure("(RR + 1) x 300", rr + 1, 300, 2 * rr, rng, every_row=True)
    want = dict(tiled=1, rr_rows=rr, nrr=2, ncb=1, ncg=1)
    exact_runs(S, dtype, rng, [(o, "n", f, want, dict(force_rr_rows=rr)) for o in (CSR, CSC) for f in (TAGS, TWO)])
    S = random_structure("(RR + 1) x (BW + 1)", rr + 1, bw + 1, 2 * rr, rng, every_row=True)
    S = Structure(S.name, S.m, S.n, np.append(S.rows, rr), np.append(S.cols, bw))     # the last row, the last column
    for ncg in (1, 2):
        want = dict(tiled=1, rr_rows=rr, nrr=2, ncb=2, ncg=ncg)
        exact_runs(S, dtype, rng, [(o, "n", f, want, dict(force_rr_rows=rr, force_ncg=ncg))
                                   for o in (CSR, CSC) for f in (TAGS, TWO)], start=4 * ncg)
    # the same matrix from the other side: A^T is the forced copy
    want = dict(tiled=1, rr_rows=512, ncb=1, ncg=1)
    exact_runs(S, dtype, rng, [(CSR, "t", TAGS, want, dict(force_rr_rows=512)), (CSC, "t", TWO, want, dict(force_rr_rows=512))])
    nres = rr // 32
    rows = np.repeat(np.arange(nres) * 32, rng.integers(1, 4, nres))
    S = Structure("one residue", rr, 300, rows, rng.integers(0, 300, rows.size))
    S = Structure(S.name, S.m, S.n, *np.unique(np.stack([S.rows, S.cols]), axis=1))
    want = dict(tiled=1, rr_rows=rr, nrr=1, ncb=1, ncg=1)
    exact_runs(S, dtype, rng, [(o, "n", f, want, dict(force_rr_rows=rr)) for o in (CSR, CSC) for f in (TAGS, TWO)], start=2)


def full_streams_structure(dt, rng):
    """RR x 300: every residue (row mod 32) has 16 rows of 256 entries, residue 9 only 15; residue 5 has 200 (fp64: 150)
    single-element rows besides.  The budget is 256 (the longest row; the mean is just below), so the serpentine deal
    fills 511 streams, leaves one of residue 9 empty and sends every single-element row to the overflow list."""
    rr, nshort = RR[dt], 200 if dt == np.float32 else 150
    rows, cols = [], []
    for q in range(32):
        for i in range(15 if q == 9 else 16):
            rows.append(np.full(256, q + 32 * i))
            cols.append(np.sort(rng.choice(300, 256, replace=False)))
    short = 5 + 32 * (16 + np.arange(nshort))
    assert short.max() < rr
    rows.append(short)
    cols.append(rng.integers(0, 300, nshort))
    return Structure("full streams", rr, 300, np.concatenate(rows), np.concatenate(cols))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_streams_row_count_runs_out_in_the_overflow_placement(dtype):
    """The first-fit overflow placement finds room on one stream only and stops at 127 rows there (`s_cnt < 127`; a row's
    place in its stream has 7 bits); the rest go to the least loaded streams with a count below 127, over the budget.
    Without the count's limit every single-element row would fit the empty stream and the tile would be 256 long (2048
    units); with it 512 streams x 260 elements = 2080 units of 64, in both layouts (the two-slot layout puts two
    single-element rows in a batch of 4: 127 of them end at 253)."""
    rng = np.random.default_rng(21)
    rr = RR[dtype]
    S = full_streams_structure(dtype, rng)
    want = dict(tiled=1, rr_rows=rr, nrr=1, ncb=1, ncg=1, units=2080, why=0)
    exact_runs(S, dtype, rng, [(o, "n", f, want, dict(force_rr_rows=rr)) for o in (CSR, CSC) for f in (TAGS, TWO)] +
               [(CSR, "t", 0, dict(tiled=1), {}), (CSC, "n", PLAIN, None, {})])


def edge_column_structure(dt, n, rng):
    bw = BW[dt]
    nb = (n + bw - 1) // bw
    firsts = np.arange(nb) * bw
    lasts = np.minimum(firsts + bw, n) - 1
    S = random_structure("edge columns", 40, n, 600, rng)
    rows = np.concatenate([S.rows, np.zeros(2 * nb, int), [1], np.full(nb, 39)])
    cols = np.concatenate([S.cols, firsts, lasts, [n - 1], lasts])
    key = np.unique(rows * n + cols)
    return Structure("40 x %d" % n, 40, n, key // n, key % n)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_block_edges_padding_fallback_and_unsorted_rows(dtype, monkeypatch):
    monkeypatch.delenv("POGS_AMD_SELL_FORMAT", raising=False)
    monkeypatch.delenv("POGS_AMD_SPMV", raising=False)
    rng = np.random.default_rng(15)
    bw = BW[dtype]
    # the x slice of the last block is 1 and BW - 1 wide (thread 0's narrow slice; the straddling vector of x_store)
    exact_runs(edge_column_structure(dtype, 2 * bw + 1, rng), dtype, rng, all_paths(dict(tiled=1)))
    exact_runs(edge_column_structure(dtype, 2 * bw - 1, rng), dtype, rng, all_paths(dict(tiled=1)), start=6)
    # one row of 18000 entries (one column block in fp32, 12288 + 5712 in fp64) among 599 single-element rows
    rows = np.concatenate([np.full(18000, 300), np.delete(np.arange(600), 300)])
    cols = np.concatenate([np.arange(18000), rng.integers(0, 30000, 599)])
    S = Structure("600 x 30000, one long row", 600, 30000, rows, cols)
    pad = dict(tiled=0, why=WHY_PADDING)
    exact_runs(S, dtype, rng, [(CSR, "n", 0, pad, {}), (CSC, "n", TAGS, pad, {}), (CSR, "n", TWO, pad, {}),
                               (CSC, "t", 0, dict(tiled=1), {}), (CSR, "t", TWO, dict(tiled=1), {}),
                               (CSR, "n", PLAIN, None, {})], start=1)
    # column blocks out of order inside the rows
    S = shuffled(random_structure("300 x (3 BW + 5)", 300, 3 * bw + 5, 6000, rng), rng)
    exact_runs(S, dtype, rng, all_paths(dict(tiled=1, ncb=4), dict(tiled=1, ncb=1)), start=2)


@gpu
def test_unsorted_rows_over_more_than_1024_column_blocks():
    """fp32, 1026 column blocks: sell_fill_kernel counts a row's earlier elements of the block over its prefix."""
    rng = np.random.default_rng(16)
    n = 1025 * BW[np.float32] + 7
    S = shuffled(random_structure("64 x (1025 BW + 7)", 64, n, 100000, rng), rng)
    exact_runs(S, np.float32, rng, [(CSR, "n", TAGS, dict(tiled=1, ncb=1026), {}), (CSR, "n", TWO, dict(tiled=1, ncb=1026), {})])


def repeated_structure(rng):
    S = random_structure("200 x 300 with repeats", 200, 300, 3000, rng)
    pick = rng.choice(S.nnz, 3, replace=False)
    rows = np.concatenate([S.rows] + [np.full(c - 1, S.rows[p]) for p, c in zip(pick, (2, 3, 64))])
    cols = np.concatenate([S.cols] + [np.full(c - 1, S.cols[p]) for p, c in zip(pick, (2, 3, 64))])
    return Structure(S.name, 200, 300, rows, cols)     # (the repeats come last inside their row and column)


def long_row_structure(count, dt, sorted_blocks, transposed):
    """4 x (BW + 50): row 1 holds `count` entries on 7 columns of the first block; not sorted_blocks: the row opens with
    an entry of the second block, so that its blocks decrease.  transposed: the same as a column of the input."""
    n = BW[dt] + 50
    cols = np.concatenate([[n - 1], np.tile([3, 9, 4, 40, 5, 17, 6], count // 7 + 1)[:count]])
    if sorted_blocks:
        cols = np.concatenate([cols[1:], cols[:1]])
    rows = np.concatenate([np.full(count + 1, 1), [0, 2, 2, 3]])
    cols = np.concatenate([cols, [5, 0, n - 2, 17]])
    name = "%d entries %s%s" % (count, "sorted" if sorted_blocks else "blocks decrease", " transposed" if transposed else "")
    return Structure(name, n, 4, cols, rows) if transposed else Structure(name, 4, n, rows, cols)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_repeated_entries_and_the_16_bit_row_count(dtype, monkeypatch):
    """Repeated entries add up.  A row of more than 65535 entries in one tile does not fit the planner's 16-bit counts:
    sell_count_kernel says so, the copy keeps the plain kernel (why = 5) and the product is exact; 65535 still counts."""
    monkeypatch.delenv("POGS_AMD_SELL_FORMAT", raising=False)
    monkeypatch.delenv("POGS_AMD_SPMV", raising=False)
    rng = np.random.default_rng(17)
    exact_runs(repeated_structure(rng), dtype, rng, all_paths(ONE_TILE))
    for count, why in ((65535, WHY_PADDING), (65536, WHY_COUNT), (70000, WHY_COUNT)):
        for sorted_blocks in (True, False):
            for transposed in (False, True):
                S = long_row_structure(count, dtype, sorted_blocks, transposed)
                long_trans = "t" if transposed else "n"                  # the product that runs on the long row's copy
                want = dict(tiled=0, why=why)
                # the long row is a row of the given copy (CSR of S, CSC of S^T) or of the one built on the device
                runs = [(o, long_trans, f, want, {}) for o in (CSR, CSC) for f in (0, TAGS, TWO)]
                # sq and x_nrm2 off (PARAMS 0 .. 3): |sum| <= 70000 x 16, exact in fp32
                seen = exact_runs(S, dtype, rng, runs[:4], start=0) + exact_runs(S, dtype, rng, runs[4:], start=2)
                assert len(seen) == 6
                other = "n" if transposed else "t"
                y, sumsq, info, infos = run(S, ints(rng, S.nnz, dtype), ints(rng, S.m if other == "t" else S.n, dtype),
                                            np.zeros(S.n if other == "t" else S.m, dtype), dtype, CSR, other, 0)
                assert info["why"] in (0, WHY_PADDING), (S.name, info)


# ---- real data ------------------------------------------------------------------------------------------------------

def sparse_scaled_normal(rng, S):
    """helpers.scaled_normal at the stored entries: standard normal times 2^-10 .. 2^10 per row and per column.  Beyond
    2^20 matrix entries the dense form is not made and the same law is drawn for the stored entries alone."""
    if S.m * S.n <= 1 << 20:
        return scaled_normal(rng, (S.m, S.n))[S.rows, S.cols]
    return rng.standard_normal(S.nnz) * np.exp2(rng.uniform(-10, 10, S.m))[S.rows] * np.exp2(rng.uniform(-10, 10, S.n))[S.cols]


def real_structures(dt, rng):
    bw, rr = BW[dt], RR[dt]
    out = [(S, {}) for S in small_structures(rng)]
    out += [(row_lengths_structure(rng), {}), (repeated_structure(rng), {}),
            (random_structure("3000 x 18433", 3000, 18433, 30000, rng), {}),
            (random_structure("2000 x 600000", 2000, 600000, 40000, rng), {}),
            (shuffled(random_structure("300 x (3 BW + 5)", 300, 3 * bw + 5, 6000, rng), rng), {}),
            (edge_column_structure(dt, 2 * bw + 1, rng), {}),
            (random_structure("(RR + 1) x (BW + 1)", rr + 1, bw + 1, 2 * rr, rng, every_row=True), dict(force_rr_rows=rr, force_ncg=2))]
    return out


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_real_data_within_the_derived_bar_and_same_bytes(dtype):
    """|y_i - ref_i| <= gamma_(L_i + ncb + ncg + 4) |alpha| (|A| |x|)_i on every path (alpha = 1 on CSR input, 0.7
    as the type holds it on CSC input, where x is scaled too); tags and two id slots give the same bytes (a row's
    elements stay together and in order in both layouts); a second run of every path gives the same bytes."""
    rng = np.random.default_rng(18)
    hi_dt = hi(np.zeros(1, dtype)).dtype
    for S, kw in real_structures(dtype, rng):
        val = sparse_scaled_normal(rng, S).astype(dtype)
        worst = 0.0
        for ord in (CSR, CSC):
            for trans in "nt":
                nin, nout = (S.n, S.m) if trans == "n" else (S.m, S.n)
                x = rng.standard_normal(nin).astype(dtype)
                x_nrm2 = 4.0 if ord == CSC else 0.0
                alpha = float(dtype(0.7)) if ord == CSC else 1.0
                ref, absref, L = product(S, val, hi(x) * hi_dt.type(0.5 if x_nrm2 else 1.0), trans, hi_dt)
                ref, absref = hi_dt.type(alpha) * ref, hi_dt.type(alpha) * absref
                got = {}
                for fmt in (TAGS, TWO, PLAIN):
                    k = kw if trans == "n" and fmt != PLAIN else {}
                    k = dict(k, x_nrm2=x_nrm2, alpha=alpha)
                    y, sumsq, info, _ = run(S, val, x, np.zeros(nout, dtype), dtype, ord, trans, fmt, **k)
                    y2, sumsq2, info2, _ = run(S, val, x, np.zeros(nout, dtype), dtype, ord, trans, fmt, **k)
                    assert same_bytes(y, y2) and sumsq == sumsq2 and info == info2, (S.name, ord, trans, fmt)
                    assert np.all(np.isfinite(y))
                    steps = L + info["ncb"] + info["ncg"] + 4
                    bar = (gamma(steps, dtype) + L * float(np.finfo(hi_dt).eps)) * absref
                    err = np.abs(hi(y) - ref)
                    assert np.all(err <= bar), (S.name, tname(dtype), ord, trans, fmt, int(np.argmax(err - bar)), info)
                    nz = bar > 0
                    worst = max(worst, float(np.max(err[nz] / bar[nz])) if nz.any() else 0.0)
                    s_ref = float(np.sum(hi(y) * hi(y)))
                    assert abs(sumsq - s_ref) <= gamma(nout + 2, np.float64) * s_ref, (S.name, sumsq, s_ref)
                    got[fmt] = (y, info)
                if got[TAGS][1]["tiled"] and got[TWO][1]["tiled"]:
                    assert got[TWO][1]["two"] == 1 and got[TAGS][1]["two"] == 0
                    assert same_bytes(got[TAGS][0], got[TWO][0]), (S.name, ord, trans)
        report("%-32s %s  max err / bar %.3f" % (S.name, tname(dtype), worst))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_refill_halves_the_product_exactly(dtype):
    """scale = 0.5 goes through scale_csr_kernel and the table of positions of the first fill: on integer data the product
    is exactly half of the scale = 1 product; an element the refill missed or misplaced keeps its old value."""
    rng = np.random.default_rng(19)
    bw = BW[dtype]
    for S in (row_lengths_structure(rng), repeated_structure(rng), random_structure("600 x 40000", 600, 40000, 6000, rng),
              shuffled(random_structure("300 x (3 BW + 5)", 300, 3 * bw + 5, 6000, rng), rng)):
        val = ints(rng, S.nnz, dtype)
        val[val == 0] = 3                   # every stored element matters
        for ord in (CSR, CSC):
            for trans in "nt":
                nin, nout = (S.n, S.m) if trans == "n" else (S.m, S.n)
                x = np.abs(ints(rng, nin, dtype)) + 1
                for fmt in (TAGS, TWO):
                    full = run(S, val, x, np.zeros(nout, dtype), dtype, ord, trans, fmt, scale=1.0)
                    half = run(S, val, x, np.zeros(nout, dtype), dtype, ord, trans, fmt, scale=0.5)
                    assert full[2]["tiled"] and half[2] == full[2], (S.name, full[2], half[2])
                    assert np.array_equal(half[0] * 2, full[0]) and half[1] * 4 == full[1], (S.name, ord, trans, fmt)


# ---- device transpose and scans -------------------------------------------------------------------------------------

def expected_transpose(S, ord, val):
    """the other CSR copy of the input: rows sorted by index, equal indices by the value's bit pattern as unsigned"""
    ptr, ind, v = S.arrays(ord, val)
    major = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    nseg = S.n if ord == CSR else S.m
    bits = v.view(np.uint32 if v.dtype == np.float32 else np.uint64)
    order = np.lexsort((bits, major, ind))
    t_ptr = np.zeros(nseg + 1, np.int32)
    t_ptr[1:] = np.cumsum(np.bincount(ind, minlength=nseg))
    return t_ptr, major[order].astype(np.int32), v[order]


def check_transpose(S, dt, rng, ord=CSR, val=None):
    val = (rng.standard_normal(S.nnz) if val is None else val).astype(dt)
    outs = []
    for _ in range(2):
        nin, nout = S.n, S.m
        out = run(S, val, np.ones(nin, dt), np.zeros(nout, dt), dt, ord, "n", TAGS, transpose=True)
        outs.append(out[4])
    want = expected_transpose(S, ord, val)
    for got, exp, what in zip(outs[0], want, ("ptr", "ind", "val")):
        assert np.array_equal(got, exp), (S.name, tname(dt), what)
    assert all(same_bytes(a, b) for a, b in zip(outs[0], outs[1])), S.name
    return outs[0]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_transpose_scan_sizes_and_segment_sorts(dtype):
    rng = np.random.default_rng(20)
    # the scan over the built copy's row counts: one kernel up to 4 x 8192 rows, three beyond
    for c1 in (1, 8191, 8192, 8193, 32768, 32769, 40961):
        S = random_structure("transpose c1 = %d" % c1, 50, c1, max(2 * c1, 40) if c1 > 1 else 30, rng)
        if c1 > 1:   # the last column is not empty: the scan's last entry and total differ
            S = Structure(S.name, 50, c1, np.append(S.rows, 7), np.append(S.cols, c1 - 1))
            S = Structure(S.name, 50, c1, *np.unique(np.stack([S.rows, S.cols]), axis=1))
        t_ptr, t_ind, t_val = check_transpose(S, dtype, rng)
        # scipy's transpose with sorted indices says the same (no repeated entries here)
        ptr, ind, v = S.arrays(CSR, np.arange(1, S.nnz + 1).astype(dtype))
        T = sp.csr_matrix((v, ind, ptr), shape=(S.m, S.n)).T.tocsr()
        T.sort_indices()
        assert np.array_equal(t_ptr, T.indptr) and np.array_equal(t_ind, T.indices)
    # segment lengths around the 256-thread passes, the 2048-element LDS sort and beyond it, none a power of two but those
    lengths = [1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4097, 5000]
    m = 5003
    rows = np.concatenate([np.sort(rng.choice(m, ln, replace=False)) for ln in lengths])
    cols = np.concatenate([np.full(ln, 2 * j + 1) for j, ln in enumerate(lengths)])
    S = Structure("segment lengths", m, 2 * len(lengths) + 1, rows, cols)
    check_transpose(S, dtype, rng)
    check_transpose(Structure("segment lengths as CSC", S.n, S.m, cols, rows), dtype, rng, ord=CSC)
    # repeated entries: ties in a segment ordered by the value's bits as unsigned (a negative value after a positive one)
    reps = np.concatenate([np.full(c, r) for r, c in ((5, 2), (9, 3), (700, 64), (4000, 300))])
    rows2 = np.concatenate([rows, reps, reps])
    cols2 = np.concatenate([cols, np.full(reps.size, 19), np.full(reps.size, 21)])      # the 4097 and 5000 segments
    S = Structure("segments with ties", m, S.n, rows2, cols2)
    val = rng.standard_normal(S.nnz)
    val[-5:] = [1.5, -1.5, 0.0, -0.0, 1.5]
    t_ptr, t_ind, t_val = check_transpose(S, dtype, rng, val=val)
    seg = slice(t_ptr[21], t_ptr[22])
    tied = t_val[seg][t_ind[seg] == 4000]
    assert tied.size in (300, 301) and np.any(tied < 0)
    first_neg = int(np.argmax(np.signbit(tied)))
    assert np.all(np.signbit(tied[first_neg:])) and not np.any(np.signbit(tied[:first_neg]))


# ---- no GPU needed --------------------------------------------------------------------------------------------------

def test_refusals_come_before_any_device_work():
    """NULL arrays, a bad dtype, ord, format, trans, sizes, ptr[0] and force values: POGS_ERROR with the reason, and no
    GPU is needed to say so."""
    ptr, ind = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32)
    val, x, y = np.ones(2, np.float32), np.ones(3, np.float32), np.zeros(2, np.float32)
    for kw, msg in ((dict(format=4), "unknown format"), (dict(format=-1), "unknown format"), (dict(num_cu=-1), "num_cu"),
                    (dict(trans="c"), "trans must be"),
                    (dict(force_rr_rows=500), "force_rr_rows"), (dict(force_rr_rows=576 + 32), "force_rr_rows"),
                    (dict(force_rr_rows=16384 + 64), "force_rr_rows"), (dict(force_ncg=2), "force_ncg"),
                    (dict(force_ncg=-1), "force_ncg")):
        with pytest.raises(RuntimeError, match=msg):
            _lib.spmv_check(ptr, ind, val, (2, 3), x, y, **kw)
    with pytest.raises(RuntimeError, match="force_rr_rows"):      # the fp64 limit is its own
        _lib.spmv_check(ptr, ind, val.astype(np.float64), (2, 3), x.astype(np.float64), y.astype(np.float64), force_rr_rows=6144 + 64)
    with pytest.raises(RuntimeError, match=r"ptr\[0\] must be 0"):
        _lib.spmv_check(np.array([1, 1, 2], np.int32), ind, val, (2, 3), x, y)
    with pytest.raises(RuntimeError, match="ptr must end"):
        _lib.spmv_check(np.array([0, 1, -2], np.int32), ind, val, (2, 3), x, y)
    with pytest.raises(RuntimeError, match="ptr must end"):      # no entries: no product to check
        _lib.spmv_check(np.zeros(3, np.int32), ind, val, (2, 3), x, y)
    with pytest.raises(RuntimeError, match="xlen / ylen"):
        _lib.spmv_check(ptr, ind, val, (2, 3), x[:2], y)
    with pytest.raises(RuntimeError, match="xlen / ylen"):
        _lib.spmv_check(ptr, ind, val, (2, 3), x, y, trans="t")
    lib = _lib.lib
    info, sumsq = np.zeros(16, np.int32), _lib.c_double(0.0)

    def call(dtype=0, ord=CSR, nrows=2, ncols=3, p=ptr, i=ind, v=val, xx=x, yy=y, ss=ctypes.byref(sumsq), inf=info):
        d = lambda a: None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else a)    # noqa: E731
        return lib.PogsAmdSpmvCheck(dtype, ord, nrows, ncols, d(p), d(i), d(v), 0, 0, 0, 0, 1.0, b"n", 0, 0.0, 1.0, 0.0,
                                    d(xx), 3, d(yy), 2, ss, d(inf), None, None, None)

    for kw in (dict(p=None), dict(i=None), dict(v=None), dict(xx=None), dict(yy=None), dict(ss=None), dict(inf=None)):
        assert call(**kw) != 0 and "null argument" in _lib.last_error(), kw
    assert call(dtype=2) != 0 and "unknown dtype" in _lib.last_error()
    assert call(ord=2) != 0 and "unknown ord" in _lib.last_error()
    assert call(nrows=0) != 0 and "nrows and ncols" in _lib.last_error()
    assert call(ncols=0) != 0 and "nrows and ncols" in _lib.last_error()
