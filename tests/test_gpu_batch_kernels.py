"""GPU tests of the batched, sparse-batched and many-problem kernels on their own (include/pogs_amd.h, Part 3:
PogsAmdBatchRowsCheck, PogsAmdBatchColsCheck, PogsAmdSpBatchSpmvCheck, PogsAmdManySetupCheck), against numpy
references formed in fp64 (long double for the fp64 bounds) from the dtype-cast inputs.

Three kinds of check:
  * exact integers: entries in [-4, 4], so every partial sum is an integer the mantissa holds and every order of
    summation gives the exact answer -- the kernel must equal the reference bit for bit, whatever the shape;
  * a precision bound on real-valued, badly scaled data: |y - y_ref| <= gamma_n (|M| |x|), gamma_n = n u / (1 - n u),
    which holds for any summation order (so it cannot flake) and fails if fp64 accumulates in fp32;
  * isolation: a problem's bytes are the same alone, in slot 15 of 16 and next to any number of other problems whose
    inputs are Inf / NaN / 1e30; the outputs of inactive problems and the padding come back untouched."""
import numpy as np
import pytest

import oracle_binding as ob
from helpers import _w_bars, gamma, hi, ints, relerr, same_bytes, scaled_normal, within_gamma
from pogs_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
FULL, LOWER, UPPER = 0, 1, 2
K = 16
SENTINEL = -7.375e-3      # what the outputs of inactive problems and the padding start as (and must stay)
NACTS = (1, 2, 3, 5, 8, 9, 16)


def vec(dt):
    return 16 // np.dtype(dt).itemsize


def rup(v, a):
    return (v + a - 1) // a * a


def slot_lists(rng, p):
    """act lists that hold problem p: alone (slot 0), slot 15 of 16, and every nact of NACTS at a random slot"""
    others = [q for q in range(K) if q != p]
    lists = [[p], others[:15] + [p]]
    for nact in NACTS:
        a = list(rng.choice(others, nact - 1, replace=False))
        a.insert(int(rng.integers(0, nact)), p)
        lists.append(a)
    return lists


def poison(rng, v, act, p, cols):
    """the other active vectors: +-Inf, NaN or 1e30 in their first `cols` entries; inactive ones all NaN"""
    v = v.copy()
    for q in range(K):
        if q == p:
            continue
        if q in act:
            v[q, :cols] = rng.choice([np.inf, -np.inf, np.nan, 1e30], cols)
        else:
            v[q] = np.nan
    return v


# ---- multi-vector row dots (launch_batch_rows) --------------------------------------------------------------------

def _rows_case(rng, dt, tri, rows, cols, data="int"):
    V = vec(dt)
    cp = rup(cols, V)
    ldm, ldx, ldy = cp + V, cp + 2 * V, rows + 3
    M = np.full((rows, ldm), np.nan, dt)
    X = np.zeros((K, ldx), dt)
    if data == "int":
        Mv, Xv = ints(rng, (rows, cols), dt), ints(rng, (K, cols), dt)
    else:
        Mv, Xv = scaled_normal(rng, (rows, cols)).astype(dt), rng.standard_normal((K, cols)).astype(dt)
    mask = np.ones((rows, cols), bool)
    if tri == LOWER:
        mask = np.tril(mask)
    elif tri == UPPER:
        mask = np.triu(mask)
    M[:, :cols] = np.where(mask, Mv, np.nan)     # outside the triangle and the padding: NaN, never to be used
    X[:, :cols] = Xv                            # X[:, cols:cp] = 0: the contract; beyond: unused
    X[:, cp:] = np.nan
    Mt = np.where(mask, Mv, 0)
    return M, X, np.full((K, ldy), SENTINEL, dt), Mt, Xv


def _check_untouched(Y, act, rows):
    inactive = [q for q in range(Y.shape[0]) if q not in act]
    assert np.all(Y[inactive] == np.asarray(SENTINEL, Y.dtype))
    assert np.all(Y[:, rows:] == np.asarray(SENTINEL, Y.dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_rows_exact_integer_parity_full(dtype):
    rng = np.random.default_rng(1)
    V = vec(dtype)
    S = 4 * V
    cols_list = sorted({c for c in (1, V - 1, V + 1, S - 1, S + 1, 4 * S - 1, 4 * S + 1, 61, 1000) if c >= 1})
    for rows in (1, 15, 16, 17, 63, 64, 65, 1037, 4099):
        for cols in cols_list:
            M, X, Y0, Mt, Xv = _rows_case(rng, dtype, FULL, rows, cols)
            act = list(rng.permutation(K)[:11])
            Y = _lib.batch_rows_check(FULL, M, cols, X, Y0, act)
            ref = Mt.astype(np.float64) @ Xv.astype(np.float64).T
            assert np.array_equal(Y[act, :rows], ref.T[act].astype(dtype)), (rows, cols)
            _check_untouched(Y, act, rows)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tri", [LOWER, UPPER])
def test_batch_rows_exact_integer_parity_triangles(dtype, tri):
    """The factor passes of the batched solve: only the triangle is read (NaN outside it must not matter)."""
    rng = np.random.default_rng(2 + tri)
    for k in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130, 257):
        M, X, Y0, Mt, Xv = _rows_case(rng, dtype, tri, k, k)
        act = list(range(K))
        Y = _lib.batch_rows_check(tri, M, k, X, Y0, act)
        ref = Mt.astype(np.float64) @ Xv.astype(np.float64).T
        assert np.array_equal(Y[:, :k], ref.T.astype(dtype)), k
        _check_untouched(Y, act, k)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tri", [FULL, LOWER, UPPER])
def test_batch_rows_precision_bound(dtype, tri):
    rng = np.random.default_rng(7 + tri)
    for rows, cols in ((1037, 1000), (65, 61), (257, 257)):
        if tri != FULL and rows != cols:
            continue
        M, X, Y0, Mt, Xv = _rows_case(rng, dtype, tri, rows, cols, data="real")
        act = list(range(K))
        Y = _lib.batch_rows_check(tri, M, cols, X, Y0, act)
        ref = hi(Mt) @ hi(Xv).T
        absref = np.abs(hi(Mt)) @ np.abs(hi(Xv)).T
        within_gamma(Y[:, :rows], ref.T, absref.T, cols, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tri", [FULL, LOWER, UPPER])
def test_batch_rows_isolation(dtype, tri):
    rng = np.random.default_rng(11 + tri)
    rows = cols = 129
    M, X, Y0, Mt, Xv = _rows_case(rng, dtype, tri, rows, cols, data="real")
    p = 6
    first = None
    for act in slot_lists(rng, p):
        Y = _lib.batch_rows_check(tri, M, cols, poison(rng, X, act, p, cols), Y0, act)
        _check_untouched(Y, act, rows)
        if first is None:
            first = Y[p].copy()
            ref = hi(Mt) @ hi(Xv[p])
            within_gamma(first[:rows], ref, np.abs(hi(Mt)) @ np.abs(hi(Xv[p])), cols, dtype)
        assert same_bytes(Y[p], first), act


# ---- multi-vector column sums (launch_batch_cols + launch_batch_cols_reduce) ---------------------------------------

def _cols_case(rng, dt, rows, cols, data="int", add=False):
    V = vec(dt)
    cp = rup(cols, V)
    ldm, ldu, ldz = cp + V, rows + 5, cp + 3
    M = np.full((rows, ldm), np.nan, dt)
    U = np.full((K, ldu), np.nan, dt)
    if data == "int":
        Mv, Uv = ints(rng, (rows, cols), dt), ints(rng, (K, rows), dt)
    else:
        Mv, Uv = scaled_normal(rng, (rows, cols)).astype(dt), rng.standard_normal((K, rows)).astype(dt)
    M[:, :cols] = Mv                            # M[:, cols:] NaN: columns >= cols come back 0 whatever M holds
    U[:, :rows] = Uv
    A = None
    if add:
        A = np.full((K, ldz), np.nan, dt)
        A[:, :cp] = ints(rng, (K, cp), dt) if data == "int" else rng.standard_normal((K, cp)).astype(dt)
    return M, U, np.full((K, ldz), SENTINEL, dt), A, Mv, Uv


def _check_cols_out(Z, act, cols, cp):
    inactive = [q for q in range(K) if q not in act]
    assert np.all(Z[inactive] == np.asarray(SENTINEL, Z.dtype))
    assert np.all(Z[act, cols:cp] == 0) and not np.any(np.signbit(Z[act, cols:cp]))
    assert np.all(Z[:, cp:] == np.asarray(SENTINEL, Z.dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_cols_exact_integer_parity(dtype):
    rng = np.random.default_rng(21)
    V = vec(dtype)
    slab = 16 * V
    big = (8192, 5000) if dtype == np.float32 else (4096, 3000)
    shapes = [(r, c) for r in (1, 17, 64, 129, 1037) for c in (1, slab - 1, slab, slab + 1, 2 * slab + 3)] + [big]
    parts = set()
    for rows, cols in shapes:
        cp = rup(cols, V)
        for add in (False, True):
            if (rows, cols) == big and add:
                continue
            M, U, Z0, A, Mv, Uv = _cols_case(rng, dtype, rows, cols, add=add)
            act = list(rng.permutation(K)[:13])
            Z, nrb, rpb = _lib.batch_cols_check(M, cols, U, Z0, act, add=A)
            parts.add((rows, nrb, rpb))
            ref = (Uv.astype(np.float64) @ Mv.astype(np.float64))
            if add:
                ref = ref + A[:, :cols]
            assert np.array_equal(Z[act, :cols], ref[act].astype(dtype)), (rows, cols, add)
            _check_cols_out(Z, act, cols, cp)
    # the partitions the cases covered (reported by the entry, not assumed)
    assert any(nrb == 1 for _, nrb, _ in parts)
    assert any(nrb > 1 and rpb % 64 != 0 and rpb < 64 for _, nrb, rpb in parts), parts        # e.g. m = 129: 48
    assert any(nrb > 1 and rpb > 64 and rpb % 64 != 0 for _, nrb, rpb in parts), parts        # partial last step
    assert any(r % rpb != 0 for r, nrb, rpb in parts if nrb > 1)                                  # short last block


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_cols_precision_bound(dtype):
    rng = np.random.default_rng(23)
    for rows, cols in ((1037, 129), (4096, 61)):
        for add in (False, True):
            M, U, Z0, A, Mv, Uv = _cols_case(rng, dtype, rows, cols, data="real", add=add)
            act = list(range(K))
            Z, _, _ = _lib.batch_cols_check(M, cols, U, Z0, act, add=A)
            ref = hi(Uv) @ hi(Mv)
            absref = np.abs(hi(Uv)) @ np.abs(hi(Mv))
            n = rows
            if add:
                ref = ref + hi(A[:, :cols])
                absref = absref + np.abs(hi(A[:, :cols]))
                n += 1
            within_gamma(Z[:, :cols], ref, absref, n, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_cols_isolation(dtype):
    rng = np.random.default_rng(29)
    rows, cols = 1037, 77
    M, U, Z0, A, Mv, Uv = _cols_case(rng, dtype, rows, cols, data="real", add=True)
    p = 9
    first = None
    for act in slot_lists(rng, p):
        Ap = poison(rng, A, act, p, rup(cols, vec(dtype)))
        Z, _, _ = _lib.batch_cols_check(M, cols, poison(rng, U, act, p, rows), Z0, act, add=Ap)
        _check_cols_out(Z, act, cols, rup(cols, vec(dtype)))
        if first is None:
            first = Z[p].copy()
        assert same_bytes(Z[p], first), act


# ---- multi-vector CSR product (sp_batch_geometry + launch_sp_batch_pack + launch_sp_batch_spmv) --------------------

class Csr:
    """A random CSR of nrows x ncols with the given row lengths (duplicate columns within a row allowed, and likely)
    and its products formed in `prec` (float64: exact for the integer data; long double for fp64 bounds)."""

    def __init__(self, rng, nrows, ncols, lengths, dt, data="int"):
        lengths = np.asarray(lengths, np.int64)
        ptr = np.zeros(nrows + 1, np.int64)
        ptr[1:] = np.cumsum(lengths)
        nnz = int(ptr[-1])
        self.ptr, self.ind = ptr.astype(np.int32), rng.integers(0, ncols, nnz).astype(np.int32)
        self.val = ints(rng, nnz, dt) if data == "int" else \
            (rng.standard_normal(nnz) * np.exp2(rng.uniform(-10, 10, nnz))).astype(dt)
        self.rows, self.nrows, self.ncols = np.repeat(np.arange(nrows), lengths), nrows, ncols
        self.maxlen = int(lengths.max()) if nrows else 0

    def args(self):
        return self.ptr, self.ind, self.val, self.ncols

    def mul(self, X, absolute=False):
        """(|CSR|) (|X|)^T rows: X is (k, >= ncols); returns (k, nrows) in the reference precision"""
        Xh = hi(X[:, :self.ncols])
        v = hi(self.val)
        if absolute:
            Xh, v = np.abs(Xh), np.abs(v)
        out = np.zeros((Xh.shape[0], self.nrows), Xh.dtype)
        for q in range(Xh.shape[0]):
            np.add.at(out[q], self.rows, v * Xh[q, self.ind])
        return out


def _sp_vectors(rng, dt, nrows, ncols, data="int"):
    ldx, ldy = ncols + 3, nrows + 2
    X = np.full((K, ldx), np.nan, dt)
    X[:, :ncols] = ints(rng, (K, ncols), dt) if data == "int" else rng.standard_normal((K, ncols)).astype(dt)
    return X, np.full((K, ldy), SENTINEL, dt)


def _sp_untouched(Y, part, act, nrows):
    inactive = [q for q in range(K) if q not in act]
    assert np.all(Y[inactive] == np.asarray(SENTINEL, Y.dtype))
    assert np.all(Y[:, nrows:] == np.asarray(SENTINEL, Y.dtype))
    if part is not None:
        assert np.all(part[inactive] == SENTINEL)


def _sp_cases(rng):
    """(name, nrows, ncols, row lengths, num_cu)"""
    out = [("mean 10", 700, 1001, rng.integers(0, 21, 700), 0),
           ("mean 100", 300, 1001, rng.integers(60, 141, 300), 0),
           ("mean 300", 200, 3001, rng.integers(200, 401, 200), 0),
           ("empty rows", 500, 257, rng.integers(0, 3, 500) * rng.integers(0, 2, 500), 0),
           ("all empty", 50, 33, np.zeros(50, int), 0),
           ("nrows 1", 1, 97, [40], 0),
           ("nrows 1 long", 1, 5003, [3000], 0)]
    long_row = rng.integers(1, 9, 400)
    long_row[123] = 2500                                         # > U * L for every kp
    out.append(("one long row", 400, 2003, long_row, 0))
    out.append(("rpw > G", 5000, 999, rng.integers(0, 7, 5000), 1))
    out.append(("rpw 2048", 70001, 1001, rng.integers(0, 7, 70001), 1))
    out.append(("rpw 2048 wide", 70001, 1001, rng.integers(100, 160, 70001) * (rng.random(70001) < 0.02), 1))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_sp_batch_spmv_exact_integer_parity(dtype):
    rng = np.random.default_rng(31)
    seen = []
    for name, nrows, ncols, lengths, num_cu in _sp_cases(rng):
        A = Csr(rng, nrows, ncols, lengths, dtype)
        X, Y0 = _sp_vectors(rng, dtype, nrows, ncols)
        prod = A.mul(X.astype(np.float64))
        for nact, beta in ((16, 0.0), (5, -2.0), (1, 0.5)):
            act = list(rng.permutation(K)[:nact])
            yin = None
            ref = prod
            if beta:
                yin = np.full((K, nrows + 7), np.nan, dtype)
                yin[:, :nrows] = ints(rng, (K, nrows), dtype)
                ref = ref + beta * yin[:, :nrows].astype(np.float64)
            Y, part, geom = _lib.sp_batch_spmv_check(*A.args(), X, Y0, act, beta=beta, yin=yin, part_fill=SENTINEL,
                                                     num_cu=num_cu)
            assert np.array_equal(Y[act, :nrows], ref[act].astype(dtype)), (name, nact)
            _sp_untouched(Y, part, act, nrows)
            # the records: exact here too (integer squares, sums below 2^53)
            y64 = Y[act, :nrows].astype(np.float64)
            assert np.array_equal(part[act].sum(axis=1), (y64 * y64).sum(axis=1)), name
            seen.append((nrows, geom))
    # coverage, from the reported geometry
    assert {g[0] for _, g in seen} == {4, 5, 6}
    G = lambda lshift: 4 * (64 >> lshift)   # noqa: E731  (row groups per workgroup)
    assert any(g[1] > G(g[0]) for _, g in seen)
    assert any(g[1] == 2048 and n % 2048 != 0 and g[2] > 1 for n, g in seen)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sp_batch_spmv_precision_bound_and_records(dtype):
    rng = np.random.default_rng(37)
    for name, nrows, ncols, lengths, num_cu in _sp_cases(rng)[:4] + _sp_cases(rng)[7:9]:
        A = Csr(rng, nrows, ncols, lengths, dtype, data="real")
        X, Y0 = _sp_vectors(rng, dtype, nrows, ncols, data="real")
        yin = rng.standard_normal((K, nrows)).astype(dtype)
        beta = 0.75
        act = list(range(K))
        Y, part, geom = _lib.sp_batch_spmv_check(*A.args(), X, Y0, act, beta=beta, yin=yin, part_fill=SENTINEL,
                                                 num_cu=num_cu)
        ref = A.mul(X) + beta * hi(yin)
        absref = A.mul(X, absolute=True) + abs(beta) * np.abs(hi(yin))
        n = A.maxlen + 2                                          # terms of the longest row, + beta yin
        within_gamma(Y[:, :nrows], ref, absref, n, dtype)
        # the records: squares of the stored values, summed in fp64 over the rows of a workgroup, then here
        y2 = np.asarray(Y[:, :nrows], np.longdouble) ** 2
        tot = y2.sum(axis=1)
        err = np.abs(np.asarray(part.sum(axis=1), np.longdouble) - tot)
        assert np.all(err <= gamma(nrows + geom[2], np.float64) * tot), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_sp_batch_spmv_isolation_every_kp(dtype):
    """nact 1, 2, 3, 5, 8, 9, 16: every KP template (1, 2, 4, 8, 16) of the product, the reduce-scatter included."""
    rng = np.random.default_rng(41)
    for name, nrows, ncols, lengths, num_cu in (_sp_cases(rng)[i] for i in (0, 1, 2, 7)):
        A = Csr(rng, nrows, ncols, lengths, dtype, data="real")
        X, Y0 = _sp_vectors(rng, dtype, nrows, ncols, data="real")
        p = 4
        first = None
        for act in slot_lists(rng, p):
            Y, part, _ = _lib.sp_batch_spmv_check(*A.args(), poison(rng, X, act, p, ncols), Y0, act,
                                                  part_fill=SENTINEL, num_cu=num_cu)
            _sp_untouched(Y, part, act, nrows)
            if first is None:
                first = (Y[p].copy(), part[p].copy())
                within_gamma(Y[p, :nrows], A.mul(X[p:p + 1])[0], A.mul(X[p:p + 1], absolute=True)[0], A.maxlen,
                             dtype)
            assert same_bytes(Y[p], first[0]) and same_bytes(part[p], first[1]), (name, act)


# ---- many-problem setup (copy, Sinkhorn-Knopp, scale, norm estimate, Gram, Cholesky, W = L^-1) ---------------------

MANY_SHAPES = [(70, 33), (37, 101), (200, 1), (1, 30), (130, 65), (150, 63), (64, 90), (65, 300), (300, 129)]


def _many_check(dt, m, n, A):
    out = _lib.many_setup_check(A)
    K = min(m, n)
    for j in range(A.shape[0]):
        A_o, d_o, e_o, nrm_o, _ = ob.oracle_equil(A[j], dtype=dt)
        tol = 1e-10 if dt == np.float64 else 3e-5
        assert relerr(out["d"][j], d_o) < tol, (m, n)
        assert relerr(out["e"][j], e_o) < tol, (m, n)
        assert relerr(out["A_eq"][j], A_o) < tol, (m, n)
        assert out["nrmA"][j] == pytest.approx(nrm_o, rel=2e-3)
        sig = np.linalg.norm(A_o.astype(np.float64), 2)
        assert sig * 0.9 <= out["nrmA"][j] <= sig * 1.001
        # W against fp64 from the path's own A_eq: the factor apart from the equilibration
        Ae = out["A_eq"][j].astype(np.float64)
        H = np.eye(K) + (Ae.T @ Ae if m > n else Ae @ Ae.T)
        W_ref = np.linalg.inv(np.linalg.cholesky(H))
        W = np.tril(out["W"][j].astype(np.float64))
        res_bar, w_bar = _w_bars(m, n, dt)
        res = np.max(np.abs(W @ H @ W.T - np.eye(K)))
        assert res <= res_bar, (m, n, res, res_bar)
        assert np.max(np.abs(W - np.tril(W_ref))) <= w_bar, (m, n)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_many_setup_against_oracle_and_fp64_factor(dtype):
    rng = np.random.default_rng(43)
    for m, n in MANY_SHAPES:
        A = rng.standard_normal((2, m, n)) * rng.uniform(0.1, 10.0, (2, m, 1)) * rng.uniform(0.1, 10.0, (2, 1, n))
        _many_check(dtype, m, n, A.astype(dtype))


def test_many_setup_envelope_edge_fp32():
    rng = np.random.default_rng(47)
    m, n = 16384, 512
    A = (rng.standard_normal((1, m, n)) * rng.uniform(0.5, 2.0, (1, m, 1))).astype(np.float32)
    _many_check(np.float32, m, n, A)


@pytest.mark.parametrize("dtype", DTYPES)
def test_many_setup_bytes_alone_and_at_position_20_of_37(dtype):
    rng = np.random.default_rng(53)
    for m, n in ((70, 33), (37, 101)):
        A = (rng.standard_normal((37, m, n)) * rng.uniform(0.1, 10.0, (37, m, 1))).astype(dtype)
        alone = _lib.many_setup_check(A[20:21])
        col = _lib.many_setup_check(A[20:21], ord=_lib.COL_MAJ)
        full = _lib.many_setup_check(A)
        for key in ("A_eq", "d", "e", "nrmA", "W"):
            assert same_bytes(alone[key][0], full[key][20]), key
            assert same_bytes(alone[key][0], col[key][0]), key


# ---- refusals, then a valid call -----------------------------------------------------------------------------------

def test_refusals_leave_the_entries_working():
    rng = np.random.default_rng(59)
    dt = np.float32
    M, X, Y0, Mt, Xv = _rows_case(rng, dt, FULL, 33, 33)
    with pytest.raises(RuntimeError, match="act entry repeats"):
        _lib.batch_rows_check(FULL, M, 33, X, Y0, [1, 1])
    Y = _lib.batch_rows_check(FULL, M, 33, X, Y0, [3])
    assert np.array_equal(Y[3, :33], (Mt.astype(np.float64) @ Xv[3].astype(np.float64)).astype(dt))
    A = Csr(rng, 40, 50, rng.integers(1, 9, 40), dt)
    Xs, Ys = _sp_vectors(rng, dt, 40, 50)
    bad = A.ptr.copy()
    bad[6] = bad[5] - 1
    with pytest.raises(RuntimeError, match="must not decrease"):
        _lib.sp_batch_spmv_check(bad, A.ind, A.val, 50, Xs, Ys, [0])
    Y, _, _ = _lib.sp_batch_spmv_check(*A.args(), Xs, Ys, [2])
    assert np.array_equal(Y[2, :40], A.mul(Xs[2:3].astype(np.float64))[0].astype(dt))
    with pytest.raises(RuntimeError, match="POGS_AMD_MANY_MAX_DIM_MAX"):
        _lib.many_setup_check(np.ones((1, 16385, 1), dt))
    out = _lib.many_setup_check(rng.standard_normal((1, 20, 10)).astype(dt))
    assert np.all(np.isfinite(out["W"]))
