"""GPU tests of the sparse solver's direct projector (Solver(sparse A, projector=PROJ_DIRECT); csrc/sparse_direct.h,
csrc/sparse.hip, csrc/sparse_batch.h): the sparse Gram kernel and the solo triangular mat-vec on their own
(PogsAmdSparseGramCheck, PogsAmdTriMatvecCheck), the factor a handle holds, its projection, solo and batched solves.

The reference trajectory of a direct sparse handle is the oracle's DENSE direct solve on A.toarray(): the sparse and the
dense equilibration are the same arithmetic (same iteration counts and norm estimates on the CPU oracle), and the
direct projector is ProjectorDirect (projector_direct_dense.cpp:87-135) whatever the storage of A.

Bars.
  Gram, exact: small integers -- every product and every sum is exact in double, so the result is the integer matrix.
  Gram, real:  |G - G_hi| <= u_T |G_hi| + gamma_c(double) |S|^T |S|, c the longest sum (the rows of S): the products of
               two floats are exact in double (two doubles: one fma rounding per term), the sum of c terms in double
               in any order is within gamma_c, and the result is rounded to T once.  G_hi: helpers.xmatmul (long
               double); its own error (about c 2^-76) and the second-order term go into a factor 1 + 1e-6 on the bar.
  mat-vec:     gamma_n in T against the sum formed beyond T: a row of L <= n terms is split over c lanes with at most e
               terms each (L >= c + e - 1), every term passes the lane's chain (<= e roundings, fma) and the levels of
               the tree at which its partner is not zero (<= ceil(log2 c) <= c - 1): <= L <= n roundings.
  factor:      the rule and the bars of test_gpu_factor_kernels._handle_check.
  projection:  4 x the error of the oracle's direct projection in the same type, against the long double solution.
  solves:      the slacks of tests/test_gpu_sparse.py (iterations within 1 / 3, x to 1e-6 / 1e-4, optval 1e-6 / 2e-4).

Measured ratios: profiles/sparse_direct_throughput.txt (the tests print them: pytest -s)."""
import ctypes
import os

import numpy as np
import pytest
import scipy.linalg as sla

import oracle_binding as ob
from helpers import PROBLEMS, gamma, hi, relerr, same_bytes, soa, within_gamma, xmatmul
from pogs_amd import _lib

sp = pytest.importorskip("scipy.sparse")

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
SENTINEL = -7.375e-3
DIRECT = _lib.PROJ_DIRECT


def _pogs():
    import pogs_amd

    return pogs_amd


def vec(dt):
    return 16 // np.dtype(dt).itemsize


def rup(v, a):
    return (v + a - 1) // a * a


def tname(dt):
    return "fp32" if dt == np.float32 else "fp64"


def report(line):
    print("sparse_direct: " + line)


# ---- the Gram kernel -----------------------------------------------------------------------------------------------

def _gram_rows(m, n, seed, values):
    """Raw CSR arrays (ptr, ind, val as float64) of an m x n matrix that scipy would canonicalise away: indices in
    random order, empty rows (1 and m - 2), an empty column (n - 2; none for n < 3), one full column (every stored
    row holds column min(2, n - 1)), one full row (3, or 2 where 3 is empty: every column but the empty one), the same
    column three times in a row (row 4, its first three entries) and a row of 70 entries (row 0) whose entry 67 repeats
    the column of entry 3, so the repeat falls into the second chunk of 64."""
    rng = np.random.default_rng(seed)
    c_full = min(2, n - 1)
    allowed = np.array([c for c in range(n) if n < 3 or c != n - 2])
    empty = {1, m - 2} if m >= 5 else set()
    full_row = 2 if m - 2 == 3 else 3
    ptr, ind = [0], []
    for i in range(m):
        if i in empty:
            cols = []
        elif i == 0:
            if len(allowed) >= 70:
                cols = list(rng.permutation(allowed)[:70])
            else:
                cols = [allowed[(7 * k) % len(allowed)] for k in range(70)]
            cols[67] = cols[3]
        elif i == full_row:
            cols = list(rng.permutation(allowed))
        else:
            k = int(rng.integers(1, min(len(allowed), 6) + 1))
            cols = list(rng.choice(allowed, size=k, replace=False))
            if c_full not in cols:
                cols.append(c_full)
            rng.shuffle(cols)
            if i == 4:
                cols = [cols[0]] * 3 + cols[1:]
        ind += [int(c) for c in cols]
        ptr.append(len(ind))
    return np.array(ptr, np.int32), np.array(ind, np.int32), values(rng, len(ind))


def _dense_of(ptr, ind, val, rows, cols):
    S = np.zeros((rows, cols), val.dtype)
    r = np.repeat(np.arange(rows), np.diff(ptr))
    np.add.at(S, (r, ind), val)
    return S


def _gram_input(shape, order, seed, values):
    """(ptr, ind, val, ord, S): the arrays of `_gram_rows` as the CSR of A (order "csr") or, built for A^T, as the CSC
    of A; S: the dense matrix with repeated entries added up."""
    m, n = shape
    if order == "csr":
        ptr, ind, val = _gram_rows(m, n, seed, values)
        return ptr, ind, val, _lib.ROW_MAJ, _dense_of(ptr, ind, val, m, n)
    ptr, ind, val = _gram_rows(n, m, seed, values)
    return ptr, ind, val, _lib.COL_MAJ, _dense_of(ptr, ind, val, n, m).T.copy()


def _int_values(rng, count):
    return rng.integers(-3, 4, count).astype(np.float64)


GRAM_SHAPES = [(37, 5), (5, 37), (300, 130), (130, 300), (9, 1), (1, 9)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ["csr", "csc"])
@pytest.mark.parametrize("shape", GRAM_SHAPES)
def test_gram_of_small_integers_is_exact_and_the_same_bytes_every_run(shape, order, dtype):
    m, n = shape
    K = min(m, n)
    ptr, ind, val, ord_, S = _gram_input(shape, order, 1000 * m + n, _int_values)
    want = (S.T @ S if m > n else S @ S.T).astype(dtype)
    ldg = K + 3
    G0 = np.full((K, ldg), SENTINEL, dtype)
    runs = [_lib.sparse_gram_check(ptr, ind, val.astype(dtype), shape, G0, ord=ord_, window=64, num_cu=256)
            for _ in range(3)]
    G, info = runs[0]
    assert (info["K"], info["tall"], info["window"], info["windows"]) == (K, int(m > n), 64, -(-K // 64))
    assert info["ld"] == rup(K, vec(dtype))
    lower = np.tril(np.ones((K, K), bool))
    assert same_bytes(G[:, :K][lower], want[lower])
    # the strict upper triangle and the columns beyond K come back as given
    assert np.all(G[:, :K][~lower] == dtype(SENTINEL)) and np.all(G[:, K:] == dtype(SENTINEL))
    assert all(same_bytes(G, r[0]) for r in runs[1:])
    auto, info0 = _lib.sparse_gram_check(ptr, ind, val.astype(dtype), shape, G0, ord=ord_, window=0, num_cu=256)
    assert same_bytes(auto, G) and info0["window"] == min(1024, rup(K, 64))
    other, _ = _lib.sparse_gram_check(ptr, ind, val.astype(dtype), shape, G0, ord=ord_, window=128, num_cu=7)
    assert same_bytes(other, G)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(300, 130), (130, 300)])
def test_gram_of_real_data_is_a_double_sum_rounded_once(shape, dtype):
    m, n = shape
    K, c = min(m, n), max(m, n)
    rng = np.random.default_rng(5 * m + n)
    A = sp.random(m, n, 0.3, random_state=rng, format="csr",
                  data_rvs=lambda k: rng.standard_normal(k) * np.exp2(rng.uniform(-8, 8, k)))
    A = A.astype(dtype)
    A.sort_indices()
    S = A.toarray().astype(np.float64)
    S = S if m > n else S.T
    G_hi = xmatmul(S.T, S)
    absG = np.abs(S).T @ np.abs(S)
    u = np.finfo(dtype).eps / 2
    bar = (u * np.abs(G_hi) + gamma(c, np.float64) * absG) * (1 + 1e-6)
    G, _ = _lib.sparse_gram_check(A.indptr, A.indices, A.data, shape, np.zeros((K, K), dtype), window=64)
    lower = np.tril(np.ones((K, K), bool))
    err = np.abs(G.astype(np.longdouble) - G_hi)
    ratio = float(np.max((err / np.where(bar > 0, bar, 1))[lower]))
    report("gram real %s %d x %d  max err / bar %.3f" % (tname(dtype), m, n, ratio))
    assert np.all(np.isfinite(G[lower])) and np.all(err[lower] <= bar[lower])


# ---- the solo triangular mat-vec ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tri", [_lib.TRI_LOWER, _lib.TRI_UPPER])
@pytest.mark.parametrize("n", [1, 3, 64, 65, 130, 517])
def test_triangular_matvec_reads_the_triangle_only(n, tri, dtype):
    rng = np.random.default_rng(10 * n + tri)
    ld = rup(n, vec(dtype)) + vec(dtype)
    inside = np.tril(np.ones((n, n), bool)) if tri == _lib.TRI_LOWER else np.triu(np.ones((n, n), bool))
    M = np.full((n, ld), np.nan, dtype)
    M[:, :n][inside] = rng.standard_normal(int(inside.sum())).astype(dtype)
    x = rng.standard_normal(n).astype(dtype)
    T = np.where(inside, M[:, :n], 0).astype(dtype)
    ref = hi(T) @ hi(x)
    absref = np.abs(hi(T)) @ np.abs(hi(x))
    y = _lib.tri_matvec_check(tri, M, x, np.full(n, np.nan, dtype))
    within_gamma(y, ref, absref, n, dtype)
    # the batched row pass with one slot: the same product by another kernel, within the same bar
    X = np.zeros((1, ld), dtype)
    X[0, :n] = x
    yb = _lib.batch_rows_check(tri, M, n, X, np.full((1, n), np.nan, dtype), [0])[0]
    within_gamma(yb, ref, absref, n, dtype)
    assert np.all(np.abs(hi(y) - hi(yb)) <= 2 * gamma(n, dtype) * absref)


# ---- handles ---------------------------------------------------------------------------------------------------------

def _raw_solver(shape, data, ptr, ind, dtype, order=None, projector=DIRECT, mem=None):
    """A Solver around a handle built through PogsAmdCreateSparse from the arrays as given (no sum, no sort); order:
    ROW_MAJ (CSR, default) / COL_MAJ (CSC)."""
    pogs = _pogs()
    order = _lib.ROW_MAJ if order is None else order
    data = np.ascontiguousarray(data, dtype)
    ptr, ind = np.ascontiguousarray(ptr, np.int32), np.ascontiguousarray(ind, np.int32)
    h = ctypes.c_void_p()
    code = _lib.F64 if dtype == np.float64 else _lib.F32
    opt = _lib.PogsAmdOptions(device=-1, projector=projector, profile=0)
    rc = _lib.lib.PogsAmdCreateSparse(ctypes.byref(h), code, order, shape[0], shape[1], len(data), data.ctypes.data,
                                      ptr.ctypes.data, ind.ctypes.data, _lib.HOST, ctypes.byref(opt), None)
    assert rc == 0, _lib.last_error()
    s = object.__new__(pogs.Solver)
    s._h, s.dtype, s.sparse, s._m_global = h, np.dtype(dtype).type, True, None
    s.m, s.n = shape
    return s


def _a_eq(s, A):
    """the equilibrated matrix of a sparse handle built from the CSR A (values in the order of the input)"""
    buf = np.zeros(A.nnz, s.dtype)
    assert _lib.lib.PogsAmdGetEquil(s._h, buf.ctypes.data_as(ctypes.c_void_p), None, None, None) == 0
    return sp.csr_matrix((buf, A.indices, A.indptr), shape=A.shape)


_handles = {}


def _handle_case(shape, dtype):
    """(A_eq dense, W, U, x0, y0, x, y) of a direct handle on a random CSR of density 0.02, made once per module"""
    key = (shape, np.dtype(dtype).name)
    if key not in _handles:
        m, n = shape
        A = sp.random(m, n, 0.02, random_state=np.random.default_rng(m + 7 * n), format="csr", dtype=np.float64)
        A.sort_indices()
        rng = np.random.default_rng(m * n)
        x0, y0 = rng.standard_normal(n).astype(dtype), rng.standard_normal(m).astype(dtype)
        with _pogs().Solver(A, dtype=dtype, projector=DIRECT) as s:
            A_eq = _a_eq(s, sp.csr_matrix(A, dtype=dtype)).toarray()
            W, U = s.factor()
            x, y = s.project(x0, y0, tol=0.5)    # (tol is not used)
            st = s.stats()
        assert st["gram_ms"] > 0 and st["chol_ms"] > 0 and st["trtri_ms"] > 0
        _handles[key] = (A_eq, W, U, x0, y0, x, y)
    return _handles[key]


HANDLE_SHAPES = [(3000, 400), (400, 3000)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", HANDLE_SHAPES)
def test_the_factor_of_a_direct_sparse_handle(shape, dtype):
    from test_gpu_factor_kernels import _handle_check

    A_eq, W, U = _handle_case(shape, dtype)[:3]
    assert A_eq.dtype == dtype and same_bytes(U, W.T.copy())
    _handle_check(dtype, A_eq, [W], "sparse direct %d x %d" % shape)


def _ld_solve(H_ld, rhs_ld):
    """H x = rhs for a small SPD H beyond fp64: an fp64 Cholesky solve refined with long double residuals"""
    c = sla.cho_factor(H_ld.astype(np.float64))
    x = np.zeros_like(rhs_ld)
    for _ in range(4):
        r = rhs_ld - H_ld @ x
        x = x + sla.cho_solve(c, r.astype(np.float64))
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", HANDLE_SHAPES)
def test_projection_of_a_direct_sparse_handle(shape, dtype):
    m, n = shape
    A_eq, _, _, x0, y0, x, y = _handle_case(shape, dtype)
    A_ld, x0_ld, y0_ld = A_eq.astype(np.longdouble), x0.astype(np.longdouble), y0.astype(np.longdouble)
    A64 = A_eq.astype(np.float64)
    if m > n:
        H = np.eye(n, dtype=np.longdouble) + xmatmul(A64.T, A64)
        x_ref = _ld_solve(H, x0_ld + A_ld.T @ y0_ld)
        y_ref = A_ld @ x_ref
    else:
        H = np.eye(m, dtype=np.longdouble) + xmatmul(A64, A64.T)
        t = _ld_solve(H, A_ld @ x0_ld - y0_ld)
        x_ref, y_ref = x0_ld - A_ld.T @ t, y0_ld + t
    xo, yo = ob.oracle_project(A_eq, x0, y0, use_cgls=False, dtype=dtype)

    def err(v, ref):
        return float(np.linalg.norm((v.astype(np.longdouble) - ref).astype(np.float64)) / np.linalg.norm(ref.astype(np.float64)))

    ex, ey, ox, oy = err(x, x_ref), err(y, y_ref), err(xo, x_ref), err(yo, y_ref)
    report("project  %s %d x %d  x err %.2e (x%.2f of the oracle's direct projection), y err %.2e (x%.2f)"
           % (tname(dtype), m, n, ex, ex / ox, ey, ey / oy))
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(y))
    assert ex <= 4 * ox and ey <= 4 * oy, (ex, ox, ey, oy)


# ---- solves ------------------------------------------------------------------------------------------------------------

_problems = {}


def _lasso_case(shape):
    """(A, b): a CSR of density 0.05 with every row and column non-empty, and a sparse-signal right-hand side"""
    if shape not in _problems:
        m, n = shape
        rng = np.random.default_rng(3 * m + n)
        A = sp.random(m, n, 0.05, random_state=rng, format="lil", dtype=np.float64)
        for i in range(max(m, n)):
            if A[i % m, i % n] == 0:
                A[i % m, i % n] = rng.standard_normal()
        A = sp.csr_matrix(A)
        A.sort_indices()
        assert np.all(np.diff(A.indptr) > 0) and np.all(np.diff(A.tocsc().indptr) > 0)
        b = A @ (rng.standard_normal(n) * (rng.random(n) < 0.2)) + 0.1 * rng.standard_normal(m)
        _problems[shape] = (A, b)
    return _problems[shape]


_oracle = {}


def _oracle_solve(shape, family, dtype, lam=None, **kw):
    """the oracle's dense direct solve of a case, made once per module"""
    key = (shape, family, np.dtype(dtype).name, lam) if not kw else None
    if key is None or key not in _oracle:
        A, b = _lasso_case(shape)
        f, g = _fg(shape, family, lam)
        r = ob.oracle_solve(A.toarray(), soa(f), soa(g), dtype=dtype, **kw)
        if key is None:
            return r
        _oracle[key] = r
    return _oracle[key]


def _fg(shape, family, lam=None):
    A, b = _lasso_case(shape)
    if family == "lasso":
        return _pogs().graph.lasso_functions(b, 0.1 if lam is None else lam, shape[1])
    return PROBLEMS[family](b, shape[1])


def _follows(got, want, dtype, label):
    f64 = dtype == np.float64
    d_it = abs(int(got["iterations"]) - int(want["iterations"]))
    ex = relerr(got["x"], want["x"])
    eo = abs(got["optval"] - want["optval"]) / max(abs(want["optval"]), 1e-300)
    report("solve    %s %-34s iterations %d (oracle %d), |dx|/|x| %.2e, optval %.2e"
           % (tname(dtype), label, got["iterations"], want["iterations"], ex, eo))
    assert got["status"] == want["status"] == 0
    assert d_it <= (1 if f64 else 3), (got["iterations"], want["iterations"])
    assert ex < (1e-6 if f64 else 1e-4)
    assert eo <= (1e-6 if f64 else 2e-4)


def _counts(st):
    """a direct handle runs no CG step; 2 products per iteration and 2 more on an iteration with exact residuals (the two
    products of a warm start are set-up of the solve and are not counted)"""
    assert st["cg_iters"] == 0
    assert st["matvecs"] == 2 * st["iterations"] + 2 * st["exact_iters"], st


TALL, WIDE = (600, 150), (150, 600)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("order", ["csr", "csc"])
@pytest.mark.parametrize("shape", [TALL, WIDE])
def test_direct_lasso_follows_the_oracles_dense_direct_solve(shape, order, dtype):
    A, b = _lasso_case(shape)
    f, g = _fg(shape, "lasso")
    want = _oracle_solve(shape, "lasso", dtype)
    assert want["iterations"] > 50
    if order == "csr":
        s = _pogs().Solver(A, dtype=dtype, projector=DIRECT)
    else:
        C = A.tocsc()
        C.sort_indices()
        s = _raw_solver(shape, C.data, C.indptr, C.indices, dtype, order=_lib.COL_MAJ)
    with s:
        got = s.solve(f, g)
        st = s.stats()
    _follows(got, want, dtype, "lasso %d x %d %s" % (shape + (order,)))
    assert st["iterations"] == got["iterations"] + 1
    _counts(st)


@pytest.mark.parametrize("family,shape", [("logistic", TALL), ("svm", TALL), ("nonneg_ls", WIDE)])
def test_direct_other_families(family, shape):
    A, _ = _lasso_case(shape)
    f, g = _fg(shape, family)
    want = _oracle_solve(shape, family, np.float64)
    with _pogs().Solver(A, dtype=np.float64, projector=DIRECT) as s:
        got = s.solve(f, g)
        _counts(s.stats())
    _follows(got, want, np.float64, "%s %d x %d" % ((family,) + shape))


@pytest.mark.parametrize("shape", [TALL, WIDE])
def test_direct_warm_start_and_begin_run(shape):
    A, _ = _lasso_case(shape)
    f, g = _fg(shape, "lasso")
    with _pogs().Solver(A, dtype=np.float64, projector=DIRECT) as s:
        cold = s.solve(f, g)
        s.reset_stats()                    # (matvecs adds up over the solves of a handle)
        warm = s.solve(f, g, x0=cold["x"], l0=cold["l"])
        _counts(s.stats())
        n_it = cold["iterations"] + 1
        s.begin_run(f, g)
        assert s.iterate(n_it)[1] == 0     # the run stops at the solve's iteration ...
        assert s.iterate(1)[1] == 1        # ... so the next one starts a new solve
    want = _oracle_solve(shape, "lasso", np.float64, x0=cold["x"], l0=cold["l"])
    assert warm["iterations"] < cold["iterations"] and want["iterations"] < _oracle_solve(shape, "lasso", np.float64)["iterations"]
    _follows(warm, want, np.float64, "lasso %d x %d warm" % shape)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("order", ["csr", "csc"])
def test_direct_unsorted_indices_and_repeated_entries_through_the_raw_abi(order, dtype):
    from test_gpu_sparse import _messy_csr

    m, n = 600, 150
    if order == "csr":
        val, ptr, ind = _messy_csr(m, n, 9, seed=41)
        A_raw = sp.csr_matrix((val.astype(dtype), ind, ptr), shape=(m, n))
        ord_ = _lib.ROW_MAJ
    else:
        val, ptr, ind = _messy_csr(n, m, 30, seed=42)                             # the rows of A^T
        A_raw = sp.csc_matrix((val.astype(dtype), ind, ptr), shape=(m, n))
        ord_ = _lib.COL_MAJ
    assert not A_raw.has_canonical_format
    A_canon = sp.csr_matrix(A_raw.astype(np.float64)).copy()
    A_canon.sum_duplicates()
    rng = np.random.default_rng(43)
    b = A_canon @ (rng.standard_normal(n) * (rng.random(n) < 0.2)) + 0.1 * rng.standard_normal(m)
    f, g = _pogs().graph.lasso_functions(b, 0.1, n)
    runs = []
    for _ in range(3):
        with _raw_solver((m, n), val, ptr, ind, dtype, order=ord_) as s:
            runs.append((s.solve(f, g), s.factor()[0]))
            _counts(s.stats())
    for r, W in runs[1:]:
        assert r["iterations"] == runs[0][0]["iterations"] and same_bytes(W, runs[0][1])
        assert all(same_bytes(r[k], runs[0][0][k]) for k in "xyl")
    got = runs[0][0]
    with _pogs().Solver(A_canon, dtype=dtype, projector=DIRECT) as s:
        canon = s.solve(f, g)
    assert got["status"] == canon["status"] == 0 and relerr(got["x"], canon["x"]) < 1e-2
    obj = lambda v: 0.5 * np.sum((A_canon @ v.astype(np.float64) - b) ** 2) + 0.1 * np.abs(v).sum()  # noqa: E731
    assert obj(got["x"]) == pytest.approx(obj(canon["x"]), rel=1e-3)


def test_direct_device_resident_csr_gives_the_host_paths_bytes():
    import torch

    A, _ = _lasso_case(TALL)
    f, g = _fg(TALL, "lasso")
    A = sp.csr_matrix(A, dtype=np.float32)
    with _pogs().Solver(A, dtype=np.float32, projector=DIRECT) as s:
        host, Wh = s.solve(f, g), s.factor()[0]
    dev = torch.device("cuda:0")
    data = torch.from_numpy(np.ascontiguousarray(A.data, np.float32)).to(dev)
    ptr = torch.from_numpy(np.ascontiguousarray(A.indptr, np.int32)).to(dev)
    ind = torch.from_numpy(np.ascontiguousarray(A.indices, np.int32)).to(dev)
    with _pogs().Solver((data.data_ptr(), ptr.data_ptr(), ind.data_ptr(), A.nnz), dtype=np.float32, shape=A.shape,
                        device_ptr=True, projector=DIRECT) as s:
        got, Wd = s.solve(f, g), s.factor()[0]
    assert got["status"] == host["status"] == 0 and got["iterations"] == host["iterations"]
    assert same_bytes(Wd, Wh) and all(same_bytes(got[k], host[k]) for k in "xyl")


# ---- nothing else moved, refusals ----------------------------------------------------------------------------------

def test_default_and_cgls_handles_are_as_before_and_the_cg_check_refuses_a_direct_handle():
    A, _ = _lasso_case(TALL)
    f, g = _fg(TALL, "lasso")
    m, n = TALL
    out = []
    for proj in (_lib.PROJ_DEFAULT, _lib.PROJ_CGLS):
        with _pogs().Solver(A, dtype=np.float32, projector=proj) as s:
            out.append((s.solve(f, g), s.stats()))
            with pytest.raises(RuntimeError, match="needs a dense handle"):
                s.factor()
    (r0, st0), (r1, st1) = out
    assert r0["iterations"] == r1["iterations"] and st0["cg_iters"] == st1["cg_iters"] > 0
    assert all(same_bytes(r0[k], r1[k]) for k in ("x", "y", "l", "mu")) and r0["optval"] == r1["optval"]
    zx, zy = np.zeros(n, np.float32), np.zeros(m, np.float32)
    with _pogs().Solver(A, dtype=np.float32, projector=DIRECT) as s:
        with pytest.raises(RuntimeError, match="direct projector"):
            _lib.sparse_cg_check(s._h, zx, zy, zx, zy, zx, zx, zy, 1e-3, loop=_lib.CG_HOST_WARM)
        assert s.solve(f, g)["status"] == 0     # the handle is as it was


def test_direct_is_refused_beyond_the_cap_and_on_row_shards():
    pogs = _pogs()
    n = _lib.SPARSE_DIRECT_MAX + 1
    data, ptr, ind = np.ones(n, np.float32), np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    h = ctypes.c_void_p(1)
    opt = _lib.PogsAmdOptions(device=-1, projector=DIRECT, profile=0)
    rc = _lib.lib.PogsAmdCreateSparse(ctypes.byref(h), _lib.F32, _lib.ROW_MAJ, n, n, n, data.ctypes.data, ptr.ctypes.data,
                                      ind.ctypes.data, _lib.HOST, ctypes.byref(opt), None)
    assert rc != 0 and not h.value and str(_lib.SPARSE_DIRECT_MAX) in _lib.last_error()
    with pytest.raises(RuntimeError, match=str(_lib.SPARSE_DIRECT_MAX)):
        pogs.Solver(sp.identity(n, dtype=np.float32, format="csr"), dtype=np.float32, projector=DIRECT)
    A, _ = _lasso_case(TALL)
    uid = (b"POGSLOCAL:" + os.urandom(8).hex().encode()).ljust(128, b"\0")
    with pytest.raises(RuntimeError, match="single-GPU"):
        pogs.Solver(A, dtype=np.float32, projector=DIRECT, dist=(0, 1, TALL[0], uid))
    # the cap itself is served by the other projector, and the next direct handle works
    with pogs.Solver(sp.identity(n, dtype=np.float32, format="csr"), dtype=np.float32, projector=_lib.PROJ_CGLS) as s:
        assert s.stats()["nrmA"] > 0
    with pogs.Solver(A, dtype=np.float32, projector=DIRECT) as s:
        assert s.factor()[0].shape == (TALL[1], TALL[1])


# ---- batched solves on a direct handle ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [TALL, WIDE])
def test_batch_on_a_direct_handle(shape, dtype):
    from test_gpu_batch import _same_bytes

    A, b = _lasso_case(shape)
    n = shape[1]
    lams = [0.02 * 1.25 ** j for j in range(16)]
    fgs = [_pogs().graph.lasso_functions(b, lam, n) for lam in lams]
    fs, gs = [fg[0] for fg in fgs], [fg[1] for fg in fgs]
    with _pogs().Solver(A, dtype=dtype, projector=DIRECT) as s:
        solo = [s.solve(f, g) for f, g in fgs]
        three = s.solve_batch(fs[:3], gs[:3])
        st3 = s.stats()
        sixteen = s.solve_batch(fs, gs)
        st16 = s.stats()
        alone = s.solve_batch([fs[1]], [gs[1]])[0]
        # the same member in slot 1 of 3 and in slot 15 of 16, among other problems
        last = s.solve_batch(fs[2:] + fs[:1] + [fs[1]], gs[2:] + gs[:1] + [gs[1]])[15]
    assert st3["cg_iters"] == 0 and st16["cg_iters"] == 0
    assert st16["batch_problem_iters"] == sum(r["iterations"] + 1 for r in sixteen)
    assert len({r["iterations"] for r in sixteen}) > 1      # the members stop at different iterations
    _same_bytes(alone, three[1])
    _same_bytes(alone, sixteen[1])
    _same_bytes(alone, last)
    for j, (r, w) in enumerate(zip(sixteen, solo)):
        _follows(r, w, dtype, "batch member %d of 16, %d x %d" % ((j,) + shape))
    for r, w in zip(three, sixteen[:3]):
        _same_bytes(r, w)
