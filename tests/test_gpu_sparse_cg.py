"""The device-resident CGLS loop of the sparse projector (csrc/cg_fused.h: cgf_reduce_kernel, cgf_step_a_kernel,
cgf_step_b_kernel, cgf_close_kernel; SparseOperator::spmv_cg; SparseSolver::cg_loop_fused with its enqueue-ahead and
growing-chunk polling) on its own, through PogsAmdSparseCgCheck (include/pogs_amd.h, Part 3), against a model of the
same recurrence written here and run in fp64 (fp32 handle) or long double (fp64 handle).

The model (`cg_model`) restates cgls.h:236-305 as cg_fused.h does: s = A^T r - x, p = s, gamma = |s|^2 (no step if
sqrt(gamma) < eps_T); per step q = A p, alpha = gamma / (|q|^2 + |p|^2), x += alpha p, r -= alpha q, y += alpha q from
y_warm, s = A^T r - x, beta = |s|^2 / gamma; stop when |s| <= |s_0| tol, or |x| tol >= 1, or at the cap, else
p = s + beta p; at the end x += x0 and the four bookkeeping sums.  A is the handle's equilibrated matrix (PogsAmdGetEquil).

Bar.  The same model run with numpy in the handle's own type gives the error rounding alone causes: for a vector,
E_ref = |working-precision model - high-precision model|_2, and the device must be within 8 max(E_ref, eps_T scale) of the
high-precision model, scale = |x0| + |x_warm| (n-sized) or |y0| + |y_warm| (m-sized); the 8 covers another order of
summation, fused multiply-adds and the double-precision record sums.  A scalar is held to the same rule with the model's
value as its scale: 8 max(E_ref, eps_T |model's value|).  That rule holds for every scalar of every case but the few in
the table RAISED: each of those exceeded it by rounding (the ratios: profiles/sparse_cg_accuracy.txt), and takes there --
in that shape, type and case only -- the larger of the rule and what the bars of the vectors it is formed from let
through (|v|^2 moves by 2 |v| bar_v + bar_v^2 when v moves by bar_v; a sum by the bars of its terms; a quotient by both
operands).  Each such case prints the ratio under the rule alone next to the one it asserts.  The sums behind them:
    alpha at the natural stop at step 8, 900 x 400 fp64.  alpha = |s_7|^2 / (|q|^2 + |p|^2), sums over the records of
        vectors that have shrunk with |s_j| / |s_0| to 1e-4 of the inputs, while their rounding errors, set by r and x in
        s = A^T r - x, have not: a relative error of 1e4 eps in each sum is rounding, and E_ref, one signed draw of an
        error of that size, can fall well below the device's draw.
    1 x 700 fp32.  y, q and r are one number each, and q is the row dot of 700 terms of either sign (A p in
        spmv_sell_kernel): its rounding error is set by the sum of the terms' magnitudes, not by |q|.  After one step
        |q|^2, dyprev2 = (alpha q)^2 and, through r_1 = r - alpha q, |s_1|^2 (s2, gamma1) and beta carry it; after two,
        |q|^2 again, gamma1, and |p|^2 and delta through p_1 = s_1 + beta p_0.
    700 x 1, both types.  One step solves a one-column problem exactly: s_1 = A^T r_1 - x_1 is rounding only, about
        p (1 - alpha_T delta) with alpha_T the one rounding of alpha to the type, and |s_1|^2 (s2, gamma1) and beta =
        |s_1|^2 / gamma are squares of one signed draw.  The vector s itself is held to its bar of 8 eps_T scale.
The raised bars are asserted finite, and a quotient's only holds where its divisor is more than twice its own bar.  No
constant comes from a device run; every case prints its largest error / bar ratio (pytest -s).

Stopping decisions do not depend on rounding: a case that needs the stop after exactly k steps takes the high-precision
model's |s_j| / |s_0|, asserts that steps k - 1 and k are a factor 2 or more apart, that step k is at 100 eps_T or more
and that |x_j| tol stays below 1/2, and puts tol at the geometric mean.  The inputs are scaled to |x0| + |x_warm| = 1 for that; y_warm = A x_warm rounded
to the type, as inside a solve.

Shapes (every context asserts from the returned geometry words that it reached its path; both types):
    900 x 400                         one block in every launch of the loop's own kernels (A's product: two row ranges)
    1025 x 1024, 1024 x 1025          the 1024 boundary of cgf_blocks and pre_blocks: a second block of one element
    513 x 700                         two row ranges of A: two records from one product with ncg 1
    3000 x 18433, 30 000 non-zeros    A has two column groups: q = A p through cgf_reduce_kernel with 3 blocks and the
                                      clamped four-way unroll; n takes 19 blocks, the last with one element.  Rows in
                                      groups of five that share ten columns: with scattered entries the rows are
                                      nearly orthogonal and |s_8| / |s_0| falls to 3e-7, the rounding of s in fp32
    18433 x 3000, 30 000 non-zeros    m far beyond n: blocks past nb_n do the m side and leave no record; A^T has two
                                      column groups, so the s functor runs in cgf_reduce_kernel
    1 x 1, 1 x 700, 700 x 1           rank one
    600 x 500                         rows 0, 1, 599 and columns 0, 499 empty

Not covered: the row-sharded branch (u, t, rec_s) needs several GPUs; kFcIndef cannot be set with shift 1 unless p is
zero; more than 1024 records in cgf_sum needs millions of rows; max_steps 2 at 1 x 1 and 700 x 1 (with one column the
first step is exact, and whether a second one runs at tol 0 hangs on the rounding noise left in s: test_rank_one runs
the cap of 2 at 1 x 700 only)."""
import ctypes
import os
import threading

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import hi, same_bytes
from pogs_amd import _lib

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
VEC_KEYS = ("x", "y_new", "xtemp", "ytemp", "r", "p", "s")
M_SIZED = ("y_new", "ytemp", "r")
SCALARS = ("norms0", "gamma0", "gamma1", "alpha", "beta", "delta", "q2", "p2", "s2", "x2", "dxprev2", "dx12", "dyprev2",
           "dy12")


def tname(dt):
    return "fp32" if dt == np.float32 else "fp64"


def report(line):
    print("sparse_cg: " + line)


# ---- matrices --------------------------------------------------------------------------------------------------

def _coo(m, n, rows, cols, seed):
    rng = np.random.default_rng(seed)
    A = sp.coo_matrix((rng.standard_normal(len(rows)), (rows, cols)), shape=(m, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def per_row(m, n, k, seed, empty_rows=(), empty_cols=()):
    """k entries in every row (fewer where n < k), none in the rows and columns listed"""
    rng = np.random.default_rng(seed)
    ok_cols = np.setdiff1d(np.arange(n), np.asarray(empty_cols, np.int64))
    rows, cols = [], []
    for i in range(m):
        if i in empty_rows:
            continue
        c = rng.choice(ok_cols, size=min(k, ok_cols.size), replace=False)
        rows += [i] * c.size
        cols += list(c)
    return _coo(m, n, rows, cols, seed + 1000)


def scattered(m, n, nnz, seed):
    """nnz entries with every row and every column hit at least once"""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([np.arange(m), rng.integers(0, m, nnz - m)]) if m >= n else rng.integers(0, m, nnz)
    cols = rng.integers(0, n, nnz) if m >= n else np.concatenate([np.arange(n), rng.integers(0, n, nnz - n)])
    if m >= n:
        cols[:n] = rng.permutation(n)
    else:
        rows[:m] = rng.permutation(m)
    return _coo(m, n, rows, cols, seed + 1000)


def grouped(m, n, g, k, seed):
    """rows in groups of g that share k columns (the first and the last column among them), no other entries: the
    singular values of the equilibrated matrix spread, so CGLS converges by a factor of about 3 per step"""
    rng = np.random.default_rng(seed)
    ng = m // g
    cols = rng.permutation(n - 2)[:ng * k - 2] + 1
    cols = rng.permutation(np.concatenate([cols, [0, n - 1]])).reshape(ng, k)
    return _coo(m, n, np.repeat(np.arange(m), k), np.repeat(cols, g, axis=0).ravel(), seed + 1000)


def blocks_1024(k):
    return max(1, -(-k // 1024))


# name -> (builder, general?, check of the geometry words (info_A, info_At, m, n))
SHAPES = {
    "900x400": (lambda: per_row(900, 400, 10, 11), True,
                lambda a, t, m, n: a["ncg"] == 1 and t["nrr"] * t["ncg"] == 1 and blocks_1024(max(m, n)) == 1),
    "1025x1024": (lambda: per_row(1025, 1024, 10, 12), True,
                  lambda a, t, m, n: blocks_1024(m) == 2 and blocks_1024(n) == 1 and a["ncg"] == 1 and t["ncg"] == 1),
    "1024x1025": (lambda: per_row(1024, 1025, 10, 13), True,
                  lambda a, t, m, n: blocks_1024(m) == 1 and blocks_1024(n) == 2 and a["ncg"] == 1 and t["ncg"] == 1),
    "513x700": (lambda: per_row(513, 700, 10, 14), True,
                lambda a, t, m, n: a["nrr"] == 2 and a["ncg"] == 1 and a["rr_rows"] == 512),
    "3000x18433": (lambda: grouped(3000, 18433, 5, 10, 15), True,
                   lambda a, t, m, n: a["ncb"] == 2 and a["ncg"] == 2 and blocks_1024(m) == 3 and blocks_1024(n) == 19
                   and n % 1024 == 1),
    "18433x3000": (lambda: scattered(18433, 3000, 30000, 16), True,
                   lambda a, t, m, n: t["ncb"] == 2 and t["ncg"] == 2 and blocks_1024(m) == 19 and blocks_1024(n) == 3),
    "600x500_empty": (lambda: per_row(600, 500, 10, 17, empty_rows=(0, 1, 599), empty_cols=(0, 499)), True,
                      lambda a, t, m, n: a["ncg"] == 1 and t["nrr"] * t["ncg"] == 1),
    "1x1": (lambda: per_row(1, 1, 1, 18), False, lambda a, t, m, n: True),
    "1x700": (lambda: per_row(1, 700, 700, 19), False, lambda a, t, m, n: True),
    "700x1": (lambda: per_row(700, 1, 1, 20), False, lambda a, t, m, n: True),
}
GENERAL = [k for k, v in SHAPES.items() if v[1]]
RANK_ONE = [k for k, v in SHAPES.items() if not v[1]]
DEEP = ("900x400", "3000x18433")   # the natural stop at step 8 as well


# ---- the model ---------------------------------------------------------------------------------------------------

class Mat:
    """A and A^T as CSR arrays with reduceat products in a given type"""

    def __init__(self, A):
        At = A.T.tocsr()
        At.sort_indices()
        self.m, self.n = A.shape
        self.a = (A.indptr, A.indices, A.data)
        self.t = (At.indptr, At.indices, At.data)

    def mul(self, trans, x, dt):
        ptr, ind, v = self.t if trans else self.a
        out = np.zeros(ptr.size - 1, dt)
        ne = np.diff(ptr) > 0
        if ne.any():
            out[ne] = np.add.reduceat(v.astype(dt) * x[ind], ptr[:-1][ne])
        return out


def cg_model(M, inp, tol, max_steps, dt, eps):
    """the recurrence in type dt; eps: the handle's machine epsilon (the zero-step test).  Returns what the entry returns
    plus y_prod = A x (ysync), ratios[j] = |s_(j+1)| / |s_0| and xnorms[j] = |x_(j+1)| after each step."""
    c = lambda v: np.asarray(v).astype(dt)   # noqa: E731
    x0, y0, xw, yw, xprev, x12, y12 = (c(inp[k]) for k in ("x0", "y0", "x_warm", "y_warm", "x_prev", "x12", "y12"))
    sq = lambda v: np.sum(v * v, dtype=dt)   # noqa: E731
    tol = dt(tol)
    r, x = y0 - yw, xw - x0
    s = M.mul(True, r, dt) - x
    p = s.copy()
    gamma = sq(s)
    out = dict(norms0=gamma, gamma0=gamma, gamma1=dt(0), steps=0, ratios=[], xnorms=[], s_prev=s.copy(),
               q=np.zeros(M.m, dt))
    y = yw.copy()
    if not np.sqrt(gamma) < dt(eps):
        norms0 = np.sqrt(gamma)
        for k in range(max_steps):
            q = M.mul(False, p, dt)
            q2, p2 = sq(q), sq(p)
            delta = q2 + p2
            alpha = gamma / delta
            x = x + alpha * p
            r = r - alpha * q
            y = y + alpha * q
            out.update(s_prev=s, q=q)
            s = M.mul(True, r, dt) - x
            s2, x2 = sq(s), sq(x)
            beta = s2 / gamma
            gamma = s2
            out["gamma%d" % ((k + 1) & 1)] = s2
            out.update(alpha=alpha, beta=beta, delta=delta, q2=q2, p2=p2, s2=s2, x2=x2, steps=k + 1)
            out["ratios"].append(np.sqrt(s2) / norms0)
            out["xnorms"].append(np.sqrt(x2))
            if np.sqrt(s2) <= norms0 * tol or np.sqrt(x2) * tol >= 1 or k + 1 >= max_steps:
                break
            p = s + beta * p
    xn = x + x0
    out.update(x=xn, y_new=y, xtemp=x0 - xn, ytemp=y0 - y, r=r, p=p, s=s, y_prod=M.mul(False, xn, dt),
               dxprev2=sq(xprev - xn), dx12=sq(x12 - xn), dyprev2=sq(yw - y), dy12=sq(y12 - y))
    return out


# ---- one handle per shape and type ---------------------------------------------------------------------------------

class Ctx:
    def __init__(self, name, dt):
        import pogs_amd

        self.name, self.dt, self.eps = name, dt, float(np.finfo(dt).eps)
        self.A = SHAPES[name][0]()
        self.m, self.n = self.A.shape
        self.solver = pogs_amd.Solver(self.A, dtype=dt)
        buf = np.zeros(self.A.nnz, dt)
        assert _lib.lib.PogsAmdGetEquil(self.solver._h, buf.ctypes.data_as(ctypes.c_void_p), None, None, None) == 0
        self.Aeq = sp.csr_matrix((buf, self.A.indices, self.A.indptr), shape=self.A.shape)
        self.M = Mat(self.Aeq)
        self.hi = hi(np.zeros(1, dt)).dtype.type
        self._inputs, self._models = {}, {}

    def inputs(self, seed=0, zero_warm=False, same=False):
        """x0, y0, x_warm, y_warm (= A x_warm), x_prev, x12, y12 with |x0| + |x_warm| = 1; same: x0 = x_warm, y0 = y_warm,
        x_prev = x_warm"""
        key = (seed, zero_warm, same)
        if key not in self._inputs:
            rng = np.random.default_rng(100 + seed)
            g = {k: rng.standard_normal(self.n) for k in ("x0", "x_warm", "x_prev", "x12")}
            g.update({k: rng.standard_normal(self.m) for k in ("y0", "y12")})
            if zero_warm:
                g["x_warm"] = np.zeros(self.n)
            c = 1.0 / (np.linalg.norm(g["x0"]) + np.linalg.norm(g["x_warm"]))
            g = {k: (c * v).astype(self.dt) for k, v in g.items()}
            g["y_warm"] = self.M.mul(False, hi(g["x_warm"]), self.hi).astype(self.dt)
            if same:
                g["x0"], g["y0"], g["x_prev"] = g["x_warm"].copy(), g["y_warm"].copy(), g["x_warm"].copy()
            self._inputs[key] = g
        return self._inputs[key]

    def models(self, inp_key, inp, tol, max_steps):
        """(high-precision model, working-precision model), computed once per argument set"""
        key = (inp_key, float(tol), max_steps)
        if key not in self._models:
            self._models[key] = (cg_model(self.M, inp, tol, max_steps, self.hi, self.eps),
                                 cg_model(self.M, inp, tol, max_steps, self.dt, self.eps))
        return self._models[key]

    def run(self, inp, tol, **kw):
        out = _lib.sparse_cg_check(self.solver._h, inp["x0"], inp["y0"], inp["x_warm"], inp["y_warm"], inp["x_prev"],
                                   inp["x12"], inp["y12"], tol, **kw)
        assert SHAPES[self.name][2](out["info"][0], out["info"][1], self.m, self.n), out["info"]
        assert all(i["tiled"] == 1 for i in out["info"])
        if kw.get("loop", 0) == 0 and out["steps"] > 0:
            # one |x|^2 record per block of the n side, none from the blocks beyond it (they do the m side only)
            nb_n = blocks_1024(self.n)
            assert np.all(np.isfinite(out["rec_x"][:nb_n])) and np.all(np.isnan(out["rec_x"][nb_n:])), (nb_n, out["rec_x"][:24])
            assert abs(out["rec_x"][:nb_n].sum() - out["x2"]) <= 1e-12 * out["x2"]
        return out

    def stop_tol(self, inp_key, inp, k):
        """tol that stops the loop after exactly k steps by the first clause, whatever the rounding"""
        ratios = self.models(inp_key, inp, 0.0, k)[0]["ratios"]
        assert len(ratios) == k
        prev = ratios[k - 2] if k >= 2 else self.hi(1)
        assert prev / ratios[k - 1] >= 2, (self.name, k, [float(v) for v in ratios])
        assert all(ratios[j - 1] / ratios[j] > 1 for j in range(1, k)), [float(v) for v in ratios]
        assert ratios[k - 1] >= 100 * self.eps, (self.name, k, float(ratios[k - 1]))   # |s_k| well above the rounding of s
        tol = float(np.sqrt(prev * ratios[k - 1]))
        xn = self.models(inp_key, inp, 0.0, k)[0]["xnorms"]
        assert all(float(v) * tol <= 0.5 for v in xn), (tol, [float(v) for v in xn])
        return tol


_CTX = {}


def get_ctx(name, dt):
    if (name, dt) not in _CTX:
        _CTX[(name, dt)] = Ctx(name, dt)
    return _CTX[(name, dt)]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for c in _CTX.values():
        c.solver.close()
    _CTX.clear()


def on(names):
    """one case per listed shape and type; the test gets the shape's context (its handle is built once)"""
    return pytest.mark.parametrize("ctx", [(s, d) for s in names for d in DTYPES], indirect=True,
                                   ids=lambda p: "%s-%s" % (p[0], tname(p[1])))


@pytest.fixture
def ctx(request):
    return get_ctx(*request.param)


# ---- comparison ----------------------------------------------------------------------------------------------------

# (shape, type, case) -> the scalars whose bar is raised there, each one that exceeded the relative rule by rounding (the
# module docstring: Bar); everywhere else, and for every other scalar in these cases, the relative rule holds alone
_ROW_DOT_1 = ("q2", "s2", "gamma1", "beta", "dyprev2")      # one step at 1 x 700: what the row dot q feeds
_EXACT_STEP = ("s2", "gamma1", "beta")                      # one step at 700 x 1: |s_1|^2 of an s_1 that is rounding only
RAISED = {
    ("900x400", "fp64", "stop 8"): ("alpha",),
    ("1x700", "fp32", "cap 1"): _ROW_DOT_1,
    ("1x700", "fp32", "tol 1e-2"): _ROW_DOT_1,
    ("1x700", "fp32", "cap 2"): ("q2", "p2", "delta", "gamma1"),
    ("700x1", "fp32", "cap 1"): _EXACT_STEP,
    ("700x1", "fp32", "tol 1e-2"): _EXACT_STEP,
    ("700x1", "fp64", "cap 1"): _EXACT_STEP,
    ("700x1", "fp64", "tol 1e-2"): _EXACT_STEP,
}


def raised_in(ctx, case):
    return RAISED.get((ctx.name, tname(ctx.dt), case), ())


def worst_ratio(ctx, inp, got, mh, mw, vecs=VEC_KEYS, scalars=SCALARS, raised=()):
    """largest error / bar over the named vectors and scalars (the module docstring: Bar) and the quantity that has it;
    for a scalar in `raised`, the bar is the larger of the relative rule and what the bars of its vectors let through,
    and its ratio under the relative rule alone is reported next to it"""
    sx = float(np.linalg.norm(hi(inp["x0"])) + np.linalg.norm(hi(inp["x_warm"])))
    sy = float(np.linalg.norm(hi(inp["y0"])) + np.linalg.norm(hi(inp["y_warm"])))

    def vbar(k):
        e_ref = float(np.linalg.norm(hi(mw[k]) - mh[k]))
        return 8 * max(e_ref, ctx.eps * (sy if k in M_SIZED + ("q",) else sx))

    def sqbar(v, bar):
        """of |v|^2 when v is within bar of the model's"""
        return 2 * float(np.linalg.norm(v)) * bar + bar * bar

    worst, where = 0.0, ""
    for k in vecs:
        assert np.all(np.isfinite(got[k])), k
        err = float(np.linalg.norm(hi(got[k]) - mh[k]))
        if err / vbar(k) > worst:
            worst, where = err / vbar(k), k
    # a scalar: the rule of the vectors with the model's value as the scale.  The few named in `raised` take, where that
    # is more, what the bars of the vectors they are formed from let through: the sum of the squares of v moves by
    # 2 |v| bar + bar^2, delta = |q|^2 + |p|^2 by the two together, a quotient by both operands
    steps = mh["steps"]
    cur = "gamma%d" % (steps & 1)                  # the slot that holds |s|^2 of the last step

    def quotient_bar(k, b_num, den, b_den):
        assert den > 2 * b_den, (k, den, b_den)    # a bound, not a pole
        return (b_num + abs(float(mh[k])) * b_den) / (den - b_den)

    def raised_bar(k):
        assert steps >= 1, k
        b_q2, b_p2 = sqbar(mh["q"], vbar("q")), sqbar(mh["p"], vbar("p"))     # (p: the last step's, see cg_model)
        b_s2, b_gprev = sqbar(mh["s"], vbar("s")), sqbar(mh["s_prev"], vbar("s_prev"))
        prev = "gamma%d" % ((steps - 1) & 1)
        g_prev = float(mh[prev])
        if k == "alpha":
            return quotient_bar(k, b_gprev, float(mh["delta"]), b_q2 + b_p2)
        if k == "beta":
            return quotient_bar(k, b_s2, g_prev, b_gprev)
        if k == "dyprev2":
            return sqbar(hi(inp["y_warm"]) - mh["y_new"], vbar("y_new"))
        return {"q2": b_q2, "p2": b_p2, "delta": b_q2 + b_p2, "s2": b_s2, cur: b_s2, prev: b_gprev}[k]

    alone, over = [], []
    for k in scalars:
        assert np.isfinite(got[k]), k
        e_ref = abs(float(ctx.hi(mw[k]) - mh[k]))
        err = abs(float(ctx.hi(got[k]) - mh[k]))
        bar = rel = 8 * max(e_ref, ctx.eps * abs(float(mh[k])))
        if k in raised:
            bar = max(rel, raised_bar(k))
            alone.append("%s %.2f" % (k, err / rel))
        assert np.isfinite(bar), (k, bar)
        r = err / bar if bar > 0 else (0.0 if err == 0 else np.inf)
        if r > 1:
            over.append("%s %.2f" % (k, r))
        if r > worst:
            worst, where = r, k
    if alone:
        where += "; raised, under the relative rule alone: " + ", ".join(alone)
    if over:
        where += "; above the bar: " + ", ".join(over)
    return worst, where


def same_result(a, b, keys=VEC_KEYS + _lib.CG_SLOTS):
    return [k for k in keys if not same_bytes(np.asarray(a[k]), np.asarray(b[k]))]


def predicted_enqueued(ahead, steps, cap=500):
    """the poll rule of cg_loop_fused: `ahead` steps, then chunks of 1, 2, 4, ... 64 until the loop has ended"""
    enq, more = min(ahead, cap), 1
    while enq < steps:
        enq += min(more, cap - enq)
        more = min(2 * more, 64)
    return enq


# ---- cases ---------------------------------------------------------------------------------------------------------

@on(GENERAL)
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_capped_steps_match_the_model(ctx, cap):
    inp = ctx.inputs()
    mh, mw = ctx.models("base", inp, 0.0, cap)
    assert mh["steps"] == cap
    got = ctx.run(inp, 0.0, max_steps=cap, ahead=1)
    assert got["steps"] == cap and got["done"] == 1.0 and got["indef"] == 0.0
    assert got["enqueued"] == predicted_enqueued(1, cap, cap)
    worst, where = worst_ratio(ctx, inp, got, mh, mw)
    report("%s %s cap %d: error / bar %.3f (%s)" % (ctx.name, tname(ctx.dt), cap, worst, where))
    assert worst <= 1.0, (worst, where)


@pytest.mark.parametrize("ctx,k", [((s, d), k) for s in GENERAL for d in DTYPES for k in ((3, 8) if s in DEEP else (3,))],
                         indirect=["ctx"], ids=lambda v: "%s-%s" % (v[0], tname(v[1])) if isinstance(v, tuple) else str(v))
def test_natural_stop_and_the_steps_enqueued_ahead(ctx, k):
    inp = ctx.inputs()
    tol = ctx.stop_tol("base", inp, k)
    mh, mw = ctx.models("base", inp, tol, 500)
    assert mh["steps"] == k and mw["steps"] == k
    runs = {}
    for ahead in (1, k, k + 5, 64):
        got = ctx.run(inp, tol, ahead=ahead)
        assert got["steps"] == k and got["done"] == 1.0
        assert got["enqueued"] == predicted_enqueued(ahead, k), (ahead, got["enqueued"])
        runs[ahead] = got
    for ahead in (k, k + 5, 64):
        assert same_result(runs[1], runs[ahead]) == [], ahead
    worst, where = worst_ratio(ctx, inp, runs[1], mh, mw, raised=raised_in(ctx, "stop %d" % k))
    report("%s %s stop at %d (tol %.3e): error / bar %.3f (%s)" % (ctx.name, tname(ctx.dt), k, tol, worst, where))
    assert worst <= 1.0, (worst, where)


@on(GENERAL)
@pytest.mark.parametrize("ahead", [1, 8])
@pytest.mark.parametrize("variant", ["same", "tiny"])
def test_zero_steps(ctx, ahead, variant):
    """same: x0 = x_warm, y0 = y_warm, so s_0 = 0.  tiny: the general inputs times eps_T / 64, so |s_0| < eps_T with
    y0 != y_warm and x0 != x_warm: ytemp - y_warm and x_warm - x0 + x0 are not trivial there."""
    if variant == "same":
        inp = ctx.inputs(same=True)
    else:
        c = ctx.dt(ctx.eps / 64)                                   # a power of two: the scaling is exact
        inp = {k: c * v for k, v in ctx.inputs().items()}
        inp["x_prev"] = inp["x_warm"].copy()
        assert inp["y0"].dtype == ctx.dt and np.any(inp["y0"] != inp["y_warm"])
    mh, mw = ctx.models(variant, inp, 1e-3, 500)
    assert mh["steps"] == 0 and mw["steps"] == 0
    assert float(np.sqrt(mh["gamma0"])) <= ctx.eps / 2             # the zero-step decision does not hang on rounding
    got = ctx.run(inp, 1e-3, ahead=ahead)
    assert got["steps"] == 0.0 and got["done"] == 1.0
    x_new = (inp["x_warm"] - inp["x0"]) + inp["x0"]                # the two roundings of the loop's x, then of the close
    assert same_bytes(got["y_new"], inp["y_warm"]) and same_bytes(got["x"], x_new)
    assert got["dyprev2"] == 0.0
    assert same_bytes(got["ytemp"], inp["y0"] - inp["y_warm"])
    assert same_bytes(got["xtemp"], inp["x0"] - x_new)
    if variant == "same":
        assert same_bytes(got["x"], inp["x_warm"]) and got["dxprev2"] == 0.0 and not got["ytemp"].any()
    worst, where = worst_ratio(ctx, inp, got, mh, mw, vecs=("x", "y_new", "xtemp", "ytemp", "r"),
                               scalars=("dxprev2", "dx12", "dy12"))
    report("%s %s zero steps (%s, ahead %d): error / bar %.3f (%s)" % (ctx.name, tname(ctx.dt), variant, ahead, worst, where))
    assert worst <= 1.0, (worst, where)


@on(GENERAL)
def test_second_stopping_clause(ctx):
    base = ctx.inputs()
    tol = ctx.stop_tol("base", base, 2)            # below the step-1 ratio: the first clause lets step 1 pass
    x1 = float(ctx.models("base", base, 0.0, 2)[0]["xnorms"][0])
    for target, want in ((4.0, 1), (0.25, 2)):
        c = target / (x1 * tol)
        inp = {k: (ctx.dt(c) * v).astype(ctx.dt) for k, v in base.items()}
        mh, mw = ctx.models("scaled%g" % target, inp, tol, 500)
        # the clause's own margin: |x_1| tol within a factor 2 of 1 in neither run, and with 0.25 step 2 ends by clause one
        assert abs(float(mh["xnorms"][0]) * tol / target - 1) < 0.01
        assert mh["steps"] == want and mw["steps"] == want
        if want == 2:
            assert float(mh["xnorms"][1]) * tol <= 0.5
        got = ctx.run(inp, tol, ahead=1)
        assert got["steps"] == want and got["done"] == 1.0
        worst, where = worst_ratio(ctx, inp, got, mh, mw)
        report("%s %s |x_1| tol = %g: error / bar %.3f (%s)" % (ctx.name, tname(ctx.dt), target, worst, where))
        assert worst <= 1.0, (worst, where)


@on(GENERAL)
def test_ysync_product_against_the_recurrence(ctx):
    inp = ctx.inputs()
    tol = ctx.stop_tol("base", inp, 3)
    mh, mw = ctx.models("base", inp, tol, 500)
    rec = ctx.run(inp, tol, ahead=3, ysync=False)
    prod = ctx.run(inp, tol, ahead=3, ysync=True)
    assert rec["steps"] == prod["steps"] == 3
    assert same_result(rec, prod, ("x", "xtemp", "r", "p", "s", "dxprev2", "dx12", "alpha", "beta")) == []
    ys = ("y_new", "ytemp")
    sc = ("dyprev2", "dy12")
    # y = A x: the recurrence and the product each against the model's product, and each against its own model
    w1, k1 = worst_ratio(ctx, inp, rec, mh, mw, vecs=ys, scalars=sc)
    w2, k2 = worst_ratio(ctx, inp, prod, dict(mh, y_new=mh["y_prod"]), dict(mw, y_new=mw["y_prod"]), vecs=("y_new",), scalars=())
    w3, k3 = worst_ratio(ctx, inp, rec, dict(mh, y_new=mh["y_prod"]), dict(mw, y_new=mw["y_prod"]), vecs=("y_new",), scalars=())
    w4, k4 = worst_ratio(ctx, inp, prod, mh, mw, vecs=ys, scalars=sc)
    report("%s %s ysync: recurrence %.3f (%s), product %.3f, recurrence against A x %.3f, product against the recurrence "
           "%.3f (%s)" % (ctx.name, tname(ctx.dt), w1, k1, w2, w3, w4, k4))
    assert max(w1, w2, w3, w4) <= 1.0, (w1, w2, w3, w4)


@on(GENERAL)
def test_the_host_polled_loop_agrees(ctx):
    inp = ctx.inputs()
    tol = ctx.stop_tol("base", inp, 3)
    mh, mw = ctx.models("base", inp, tol, 500)
    warm = ctx.run(inp, tol, loop=_lib.CG_HOST_WARM)
    assert warm["enqueued"] == 3
    cmp_v, cmp_s = ("x", "xtemp", "r", "s"), ("dxprev2", "dx12", "s2", "x2")
    w1, k1 = worst_ratio(ctx, inp, warm, mh, mw, vecs=cmp_v, scalars=cmp_s)
    w1y, _ = worst_ratio(ctx, inp, warm, dict(mh, y_new=mh["y_prod"]), dict(mw, y_new=mw["y_prod"]), vecs=("y_new",), scalars=())
    # cold: x_warm = 0, y_warm = 0; both loops against one model
    inp0 = ctx.inputs(zero_warm=True)
    assert not inp0["y_warm"].any()
    tol0 = ctx.stop_tol("zero_warm", inp0, 3)
    mh0, mw0 = ctx.models("zero_warm", inp0, tol0, 500)
    fused = ctx.run(inp0, tol0, ahead=3)
    cold = ctx.run(inp0, tol0, loop=_lib.CG_HOST_COLD)
    assert fused["steps"] == 3 and cold["enqueued"] == 3
    w2, k2 = worst_ratio(ctx, inp0, fused, mh0, mw0)
    w3, k3 = worst_ratio(ctx, inp0, cold, mh0, mw0, vecs=cmp_v, scalars=cmp_s)
    report("%s %s host-polled: warm %.3f (%s), its y %.3f, cold start: device-resident %.3f (%s), host-polled %.3f (%s)"
           % (ctx.name, tname(ctx.dt), w1, k1, w1y, w2, k2, w3, k3))
    assert max(w1, w1y, w2, w3) <= 1.0, (w1, w1y, w2, w3)


def _lasso(ctx):
    import pogs_amd

    rng = np.random.default_rng(7)
    b = rng.standard_normal(ctx.m)
    return pogs_amd.graph.lasso_functions(b, 0.1, ctx.n)


@on(("900x400", "1024x1025"))
def test_the_call_keeps_no_state_and_leaves_the_handle_as_it_was(ctx):
    import pogs_amd

    inp = ctx.inputs()
    tol = ctx.stop_tol("base", inp, 3)
    f, g = _lasso(ctx)
    with pogs_amd.Solver(ctx.A, dtype=ctx.dt) as fresh:
        want = fresh.solve(f, g)
        want_stats = fresh.stats()
    first = ctx.run(inp, tol, ahead=2)
    assert same_result(first, ctx.run(inp, tol, ahead=2)) == []
    stats0 = ctx.solver.stats()
    ctx.run(inp, tol, ahead=2)
    assert ctx.solver.stats() == stats0
    got = ctx.solver.solve(f, g)
    for k in ("x", "y", "l", "mu"):
        assert same_bytes(got[k], want[k]), k
    assert (got["iterations"], got["status"], got["optval"]) == (want["iterations"], want["status"], want["optval"])
    assert ctx.solver.stats()["cg_iters"] - stats0["cg_iters"] == want_stats["cg_iters"]
    assert same_result(first, ctx.run(inp, tol, ahead=2)) == []       # after a full solve (the other pair of buffers)
    again = ctx.solver.solve(f, g)
    assert same_bytes(again["x"], want["x"]) and again["iterations"] == want["iterations"]


@on(RANK_ONE)
def test_rank_one(ctx):
    """max_steps 1 and 2 against the model (2 only for n > 1: with one column the first step is exact, and whether a
    second one runs on the rounding noise left in s is not a property of the loop), then tol = 1e-2."""
    inp = ctx.inputs()
    worst = 0.0
    for cap in ((1, 2) if ctx.n > 1 else (1,)):
        mh, mw = ctx.models("base", inp, 0.0, cap)
        assert mh["steps"] == cap
        got = ctx.run(inp, 0.0, max_steps=cap, ahead=cap)
        assert got["steps"] == cap and got["done"] == 1.0
        w, where = worst_ratio(ctx, inp, got, mh, mw, raised=raised_in(ctx, "cap %d" % cap))
        report("%s %s cap %d: error / bar %.3f (%s)" % (ctx.name, tname(ctx.dt), cap, w, where))
        worst = max(worst, w)
    # tol = 1e-2: the model's ratios must be a factor 2 away from it at every step it takes
    mh, mw = ctx.models("base", inp, 1e-2, 500)
    assert mh["steps"] == mw["steps"] and all(float(v) <= 0.5e-2 or float(v) >= 2e-2 for v in mh["ratios"])
    assert all(float(v) * 1e-2 <= 0.5 for v in mh["xnorms"])
    got = ctx.run(inp, 1e-2, ahead=1)
    assert got["steps"] == mh["steps"] and got["done"] == 1.0
    assert got["enqueued"] == predicted_enqueued(1, mh["steps"])
    w, where = worst_ratio(ctx, inp, got, mh, mw, raised=raised_in(ctx, "tol 1e-2"))
    report("%s %s tol 1e-2, %d steps: error / bar %.3f (%s)" % (ctx.name, tname(ctx.dt), mh["steps"], w, where))
    assert max(worst, w) <= 1.0


# ---- refusals ------------------------------------------------------------------------------------------------------

def _raw(handle, inp, dt, null=None, **kw):
    """the entry itself with one argument nulled; (return code, message)"""
    n, m = inp["x0"].size, inp["y0"].size
    arg = dict(tol=1e-3, max_steps=500, ahead=1, ysync=0, loop=0)
    arg.update(kw)
    ins = [inp[k] for k in ("x0", "y0", "x_warm", "y_warm", "x_prev", "x12", "y12")]
    outs = [np.zeros(k, dt) for k in (n, m, n, m, m, n, n)] + [np.zeros(17), np.zeros(512), np.zeros(16, np.int32), np.zeros(1, np.int32)]
    ptrs = [a.ctypes.data for a in ins + outs]
    if null is not None:
        ptrs[null] = None
    rc = _lib.lib.PogsAmdSparseCgCheck(handle, *ptrs[:7], arg["tol"], arg["max_steps"], arg["ahead"], arg["ysync"],
                                       arg["loop"], *ptrs[7:])
    return rc, _lib.last_error()


@on(("900x400",))
def test_refusals_leave_the_handle_usable(ctx, monkeypatch):
    import pogs_amd

    inp = ctx.inputs()
    h = ctx.solver._h
    for kw, word in ((dict(ahead=0), "ahead"), (dict(max_steps=0), "max_steps"), (dict(loop=3), "loop"),
                     (dict(ysync=2), "ysync"), (dict(null=0), "null"), (dict(null=6), "null"), (dict(null=9), "null"),
                     (dict(null=15), "null"), (dict(null=17), "null")):
        rc, msg = _raw(h, inp, ctx.dt, **kw)
        assert rc == 6 and word in msg, (kw, rc, msg)
    # a dense handle; a handle whose copies are not tiled (loop 0 only)
    with pogs_amd.Solver(ctx.A.toarray(), dtype=ctx.dt) as dense:
        rc, msg = _raw(dense._h, inp, ctx.dt)
        assert rc == 6 and "sparse handle" in msg, msg
    with monkeypatch.context() as mp:
        mp.setenv("POGS_AMD_SPMV", "plain")
        plain = pogs_amd.Solver(ctx.A, dtype=ctx.dt)
    with plain:
        rc, msg = _raw(plain._h, inp, ctx.dt)
        assert rc == 6 and "tiled" in msg, msg
        assert _raw(plain._h, inp, ctx.dt, loop=1)[0] == 0
    f, g = _lasso(ctx)
    with pogs_amd.Solver(ctx.A, dtype=ctx.dt) as fresh:
        want = fresh.solve(f, g)
    got = ctx.solver.solve(f, g)
    assert same_bytes(got["x"], want["x"]) and got["iterations"] == want["iterations"]


@on(("900x400",))
def test_a_row_sharded_handle_is_refused(ctx, monkeypatch):
    import pogs_amd

    monkeypatch.setenv("POGS_AMD_TEST_TRANSPORT", "1")
    uid = (b"POGSLOCAL:" + os.urandom(8).hex().encode()).ljust(128, b"\0")
    inp = ctx.inputs()
    A = ctx.A.tocsr()
    half = ctx.m // 2
    seen, errors = [None, None], []

    def work(r):
        try:
            lo, hi_ = (0, half) if r == 0 else (half, ctx.m)
            with pogs_amd.Solver(A[lo:hi_], dtype=ctx.dt, dist=(r, 2, ctx.m, uid)) as s:
                part = dict(inp, y0=inp["y0"][lo:hi_], y_warm=inp["y_warm"][lo:hi_], y12=inp["y12"][lo:hi_])
                seen[r] = _raw(s._h, part, ctx.dt)
        except Exception as e:  # pragma: no cover - surfaced below
            errors.append((r, e))

    threads = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(600)
    assert not errors, errors
    for rc, msg in seen:
        assert rc == 6 and "row-sharded" in msg, (rc, msg)
