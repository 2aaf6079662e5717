"""The dense one-pass, device-resident CGLS projector (POGS_AMD_PROJ_CGLS_FUSED; csrc/dense_cg_fused.h: DcgQRowOp in
stream_rows_kernel DOT + ACC, dcg_step_a_kernel, cgf_step_b_kernel, cgf_close_kernel, DenseSolver::cg_loop_fused with its
enqueue-ahead and growing-chunk polling), through PogsAmdDenseCgCheck, Solver.project and full solves.

One projection against a model.  `cg_model` restates the loop's recurrence on A_eq (Solver.equilibrated()):
r = y0 - y_warm, x = x_warm - x0, s = A^T r - x, p = s, gamma = |s|^2 (no step if sqrt(gamma) < eps_T); per step q = A p,
t = A^T q, alpha = gamma / (|q|^2 + |p|^2), s -= alpha (t + p), x += alpha p, r -= alpha q, y += alpha q from y_warm,
beta = |s|^2 / gamma; stop when |s| <= |s_0| tol, or |x| tol >= 1, or at the cap, else p = s + beta p; at the end
x += x0.  It runs once in fp64 (fp32 handle) or long double (fp64 handle) and once with numpy in the handle's own type.
Yardstick of a vector: Y = max(|working-type model - high-precision model|_2, eps_T scale), scale = |x0| + |x_warm|
(n-sized) or |y0| + |y_warm| (m-sized) -- the floor is one rounding of the inputs, for the cases where the two models
happen to agree.  The device must be within FACTOR * Y of the high-precision model.  FACTOR: the next power of two above
the largest ratio measured over every case of this file (profiles/dense_cgls_fused_accuracy.txt), at most 8.  Every case
prints its ratios (pytest -s).

Stopping decisions do not depend on rounding: a case that needs the stop after exactly k steps takes the high-precision
model's |s_j| / |s_0| (clause 1) or |x_j| (clause 2), asserts a factor 2 between what must hold and what must not, and
puts tol at the geometric mean.

Shapes: (203, 33) and (70, 257) ragged last tiles, (33, 203) wide, (1500, 1300) another streaming shape with several
blocks in every launch, (33, 40001) fp32 windowed (rows wider than one register tile: two reads of A per step).

Pass count (the point of the projector).  One projection by the recurrence: 1 (A^T r at the start) + steps; with the
explicit product y = A x one more.  A full solve: matvecs - cg_iters = iterations (the start product of each projection)
+ ceil(iterations / 16) (the product y = A x of every POGS_AMD_YSYNC-th iteration, default 16, counted from 0)
+ exact_iters (one pass each for the exact residuals).  On a windowed plan a step reads A twice."""
import numpy as np
import pytest

import oracle_binding as ob
from helpers import hi, relerr, same_bytes, soa
from pogs_amd import _lib

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
VEC_KEYS = ("x", "y_new", "r", "p", "s")
M_SIZED = ("y_new", "r")
FACTOR = 2.0
PLAIN = [(203, 33), (70, 257), (33, 203), (1500, 1300)]
WINDOWED = (33, 40001)


def tname(dt):
    return "fp32" if dt == np.float32 else "fp64"


def report(line):
    print("dense_cgls_fused: " + line)


def _pogs():
    import pogs_amd
    return pogs_amd


def matrix(m, n, seed, dt):
    from pogs_amd import synth
    return synth.dense_lasso(m, n, seed=seed, dtype=dt)


def ill_matrix(m, n, seed):
    """squared singular values 0.93^j, columns scaled over five decades.  The equilibration takes the column scales out
    and normalises |A_eq|_F^2 to min(m, n), so the largest eigenvalue of A_eq^T A_eq is about 0.07 min(m, n) with the
    others spread densely below it: at 1700 x 1500 I + A^T A has a condition number near 100 and CGLS needs more than
    40 steps to bring |s| / |s_0| to the rounding level of fp32"""
    rng = np.random.default_rng(seed)
    k = min(m, n)
    U, _ = np.linalg.qr(rng.standard_normal((m, k)))
    V, _ = np.linalg.qr(rng.standard_normal((n, k)))
    A = (U * np.sqrt(0.93 ** np.arange(k))) @ V.T
    return A * np.exp(rng.uniform(np.log(1e-2), np.log(1e3), n))


# ---- the model ---------------------------------------------------------------------------------------------------

def cg_model(A, inp, tol, max_steps, dt, eps):
    c = lambda v: np.asarray(v).astype(dt)   # noqa: E731
    A = c(A)
    At = np.ascontiguousarray(A.T)
    x0, y0, xw, yw = (c(inp[k]) for k in ("x0", "y0", "x_warm", "y_warm"))
    sq = lambda v: np.sum(v * v, dtype=dt)   # noqa: E731
    tol = dt(tol)
    r, x = y0 - yw, xw - x0
    s = At @ r - x
    p = s.copy()
    gamma = sq(s)
    out = dict(steps=0, ratios=[], xnorms=[])
    y = yw.copy()
    if not np.sqrt(gamma) < dt(eps):
        norms0 = np.sqrt(gamma)
        for k in range(max_steps):
            q = A @ p
            t = At @ q
            alpha = gamma / (sq(q) + sq(p))
            s = s - alpha * (t + p)
            x = x + alpha * p
            r = r - alpha * q
            y = y + alpha * q
            s2, x2 = sq(s), sq(x)
            beta = s2 / gamma
            gamma = s2
            out["steps"] = k + 1
            out["ratios"].append(np.sqrt(s2) / norms0)
            out["xnorms"].append(np.sqrt(x2))
            if np.sqrt(s2) <= norms0 * tol or np.sqrt(x2) * tol >= 1 or k + 1 >= max_steps:
                break
            p = s + beta * p
    xn = x + x0
    out.update(x=xn, y_new=y, r=r, p=p, s=s, y_prod=A @ xn)
    return out


def predict_enqueued(ahead, steps, max_steps):
    """the poll rule: min(ahead, max_steps) steps, then chunks of 1, 2, 4, ... (at most 64) until the loop has ended"""
    enq = max(1, min(ahead, max_steps))
    more = 1
    while enq < steps:
        enq += min(more, max_steps - enq)
        more = min(2 * more, 64)
    return enq


# ---- one handle per matrix and type --------------------------------------------------------------------------------

class Ctx:
    def __init__(self, key, dt):
        pogs = _pogs()
        self.key, self.dt, self.eps = key, dt, float(np.finfo(dt).eps)
        kind, m, n = key
        self.m, self.n = m, n
        A = ill_matrix(m, n, 5).astype(dt) if kind == "ill" else matrix(m, n, 23, dt)[0]
        self.solver = pogs.Solver(A, dtype=dt, projector=_lib.PROJ_CGLS_FUSED)
        self.Aeq = self.solver.equilibrated()[0]
        self.hi = hi(np.zeros(1, dt)).dtype.type
        self.windowed = n > 32768
        # the wide windowed matrix converges by two decades per step: its third step is at the rounding level of s, and
        # |x_1| is small against the inputs
        self.k_stop, self.big = (2, 1e5) if self.windowed else (3, 1e3)
        self._inputs, self._models = {}, {}

    def inputs(self, seed=0, scale=1.0):
        """x0, y0, x_warm, y_warm (= A x_warm rounded to the type, as inside a solve) with |x0| + |x_warm| = scale"""
        key = (seed, scale)
        if key not in self._inputs:
            rng = np.random.default_rng(100 + seed)
            g = {k: rng.standard_normal(self.n) for k in ("x0", "x_warm")}
            g["y0"] = rng.standard_normal(self.m)
            c = scale / (np.linalg.norm(g["x0"]) + np.linalg.norm(g["x_warm"]))
            g = {k: (c * v).astype(self.dt) for k, v in g.items()}
            g["y_warm"] = (hi(self.Aeq) @ hi(g["x_warm"])).astype(self.dt)
            self._inputs[key] = g
        return self._inputs[key]

    def models(self, inp_key, inp, tol, max_steps):
        key = (inp_key, float(tol), max_steps)
        if key not in self._models:
            self._models[key] = (cg_model(self.Aeq, inp, tol, max_steps, self.hi, self.eps),
                                 cg_model(self.Aeq, inp, tol, max_steps, self.dt, self.eps))
        return self._models[key]

    def run(self, inp, tol, **kw):
        return _lib.dense_cg_check(self.solver._h, inp["x0"], inp["y0"], inp["x_warm"], inp["y_warm"], tol, **kw)

    def stop_tol(self, inp_key, inp, k):
        """tol that stops the loop after exactly k steps by the first clause, whatever the rounding"""
        ref = self.models(inp_key, inp, 0.0, k)[0]
        ratios = ref["ratios"]
        assert len(ratios) == k
        prev = ratios[k - 2] if k >= 2 else self.hi(1)
        assert prev / ratios[k - 1] >= 2, (self.key, k, [float(v) for v in ratios])
        assert all(ratios[j - 1] / ratios[j] > 1 for j in range(1, k)), [float(v) for v in ratios]
        assert ratios[k - 1] >= 100 * self.eps
        tol = float(np.sqrt(prev * ratios[k - 1]))
        assert all(float(v) * tol <= 0.5 for v in ref["xnorms"])
        return tol


_CTX = {}


def get_ctx(key, dt):
    if (key, dt) not in _CTX:
        _CTX[(key, dt)] = Ctx(key, dt)
    return _CTX[(key, dt)]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for c in _CTX.values():
        c.solver.close()
    _CTX.clear()


CASES = [(("syn",) + s, d) for s in PLAIN for d in DTYPES] + [(("syn",) + WINDOWED, np.float32)]


def on(cases):
    return pytest.mark.parametrize("ctx", cases, indirect=True,
                                   ids=lambda p: "%s%dx%d-%s" % (p[0][0] if p[0][0] != "syn" else "", p[0][1], p[0][2], tname(p[1])))


@pytest.fixture
def ctx(request):
    return get_ctx(*request.param)


def compare(ctx, case, out, ref, work, inp, ysync=False):
    """every vector of the entry within FACTOR yardsticks of the high-precision model; returns the largest ratio"""
    worst = 0.0
    sx = float(np.linalg.norm(hi(inp["x0"])) + np.linalg.norm(hi(inp["x_warm"])))
    sy = float(np.linalg.norm(hi(inp["y0"])) + np.linalg.norm(hi(inp["y_warm"])))
    lines = []
    for k in VEC_KEYS:
        mk = "y_prod" if (k == "y_new" and ysync) else k
        want, wk = ref[mk], work[mk]
        assert np.all(np.isfinite(out[k])), k
        yard = max(float(np.linalg.norm(hi(wk) - want)), ctx.eps * (sy if k in M_SIZED else sx))
        err = float(np.linalg.norm(hi(out[k]) - want))
        lines.append((k, err / yard))
        worst = max(worst, err / yard)
    report("%dx%d %s %-14s steps %3d  ratios %s" % (ctx.m, ctx.n, tname(ctx.dt), case, out["steps"],
                                                   " ".join("%s %.2f" % kv for kv in lines)))
    for k, ratio in lines:
        assert ratio <= FACTOR, (case, k, ratio)
    return worst


# ---- one projection ------------------------------------------------------------------------------------------------

@on(CASES)
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_capped_projection_matches_the_model(ctx, cap):
    inp = ctx.inputs()
    ref, work = ctx.models(0, inp, 0.0, cap)
    out = ctx.run(inp, 0.0, max_steps=cap, ahead=1)
    assert out["steps"] == cap == ref["steps"] and out["done"] == 1.0
    compare(ctx, "cap %d" % cap, out, ref, work, inp)
    # the pass count: A^T r at the start, then one launch over A per step (two on a windowed plan)
    assert out["matvecs"] == 1 + (2 if ctx.windowed else 1) * cap


@on(CASES)
def test_stop_by_the_residual_clause_and_the_poll_rule(ctx):
    """|s_k| <= |s_0| tol after exactly k steps; ahead = 1, k, k + 5, 64 give the same bytes and the predicted enqueues"""
    inp = ctx.inputs()
    k = ctx.k_stop
    tol = ctx.stop_tol(0, inp, k)
    ref, work = ctx.models(0, inp, tol, 500)
    assert ref["steps"] == k == work["steps"]
    first = None
    for ahead in (1, k, k + 5, 64):
        out = ctx.run(inp, tol, max_steps=500, ahead=ahead)
        assert out["steps"] == k and out["done"] == 1.0
        assert out["enqueued"] == predict_enqueued(ahead, k, 500), (ahead, out["enqueued"])
        assert out["matvecs"] == 1 + (2 if ctx.windowed else 1) * k
        if first is None:
            first = out
            compare(ctx, "stop %d" % k, out, ref, work, inp)
        else:
            for key in VEC_KEYS:
                assert same_bytes(out[key], first[key]), (ahead, key)
            for key in _lib.CG_SLOTS:
                assert out[key] == first[key] or (np.isnan(out[key]) and np.isnan(first[key])), (ahead, key)


@on(CASES)
def test_stop_by_the_solution_clause(ctx):
    """|x_1| tol >= 1 while |s_1| > |s_0| tol: one step, ended by the second clause alone"""
    inp = ctx.inputs(scale=ctx.big)
    probe = ctx.models(("big", 0), inp, 0.0, 1)[0]
    lo, hi_ = 1.0 / float(probe["xnorms"][0]), float(probe["ratios"][0])
    assert hi_ / lo >= 4, (lo, hi_)
    tol = float(np.sqrt(lo * hi_))
    ref, work = ctx.models(("big", 0), inp, tol, 500)
    assert ref["steps"] == 1 == work["steps"]
    out = ctx.run(inp, tol, max_steps=500, ahead=2)
    assert out["steps"] == 1 and out["enqueued"] == 2
    assert np.sqrt(out["x2"]) * tol >= 1 and np.sqrt(out["s2"]) > np.sqrt(out["norms0"]) * tol
    compare(ctx, "x clause", out, ref, work, inp)


@on(CASES)
def test_y_by_the_product(ctx):
    inp = ctx.inputs()
    k = ctx.k_stop
    tol = ctx.stop_tol(0, inp, k)
    ref, work = ctx.models(0, inp, tol, 500)
    out = ctx.run(inp, tol, max_steps=500, ahead=k, ysync=True)
    assert out["steps"] == k
    compare(ctx, "ysync", out, ref, work, inp, ysync=True)
    assert out["matvecs"] == 2 + (2 if ctx.windowed else 1) * k
    rec = ctx.run(inp, tol, max_steps=500, ahead=k)
    for key in ("x", "r", "p", "s"):
        assert same_bytes(out[key], rec[key]), key


def test_zero_steps_when_the_start_is_the_projection():
    """s_0 = 0: the loop ends in its first launch 2, x = x_warm, y = y_warm"""
    ctx = get_ctx(("syn", 203, 33), np.float32)
    z = np.zeros(ctx.n, ctx.dt), np.zeros(ctx.m, ctx.dt)
    out = _lib.dense_cg_check(ctx.solver._h, z[0], z[1], z[0], z[1], 1e-3, ahead=2)
    assert out["steps"] == 0 and out["done"] == 1.0 and out["matvecs"] == 1
    assert not out["x"].any() and not out["y_new"].any()


ILL = [(("ill", 1700, 1500), np.float32)]


@on(ILL)
def test_ill_conditioned_matrix_over_forty_steps(ctx):
    """48 steps at the cap.  Both models say that |s_40| / |s_0| is still 100 eps or more: a solve in fp32 that asks for
    the rounding level of s needs these steps.  The recurrence of s runs over all 48 without a resynchronisation: the drift
    stays inside the bar (the ratios are in profiles/dense_cgls_fused_accuracy.txt)."""
    inp = ctx.inputs()
    ref, work = ctx.models(0, inp, 0.0, 48)
    assert ref["steps"] == 48 and ref["ratios"][39] >= 100 * ctx.eps and work["ratios"][39] >= 100 * ctx.eps
    out = ctx.run(inp, 0.0, max_steps=48, ahead=48)
    assert out["steps"] == 48 and out["enqueued"] == 48 and out["matvecs"] == 49
    compare(ctx, "ill 48", out, ref, work, inp)


def test_other_handles_are_refused():
    pogs = _pogs()
    sp = pytest.importorskip("scipy.sparse")
    A = matrix(60, 20, 3, np.float32)[0]
    x, y = np.zeros(20, np.float32), np.zeros(60, np.float32)
    for kw in (dict(projector=_lib.PROJ_CGLS), dict()):
        with pogs.Solver(A, dtype=np.float32, **kw) as s:
            with pytest.raises(RuntimeError, match="POGS_AMD_PROJ_CGLS_FUSED"):
                _lib.dense_cg_check(s._h, x, y, x, y, 1e-3)
    with pogs.Solver(sp.csr_matrix(A), dtype=np.float32) as s:
        with pytest.raises(RuntimeError, match="POGS_AMD_PROJ_CGLS_FUSED"):
            _lib.dense_cg_check(s._h, x, y, x, y, 1e-3)
    uid = b"POGSLOCAL:0".ljust(128, b"\0")
    with pytest.raises(RuntimeError, match="single-GPU"):
        pogs.Solver(A, dtype=np.float32, projector=_lib.PROJ_CGLS_FUSED, dist=(0, 2, 120, uid))


# ---- Solver.project ------------------------------------------------------------------------------------------------

def _tol(dtype, t64, t32):
    return t64 if dtype == np.float64 else t32


@on(CASES)
def test_project_kkt(ctx):
    """the two residual expressions and the bounds of test_dense_cgls_projector_option (tests/test_gpu_dense.py)"""
    m, n, dtype = ctx.m, ctx.n, ctx.dt
    rng = np.random.default_rng(1)
    x0, y0 = rng.standard_normal(n), rng.standard_normal(m)
    x, y = ctx.solver.project(x0, y0, tol=_tol(dtype, 1e-10, 1e-6))
    A64 = ctx.Aeq.astype(np.float64)
    eps = _tol(dtype, 1e-8, 3e-4)
    r1 = np.linalg.norm(A64 @ x - y) / np.sqrt(m)
    r2 = np.linalg.norm(A64.T @ (A64 @ x.astype(np.float64) - y0) + (x - x0)) / np.sqrt(n)
    report("%dx%d %s project: |A x - y| %.2e  KKT %.2e  (bound %.0e)" % (m, n, tname(dtype), r1, r2, eps))
    assert r1 < eps
    assert r2 < eps


# ---- full solves ---------------------------------------------------------------------------------------------------
# Instances.  lasso: synth.dense_lasso with lambda 0.1, the recipe of test_dense_cgls_projector_option.  Its seed is, per
# shape, the first from 23 (that test's) upward at which the REFERENCE is a yardstick for a CGLS implementation in fp32:
# the fp32 oracle with CGLS converges and its iteration count lies within max(3, 10 %) of the fp32 oracle's with the
# direct projector -- the acceptance window, applied to the reference against itself.  Where the oracle's own inexact
# projection triples its count (203 x 33, seed 23: 142 iterations with CGLS, 47 direct, 41 in fp64) the count says nothing
# about another implementation of the loop.  The rule looks at the oracle alone (CPU); the test asserts it for the seed
# it uses.  203 x 33: seed 24 (47 / 47); 70 x 257 and 33 x 203: seed 23 (629 / 628, 851 / 804).  At 1500 x 1300 with
# lambda 0.1 the fp32 oracle with CGLS converges at none of the seeds 23 .. 26 (2499 iterations each), and the fallback
# of the acceptance (x against the direct oracle's) has no footing there either: in fp64 the oracle's own CGLS and direct
# solutions of seed 23 lie 1.3e-3 apart (m / n = 1.15: 1209 of 1300 entries non-zero, the optimum is flat at the
# default tolerances), more than the 3e-4 allowed.  That shape takes lambda 1 with seed 23, where the rule holds (96 / 95
# iterations; the two fp64 solutions 9e-5 apart).  logistic:
# synth.dense_logistic with logit_std 2 and lambda 1 -- at lambda 0.01 the 1500 x 1300 instance is nearly separable and
# the reference algorithm itself, with its exact projector, runs into max_iter in both precisions (the oracle returns
# status 3), so there would be nothing to compare with; at lambda 1 the direct oracle converges in about 100 iterations.
# The warm solves start from the reference's own cold solution (x, l), so that their reference is computed once too.
# The same rule holds for the start: from it the fp32 oracle with CGLS must take a count within max(3, 10 %) of the fp32
# oracle's with the direct projector.  At lasso 1500 x 1300 it does not (183 against 4 from the solution itself, at the
# seeds 23 .. 26 alike; the fp64 oracle takes 3): that instance starts from HALF the reference's solution (x / 2, l / 2),
# where it does (90 / 89).  The test asserts the rule for the start it uses.

_ORACLE, _SOLVES = {}, {}
LASSO = {(203, 33): (24, 0.1), (1500, 1300): (23, 1.0)}   # (seed, lambda); every other shape: (23, 0.1)
WARM_SCALE = {("lasso", (1500, 1300)): 0.5}                # the warm start as a multiple of the reference's solution: 1


def _reference(A, f, g, dtype, **start):
    want = ob.oracle_solve(A, soa(f), soa(g), dtype=dtype, use_cgls=True, **start)
    if want["status"] != 0:
        direct = ob.oracle_solve(A, soa(f), soa(g), dtype=dtype, use_cgls=False, **start)
        assert direct["status"] == 0, "the reference algorithm does not solve this instance"
        want = dict(direct, iterations=None)
    return want


def oracle(shape, dtype, prob):
    """(A, f, g, reference of the cold solve, reference of the warm solve from its "start"); a reference is
    the oracle with CGLS where that converges, else the oracle with the direct projector (iterations None)"""
    key = (shape, dtype, prob)
    if key not in _ORACLE:
        from pogs_amd import synth
        pogs = _pogs()
        m, n = shape
        if prob == "lasso":
            seed, lambd = LASSO.get(shape, (23, 0.1))
            A, b, _ = matrix(m, n, seed, dtype)
            f, g = pogs.graph.lasso_functions(b, lambd, n)
        else:
            A, b, _ = synth.dense_logistic(m, n, seed=23, dtype=dtype, logit_std=2.0)
            f, g = pogs.graph.logistic_functions(b, 1.0, n)
        cold = _reference(A, f, g, dtype)
        if prob == "lasso" and dtype == np.float32:
            # the rule of the instance (above): the reference with CGLS against the reference with the direct projector
            assert cold["iterations"] is not None, "the fp32 oracle with CGLS does not converge on this instance"
            direct = ob.oracle_solve(A, soa(f), soa(g), dtype=dtype, use_cgls=False)
            assert direct["status"] == 0
            assert abs(cold["iterations"] - direct["iterations"]) <= max(3, int(0.1 * direct["iterations"])), \
                (shape, cold["iterations"], direct["iterations"])
        c = WARM_SCALE.get((prob, shape), 1.0)
        start = ((c * cold["x"]).astype(dtype), (c * cold["l"]).astype(dtype))
        warm = _reference(A, f, g, dtype, x0=start[0], l0=start[1])
        if dtype == np.float32 and warm["iterations"] is not None:
            direct = ob.oracle_solve(A, soa(f), soa(g), dtype=dtype, use_cgls=False, x0=start[0], l0=start[1])
            assert direct["status"] == 0
            assert abs(warm["iterations"] - direct["iterations"]) <= max(3, int(0.1 * direct["iterations"])), \
                (prob, shape, warm["iterations"], direct["iterations"])
        warm["start"] = start
        _ORACLE[key] = (A, f, g, cold, warm)
    return _ORACLE[key]


def solves(shape, dtype, prob):
    """every solve of one instance, run once: a PROJ_CGLS handle before any fused handle of the instance exists, the fused
    handle cold, a second PROJ_CGLS handle next to it, the fused handle again, and warm from the start of the warm reference"""
    key = (shape, dtype, prob)
    if key not in _SOLVES:
        pogs = _pogs()
        A, f, g, _, want_warm = oracle(shape, dtype, prob)
        r = {}
        with pogs.Solver(A, dtype=dtype, projector=_lib.PROJ_CGLS) as s:
            r["before"] = s.solve(f, g)
            r["st_cgls"] = s.stats()
        with pogs.Solver(A, dtype=dtype, projector=_lib.PROJ_CGLS_FUSED) as s:
            s.reset_stats()
            r["cold"] = s.solve(f, g)
            r["st"] = s.stats()
            with pogs.Solver(A, dtype=dtype, projector=_lib.PROJ_CGLS) as s2:
                r["beside"] = s2.solve(f, g)
            r["again"] = s.solve(f, g)
            s.warm_start(*want_warm["start"])
            r["warm"] = s.solve(f, g)
        _SOLVES[key] = r
    return _SOLVES[key]


def accept(got, want, dtype):
    """the acceptance of test_dense_cgls_projector_option"""
    assert got["status"] == 0
    if want["iterations"] is not None:
        assert abs(got["iterations"] - want["iterations"]) <= max(3, int(0.1 * want["iterations"]))
    assert relerr(got["x"], want["x"]) < _tol(dtype, 1e-5, 3e-4)


INSTANCES = [(p, s, d) for p in ("lasso", "logistic") for s in PLAIN for d in DTYPES]
instances = pytest.mark.parametrize("prob,shape,dtype", INSTANCES, ids=lambda v: v if isinstance(v, str) else
                                    ("%dx%d" % v if isinstance(v, tuple) else tname(v)))


@instances
def test_full_solve_against_the_oracle(prob, shape, dtype):
    """Cold, against oracle_solve(use_cgls=True) under the acceptance of test_dense_cgls_projector_option.

    Measured on an MI355X (each line also printed by the test): the fused handle follows the PROJ_CGLS handle's
    trajectory -- the same iteration count in every instance, and the oracle's within one iteration.  The fp32 oracle with
    CGLS is a poor reference on some instances of these shapes (it stalls or takes several times the iterations of its own
    fp64 run: SURVEY.md finding 5): the lasso instances are chosen by a rule on the oracle alone, see "Instances" above.
    The figures of every case are in profiles/dense_cgls_fused_accuracy.txt, section 3."""
    _, _, _, want, _ = oracle(shape, dtype, prob)
    r = solves(shape, dtype, prob)
    report("%s %dx%d %s cold: iterations %d (oracle %s, cgls %d), relerr x %.2e (cgls %.2e), status %d"
           % (prob, shape[0], shape[1], tname(dtype), r["cold"]["iterations"], want["iterations"], r["before"]["iterations"],
              relerr(r["cold"]["x"], want["x"]), relerr(r["before"]["x"], want["x"]), r["cold"]["status"]))
    accept(r["cold"], want, dtype)


@instances
def test_full_solve_after_warm_start_against_the_oracle(prob, shape, dtype):
    """After warm_start, against the oracle started from the same point ("Instances" above), under the same acceptance."""
    _, _, _, _, want_warm = oracle(shape, dtype, prob)
    r = solves(shape, dtype, prob)
    report("%s %dx%d %s warm: iterations %d (oracle %s), relerr x %.2e, status %d"
           % (prob, shape[0], shape[1], tname(dtype), r["warm"]["iterations"], want_warm["iterations"],
              relerr(r["warm"]["x"], want_warm["x"]), r["warm"]["status"]))
    accept(r["warm"], want_warm, dtype)


@instances
def test_full_solve_deterministic_pass_count_and_cgls_untouched(prob, shape, dtype):
    r = solves(shape, dtype, prob)
    st, st_cgls = r["st"], r["st_cgls"]
    iters = st["iterations"]
    report("%s %dx%d %s: passes / iteration %.2f (cgls %.2f), cg steps / iteration %.2f (cgls %.2f), iterations %d (cgls %d)"
           % (prob, shape[0], shape[1], tname(dtype), st["matvecs"] / iters, st_cgls["matvecs"] / st_cgls["iterations"],
              st["cg_iters"] / iters, st_cgls["cg_iters"] / st_cgls["iterations"], iters, st_cgls["iterations"]))
    # two runs of one solve: the same bytes; a PROJ_CGLS handle next to a fused one: the bytes it gives without one
    for k in ("x", "y", "l", "mu"):
        assert same_bytes(r["cold"][k], r["again"][k]), k
        assert same_bytes(r["before"][k], r["beside"][k]), k
    assert r["cold"]["iterations"] == r["again"]["iterations"] and r["before"]["iterations"] == r["beside"]["iterations"]
    # the pass count (module docstring)
    assert st["cg_iters"] > 0
    assert st["matvecs"] - st["cg_iters"] == iters + -(-iters // 16) + st["exact_iters"], st
    assert st_cgls["matvecs"] >= 2 * st_cgls["cg_iters"] > 0


def test_col_major_and_device_resident_matrix():
    pogs = _pogs()
    import torch

    m, n, dtype = 203, 33, np.float64
    A, f, g, want, _ = oracle((m, n), dtype, "lasso")
    with pogs.Solver(A, dtype=dtype, projector=_lib.PROJ_CGLS_FUSED) as s:
        ref = s.solve(f, g)
    with pogs.Solver(np.asfortranarray(A), dtype=dtype, order=pogs.Ordering.COL_MAJ, projector=_lib.PROJ_CGLS_FUSED) as s:
        col = s.solve(f, g)
    t = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    with pogs.Solver(t.data_ptr(), dtype=dtype, shape=(m, n), device_ptr=True, projector=_lib.PROJ_CGLS_FUSED) as s:
        dev = s.solve(f, g)
    for got in (col, dev):
        accept(got, want, dtype)
        assert got["iterations"] == ref["iterations"]
        assert same_bytes(got["x"], ref["x"])


def test_begin_run_iterate_and_mul():
    pogs = _pogs()
    m, n, dtype = 203, 33, np.float64
    A, f, g, want, _ = oracle((m, n), dtype, "lasso")
    with pogs.Solver(A, dtype=dtype, projector=_lib.PROJ_CGLS_FUSED) as s:
        s.begin_run(f, g)
        s.iterate(20)
        st = s.stats()
        assert st["cg_iters"] > 0 and st["matvecs"] > st["cg_iters"]
        A_eq = s.equilibrated()[0]
        v = np.arange(n, dtype=dtype) / n
        y = s.mul("n", 1.0, v, 0.0, np.zeros(m, dtype))
        assert relerr(y, A_eq.astype(np.float64) @ v) < 1e-12
        got = s.solve(f, g)
    accept(got, want, dtype)


# ---- refusals ------------------------------------------------------------------------------------------------------

def test_batch_entries_and_get_factor_refuse_and_the_handle_solves_afterwards():
    pogs = _pogs()
    m, n, dtype = 203, 33, np.float64
    A, f, g, want, _ = oracle((m, n), dtype, "lasso")
    with pogs.Solver(A, dtype=dtype, projector=_lib.PROJ_CGLS_FUSED) as s:
        first = s.solve(f, g)
        with pytest.raises(RuntimeError, match="CGLS"):
            s.solve_batch([f, f], [g, g])
        with pytest.raises(RuntimeError, match="CGLS"):
            s.solve_batch([f, f], [g, g], x0=np.zeros((2, n), dtype), l0=np.zeros((2, m), dtype))
        with pytest.raises(RuntimeError, match="CGLS"):
            s.factor()
        after = s.solve(f, g)
    accept(after, want, dtype)
    assert same_bytes(first["x"], after["x"]) and first["iterations"] == after["iterations"]


def test_verbose_line_names_the_projector(capfd):
    pogs = _pogs()
    A, f, g, _, _ = oracle((203, 33), np.float64, "lasso")
    with pogs.Solver(A, dtype=np.float64, projector=_lib.PROJ_CGLS_FUSED) as s:
        s.solve(f, g, verbose=1)
    assert "dense/cgls-fused" in capfd.readouterr().out
