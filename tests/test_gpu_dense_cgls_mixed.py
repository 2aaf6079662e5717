"""Mixed storage with the one-pass CGLS projector (PogsAmdCreateDenseMixed; Solver(A, dtype=float64, storage=float32,
projector=PROJ_CGLS_FUSED)): an fp64 PROJ_CGLS_FUSED handle whose equilibrated matrix is rounded to float32 once and
whose recurring launches -- A^T r at the start of a projection, the one pass of every CG step, the y-sync product --
read the float32 copy through stream_rows_mixed_kernel (csrc/stream_mixed.h, csrc/dense_cg_fused.h).

Instances: the lasso and logistic ones of test_gpu_dense_cgls_fused in fp64 at its four shapes (tall, wide, and 1500 x
1300 with several blocks in every launch), plus logistic at 40 x 10238 and 24 x 5122, whose rows take the 256 x 10 and
256 x 6 shapes of the mixed plan -- executed as 512 threads -- with n_pad % 4 == 2.  (Lasso with lambda 0.1 at those two
runs into max_iter on the reference itself, so there is nothing to compare with.)

  * the stored matrix is the float32 rounding of the plain fused handle's equilibrated matrix; d and e are its bytes;
  * one projection through PogsAmdDenseCgCheck against cg_model on the handle's OWN equilibrated matrix, under the
    factor of test_gpu_dense_cgls_fused.compare, with the pass count 1 + steps (+ 1 with the product);
  * cold solves against the oracle on the ORIGINAL A under that file's acceptance, and relerr(x) <= 10 x yard, yard the
    distance, measured here on the CPU, between the oracle's solutions for A and for float32(A) (the factor 10 is
    tests/test_gpu_mixed_storage.py's: the handle rounds the equilibrated entries, the yardstick the raw ones);
  * POGS_AMD_MIXED_PASS on against off: equal iteration counts, relerr(x) <= max(10 d_ref, 1e-15) with d_ref the plain
    fused handle's distance from the oracle (only summation orders differ);
  * counters: a second solve gives the same bytes, matvecs - cg_iters = iters + ceil(iters / 16) + exact_iters, and with
    profiling stream_bytes = m n (4 F + 8 D), F = iters + cg_iters + ceil(iters / 16) launches over floats and
    D = exact_iters over doubles (switch off: 8 m n per launch);
  * warm start, begin_run / iterate, mul, project (the KKT check of test_project_kkt); the batch entries and factor()
    refuse and the handle solves afterwards to the same bytes.
Every case prints its figures (pytest -s); profiles/dense_cgls_mixed_accuracy.txt is that table."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import oracle_binding as ob
from helpers import relerr, same_bytes, soa
from pogs_amd import _lib
from test_gpu_dense_cgls_fused import PLAIN, accept, cg_model, compare, matrix, oracle

pytestmark = pytest.mark.gpu
F64 = np.float64
WIDE_EXTRA = [(40, 10238), (24, 5122)]
INSTANCES = [(p, s) for p in ("lasso", "logistic") for s in PLAIN] + [("logistic", s) for s in WIDE_EXTRA]
instances = pytest.mark.parametrize("prob,shape", INSTANCES, ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
_SOLVES, _YARD = {}, {}


def report(line):
    print("dense_cgls_mixed: " + line)


def _pogs():
    import pogs_amd
    return pogs_amd


@contextmanager
def switch(value):
    """POGS_AMD_MIXED_PASS as a handle reads it at create; None: unset (the default, on)"""
    old = os.environ.pop("POGS_AMD_MIXED_PASS", None)
    if value is not None:
        os.environ["POGS_AMD_MIXED_PASS"] = value
    try:
        yield
    finally:
        os.environ.pop("POGS_AMD_MIXED_PASS", None)
        if old is not None:
            os.environ["POGS_AMD_MIXED_PASS"] = old


def mixed(A, sw=None, **kw):
    with switch(sw):
        return _pogs().Solver(A, dtype=F64, storage=np.float32, projector=_lib.PROJ_CGLS_FUSED, **kw)


def plain(A, **kw):
    return _pogs().Solver(A, dtype=F64, projector=_lib.PROJ_CGLS_FUSED, **kw)


def solves(prob, shape):
    """every solve of one instance, run once: the plain fused handle cold; the mixed handle (profiling on) cold, again and
    warm from the warm reference's start; the mixed handle with the switch off cold"""
    key = (prob, shape)
    if key not in _SOLVES:
        A, f, g, _, want_warm = oracle(shape, F64, prob)
        r = {}
        with plain(A) as s:
            r["plain"] = s.solve(f, g)
        with mixed(A, profile=True) as s:
            assert s.storage == _pogs().STORE_F32
            s.reset_stats()
            r["on"] = s.solve(f, g)
            r["st_on"] = s.stats()
            r["again"] = s.solve(f, g)
            s.warm_start(*want_warm["start"])
            r["warm"] = s.solve(f, g)
        with mixed(A, sw="0", profile=True) as s:
            s.reset_stats()
            r["off"] = s.solve(f, g)
            r["st_off"] = s.stats()
        _SOLVES[key] = r
    return _SOLVES[key]


def yardstick(prob, shape):
    """relerr(x) between the oracle's solutions for A and for float32(A), both with CGLS in fp64 (CPU)"""
    key = (prob, shape)
    if key not in _YARD:
        A, f, g, want, _ = oracle(shape, F64, prob)
        A32 = A.astype(np.float32).astype(F64)
        assert not np.array_equal(A32, A)
        rounded = ob.oracle_solve(A32, soa(f), soa(g), dtype=F64, use_cgls=True)
        assert rounded["status"] == 0 and want["iterations"] is not None
        assert rounded["iterations"] == want["iterations"], (rounded["iterations"], want["iterations"])
        _YARD[key] = relerr(rounded["x"], want["x"])
        assert _YARD[key] > 0
    return _YARD[key]


# ---- the stored matrix ---------------------------------------------------------------------------------------------

SHAPES = PLAIN + WIDE_EXTRA
shapes = pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)


@shapes
def test_the_stored_matrix_is_the_rounded_equilibrated_matrix(shape):
    A = matrix(shape[0], shape[1], 23, F64)[0]
    with plain(A) as s:
        Ap, dp, ep, _ = s.equilibrated()
    for sw in (None, "0"):
        with mixed(A, sw=sw) as s:
            Am, dm, em, nrm = s.equilibrated()
        assert np.array_equal(Am.astype(np.float32).astype(F64), Am)          # survives a float round trip
        assert np.array_equal(Am, Ap.astype(np.float32).astype(F64))          # the plain handle's, rounded
        assert np.all(np.abs(Am - Ap) <= 2.0 ** -24 * np.abs(Ap))
        assert not np.array_equal(Am, Ap)
        assert same_bytes(dm, dp) and same_bytes(em, ep) and np.isfinite(nrm) and nrm > 0


# ---- one projection ------------------------------------------------------------------------------------------------

class Ctx:
    """what test_gpu_dense_cgls_fused.compare and its model need of a handle"""

    def __init__(self, shape):
        self.m, self.n = shape
        self.dt, self.eps, self.hi = F64, float(np.finfo(F64).eps), np.longdouble
        self.solver = mixed(matrix(shape[0], shape[1], 23, F64)[0])
        self.Aeq = self.solver.equilibrated()[0]
        rng = np.random.default_rng(100)
        g = {k: rng.standard_normal(self.n) for k in ("x0", "x_warm")}
        g["y0"] = rng.standard_normal(self.m)
        c = 1.0 / (np.linalg.norm(g["x0"]) + np.linalg.norm(g["x_warm"]))
        self.inp = {k: c * v for k, v in g.items()}
        self.inp["y_warm"] = (self.Aeq.astype(np.longdouble) @ self.inp["x_warm"].astype(np.longdouble)).astype(F64)

    def models(self, tol, max_steps):
        return (cg_model(self.Aeq, self.inp, tol, max_steps, self.hi, self.eps),
                cg_model(self.Aeq, self.inp, tol, max_steps, self.dt, self.eps))

    def run(self, tol, **kw):
        i = self.inp
        return _lib.dense_cg_check(self.solver._h, i["x0"], i["y0"], i["x_warm"], i["y_warm"], tol, **kw)


_CTX = {}


@pytest.fixture
def ctx(request):
    if request.param not in _CTX:
        _CTX[request.param] = Ctx(request.param)
    return _CTX[request.param]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for c in _CTX.values():
        c.solver.close()
    _CTX.clear()


on_shapes = pytest.mark.parametrize("ctx", SHAPES, indirect=True, ids=lambda s: "%dx%d" % s)


@on_shapes
def test_one_projection_matches_the_model_on_the_handles_own_matrix(ctx):
    for cap in (1, 2, 3):
        ref, work = ctx.models(0.0, cap)
        out = ctx.run(0.0, max_steps=cap, ahead=1)
        assert out["steps"] == cap == ref["steps"] and out["done"] == 1.0 and out["matvecs"] == 1 + cap
        compare(ctx, "cap %d" % cap, out, ref, work, ctx.inp)
    # to the residual stop after k steps, the tol at the geometric mean of the model's ratios around it
    # (k: 3, or fewer where the model says that |s_3| / |s_0| is already at the rounding level -- the very wide shapes
    #  converge by several decades per step; the choice looks at the high-precision model alone)
    ratios = [np.longdouble(1)] + list(ctx.models(0.0, 3)[0]["ratios"])
    k = max(j for j in (1, 2, 3) if ratios[j] >= 100 * ctx.eps)
    assert ratios[k - 1] / ratios[k] >= 2 and ratios[k] >= 100 * ctx.eps, [float(v) for v in ratios]
    tol = float(np.sqrt(ratios[k - 1] * ratios[k]))
    ref, work = ctx.models(tol, 500)
    assert ref["steps"] == k == work["steps"]
    first = None
    for ahead in (1, k, k + 5, 64):
        out = ctx.run(tol, max_steps=500, ahead=ahead)
        assert out["steps"] == k and out["done"] == 1.0 and out["matvecs"] == 1 + k
        if first is None:
            first = out
            compare(ctx, "stop %d" % k, out, ref, work, ctx.inp)
        else:
            assert all(same_bytes(out[key], first[key]) for key in ("x", "y_new", "r", "p", "s")), ahead
    out = ctx.run(tol, max_steps=500, ahead=k, ysync=True)
    assert out["steps"] == k and out["matvecs"] == 2 + k
    compare(ctx, "ysync", out, ref, work, ctx.inp, ysync=True)
    assert all(same_bytes(out[key], first[key]) for key in ("x", "r", "p", "s"))


@on_shapes
def test_project_kkt_mul_and_the_refusals(ctx):
    """the two residual expressions and the fp64 bounds of test_gpu_dense_cgls_fused.test_project_kkt"""
    m, n = ctx.m, ctx.n
    rng = np.random.default_rng(1)
    x0, y0 = rng.standard_normal(n), rng.standard_normal(m)
    x, y = ctx.solver.project(x0, y0, tol=1e-10)
    r1 = np.linalg.norm(ctx.Aeq @ x - y) / np.sqrt(m)
    r2 = np.linalg.norm(ctx.Aeq.T @ (ctx.Aeq @ x - y0) + (x - x0)) / np.sqrt(n)
    report("%dx%d project: |A x - y| %.2e  KKT %.2e  (bound 1e-08)" % (m, n, r1, r2))
    assert r1 < 1e-8 and r2 < 1e-8
    v = np.arange(n, dtype=F64) / n
    assert relerr(ctx.solver.mul("n", 1.0, v, 0.0, np.zeros(m)), ctx.Aeq @ v) < 1e-12
    w = np.arange(m, dtype=F64) / m
    assert relerr(ctx.solver.mul("t", 1.0, w, 0.0, np.zeros(n)), ctx.Aeq.T @ w) < 1e-12


# ---- full solves ---------------------------------------------------------------------------------------------------

@instances
def test_cold_solve_against_the_oracle_on_the_original_matrix(prob, shape):
    _, _, _, want, _ = oracle(shape, F64, prob)
    r, yard = solves(prob, shape), yardstick(prob, shape)
    d_on, d_ref = relerr(r["on"]["x"], want["x"]), relerr(r["plain"]["x"], want["x"])
    d_switch = relerr(r["on"]["x"], r["off"]["x"])
    report("%-8s %5d x %-5d iterations %4d (oracle %s, plain %d, off %d)  mixed-oracle %.3e  plain-oracle %.3e  yardstick(A, float(A)) %.3e"
           "  switch on-off %.3e" % (prob, shape[0], shape[1], r["on"]["iterations"], want["iterations"], r["plain"]["iterations"],
                                     r["off"]["iterations"], d_on, d_ref, yard, d_switch))
    accept(r["on"], want, F64)
    assert d_on <= 10 * yard
    # the switch: the same rounded problem, other summation orders
    assert r["on"]["iterations"] == r["off"]["iterations"]
    assert d_switch <= max(10 * d_ref, 1e-15)


@instances
def test_warm_solve_against_the_oracle(prob, shape):
    _, _, _, _, want_warm = oracle(shape, F64, prob)
    r = solves(prob, shape)
    report("%-8s %5d x %-5d warm: iterations %d (oracle %s), relerr x %.2e" % (prob, shape[0], shape[1], r["warm"]["iterations"],
                                                                            want_warm["iterations"], relerr(r["warm"]["x"], want_warm["x"])))
    accept(r["warm"], want_warm, F64)


@instances
def test_counters_and_determinism(prob, shape):
    m, n = shape
    r = solves(prob, shape)
    for k in ("x", "y", "l", "mu"):
        assert same_bytes(r["on"][k], r["again"][k]), k
    assert r["on"]["iterations"] == r["again"]["iterations"]
    for st, per in ((r["st_on"], 4), (r["st_off"], 8)):
        iters = st["iterations"]
        ysyncs = -(-iters // 16)
        assert st["cg_iters"] > 0
        assert st["matvecs"] - st["cg_iters"] == iters + ysyncs + st["exact_iters"], st
        F, D = iters + st["cg_iters"] + ysyncs, st["exact_iters"]
        assert st["stream_launches"] == F + D, st
        assert st["stream_bytes"] == float(m) * n * (per * F + 8 * D), st
    report("%-8s %5d x %-5d passes / iteration %.2f, cg steps / iteration %.2f, float launches %d, fp64 launches %d"
           % (prob, m, n, r["st_on"]["matvecs"] / r["st_on"]["iterations"], r["st_on"]["cg_iters"] / r["st_on"]["iterations"],
              r["st_on"]["stream_launches"] - r["st_on"]["exact_iters"], r["st_on"]["exact_iters"]))


def test_begin_run_iterate_device_pointer_and_col_major():
    import torch

    m, n = 33, 203
    A, f, g, want, _ = oracle((m, n), F64, "lasso")
    ref = solves("lasso", (m, n))["on"]
    with mixed(A) as s:
        s.begin_run(f, g)
        s.iterate(20)
        st = s.stats()
        assert st["cg_iters"] > 0 and st["matvecs"] > st["cg_iters"]
        got = s.solve(f, g)
    accept(got, want, F64)
    assert same_bytes(got["x"], ref["x"])
    t = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    with switch(None):
        with _pogs().Solver(t.data_ptr(), dtype=F64, shape=(m, n), device_ptr=True, storage=np.float32,
                            projector=_lib.PROJ_CGLS_FUSED) as s:
            dev = s.solve(f, g)
        with _pogs().Solver(np.asfortranarray(A), dtype=F64, order=_pogs().Ordering.COL_MAJ, storage=np.float32,
                            projector=_lib.PROJ_CGLS_FUSED) as s:
            col = s.solve(f, g)
    for other in (dev, col):
        assert other["iterations"] == ref["iterations"] and same_bytes(other["x"], ref["x"])


def test_batch_entries_and_factor_refuse_and_the_handle_solves_afterwards():
    m, n = 70, 257
    A, f, g, want, _ = oracle((m, n), F64, "lasso")
    with mixed(A) as s:
        first = s.solve(f, g)
        with pytest.raises(RuntimeError, match="CGLS"):
            s.solve_batch([f, f], [g, g])
        with pytest.raises(RuntimeError, match="CGLS"):
            s.solve_batch([f, f], [g, g], x0=np.zeros((2, n)), l0=np.zeros((2, m)))
        with pytest.raises(RuntimeError, match="CGLS"):
            s.factor()
        after = s.solve(f, g)
    accept(after, want, F64)
    assert same_bytes(first["x"], after["x"]) and first["iterations"] == after["iterations"]
