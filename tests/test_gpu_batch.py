"""GPU tests of batched solves (Solver.solve_batch / PogsAmdSolveBatchFn): k problems on one handle's matrix with every
pass over A shared.  Each member is checked against its own oracle solve, and a member's bytes must not depend on the
other members of its batch or on its slot (the multi-vector products are per-column MFMA chains and every partial sum
runs in a fixed order)."""
import ctypes
import time

import numpy as np
import pytest

import oracle_binding as ob
from helpers import PROBLEMS, fn_arrays, objective, relerr, soa

pytestmark = pytest.mark.gpu


def _pogs():
    import pogs_amd

    return pogs_amd


def _tol(dtype, f64, f32):
    return f64 if dtype == np.float64 else f32


def _check(A, f, g, got, want, dtype, tight):
    """The bars of test_gpu_dense._check_solution, restated: same status; iterations within 2 (tight, fp64) or
    max(3, 10 %); ||dx||/||x|| and ||dy||/||y|| < 1e-6 (tight) / 1e-4 (fp32: _xtol32 of the two iteration counts,
    the suite's fp32 bar against the oracle); the dual within 10x that on the scale of y;
    optval within 1e-7 (tight) / 1e-4 relative (fp32: the same _xtol32); optval equal to sum f(y) + sum g(x) recomputed in numpy; and the true
    objective at x within 5 % of optval."""
    from helpers import _fsum

    assert got["status"] == want["status"]
    it_g, it_w = got["iterations"], want["iterations"]
    if want["status"] != 0:
        assert it_g == it_w
        return
    slack = 2 if tight else max(3, int(0.1 * it_w))
    assert abs(it_g - it_w) <= slack, (it_g, it_w)
    xtol = 1e-6 if tight else (1e-4 if dtype == np.float64 else _xtol32(it_g, it_w))
    assert relerr(got["x"], want["x"]) < xtol
    assert relerr(got["y"], want["y"]) < xtol
    l_scale = max(np.linalg.norm(want["l"]), 1e-2 * np.linalg.norm(want["y"]))
    assert np.linalg.norm(got["l"].astype(np.float64) - want["l"]) / l_scale < 10 * xtol
    otol = 1e-7 if tight else (1e-4 if dtype == np.float64 else _xtol32(it_g, it_w))
    assert got["optval"] == pytest.approx(want["optval"], rel=otol, abs=1e-9 if tight else 1e-6)
    obj = _fsum(f, got["y"].astype(np.float64)) + _fsum(g, got["x"].astype(np.float64))
    assert obj == pytest.approx(got["optval"], rel=_tol(dtype, 1e-9, 1e-4), abs=_tol(dtype, 1e-9, 1e-4))
    true_obj = objective(np.asarray(A, np.float64), f, g, got["x"].astype(np.float64))
    assert true_obj == pytest.approx(got["optval"], rel=0.05, abs=1e-2)


def _xtol32(got_iters, want_iters, loose=2e-4):
    """test_gpu_dense._xtol32: 2e-5 at the same iteration count, else 1e-4 per iteration apart, capped at 2e-4."""
    d = abs(int(got_iters) - int(want_iters))
    return 2e-5 if d == 0 else min(loose, 1e-4 * (1 + d))


def _problem_200x100():
    rng = np.random.default_rng(7)
    m, n = 200, 100
    A = rng.standard_normal((m, n))
    b = A @ (rng.standard_normal(n) * (rng.random(n) < 0.2)) + 0.1 * rng.standard_normal(m)
    return A, b


def _same_bytes(r1, r2):
    for k in ("x", "y", "l", "mu"):
        assert r1[k].tobytes() == r2[k].tobytes(), k
    assert np.float64(r1["optval"]).tobytes() == np.float64(r2["optval"]).tobytes()
    assert r1["iterations"] == r2["iterations"] and r1["status"] == r2["status"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_families_200x100(dtype):
    pogs = _pogs()
    A, b = _problem_200x100()
    n = A.shape[1]
    names = list(PROBLEMS)
    fgs = [PROBLEMS[p](b, n) for p in names]
    with pogs.Solver(A, dtype=dtype) as s:
        got = s.solve_batch([fg[0] for fg in fgs], [fg[1] for fg in fgs])
        solo = [s.solve(f, g) for f, g in fgs] if dtype == np.float64 else None
    assert len(got) == len(names)
    for j, (f, g) in enumerate(fgs):
        want = ob.oracle_solve(A, soa(f), soa(g), dtype=dtype)
        _check(A, f, g, got[j], want, dtype, tight=(dtype == np.float64))
        if solo is not None:
            assert got[j]["iterations"] == solo[j]["iterations"], names[j]
            if solo[j]["status"] == 0:
                assert relerr(got[j]["x"], solo[j]["x"]) < 1e-9, names[j]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_member_bytes_do_not_depend_on_the_batch(dtype):
    pogs = _pogs()
    A, b = _problem_200x100()
    n = A.shape[1]
    P = PROBLEMS["lasso"](b, n)
    Q = PROBLEMS["huber"](b, n)
    R = PROBLEMS["logistic"](b, n)
    with pogs.Solver(A, dtype=dtype) as s:
        alone = s.solve_batch([P[0]], [P[1]])[0]
        mid = s.solve_batch([Q[0], P[0], R[0]], [Q[1], P[1], R[1]])
        others = [PROBLEMS[k](b, n) for k in ("ridge", "elastic_net", "svm", "nonneg_ls", "logistic0")]
        fs = [others[j % len(others)][0] for j in range(15)] + [P[0]]
        gs = [others[j % len(others)][1] for j in range(15)] + [P[1]]
        sixteen = s.solve_batch(fs, gs)
        again = s.solve_batch(fs, gs)
    _same_bytes(alone, mid[1])
    _same_bytes(alone, sixteen[15])
    for r1, r2 in zip(sixteen, again):
        _same_bytes(r1, r2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_frozen_members(dtype):
    pogs = _pogs()
    A, b = _problem_200x100()
    m, n = A.shape
    easy = PROBLEMS["ridge"](b, n)
    hard = PROBLEMS["svm"](b, n)
    # minimize sum y subject to y = A x: unbounded below, so it runs into max_iter
    capped = (pogs.FunctionVector(m, pogs.Function.kIdentity), pogs.FunctionVector(n, pogs.Function.kZero))
    with pogs.Solver(A, dtype=dtype) as s:
        solo_easy = s.solve_batch([easy[0]], [easy[1]])[0]
        solo_hard = s.solve_batch([hard[0]], [hard[1]])[0]
        assert solo_easy["status"] == 0 and solo_hard["status"] == 0
        assert solo_easy["iterations"] < solo_hard["iterations"], (solo_easy["iterations"], solo_hard["iterations"])
        max_iter = solo_hard["iterations"] + 40
        got = s.solve_batch([easy[0], hard[0], capped[0]], [easy[1], hard[1], capped[1]], max_iter=max_iter)
        st = s.stats()
    assert [r["status"] for r in got] == [0, 0, 3]
    assert got[2]["iterations"] == max_iter - 1
    _same_bytes(got[0], solo_easy)
    _same_bytes(got[1], solo_hard)
    assert st["iterations"] == max_iter
    assert st["batch_problem_iters"] == sum(r["iterations"] + 1 for r in got)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_per_problem_rho(dtype):
    pogs = _pogs()
    A, b = _problem_200x100()
    n = A.shape[1]
    fgs = [PROBLEMS["lasso"](b, n), PROBLEMS["ridge"](b, n), PROBLEMS["huber"](b, n)]
    rhos = [0.5, 1.0, 3.0]
    with pogs.Solver(A, dtype=dtype) as s:
        got = s.solve_batch([fg[0] for fg in fgs], [fg[1] for fg in fgs], rho=rhos, adaptive_rho=False)
    for (f, g), r, res in zip(fgs, rhos, got):
        want = ob.oracle_solve(A, soa(f), soa(g), dtype=dtype, rho=r, adaptive_rho=False)
        _check(A, f, g, res, want, dtype, tight=(dtype == np.float64))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(1037, 61), (4099, 1000), (33, 31)])
def test_batch_shapes(dtype, shape):
    pogs = _pogs()
    m, n = shape
    rng = np.random.default_rng(m + n)
    A = rng.standard_normal((m, n))
    b = A @ (rng.standard_normal(n) * (rng.random(n) < 0.2)) + 0.1 * rng.standard_normal(m)
    fgs = [PROBLEMS["lasso"](b, n), PROBLEMS["logistic"](b, n), PROBLEMS["ridge"](b, n)]
    with pogs.Solver(A, dtype=dtype) as s:
        got = s.solve_batch([fg[0] for fg in fgs], [fg[1] for fg in fgs])
    for (f, g), res in zip(fgs, got):
        want = ob.oracle_solve(A, soa(f), soa(g), dtype=dtype)
        _check(A, f, g, res, want, dtype, tight=False)


def _raw_batch(s, k, fs, gs):
    """PogsAmdSolveBatchFn with k as given (no splitting): (return code, last error)."""
    from pogs_amd import _lib

    fa, ga, keep = fn_arrays(fs, gs, s.dtype)
    x = np.zeros((max(len(fs), 1), s.n), s.dtype)
    it = np.zeros(max(len(fs), 1), np.uint32)
    st = np.zeros(max(len(fs), 1), np.int32)
    rc = _lib.lib.PogsAmdSolveBatchFn(s._h, k, fa, ga, None, 1e-4, 1e-4, 2500, 0, 1, 1, x.ctypes.data, None, None, None,
                                      None, it.ctypes.data, st.ctypes.data)
    del keep
    return rc, _lib.last_error()


def _call_with_nulls(s, f, g, x_null, it_null, st_null):
    from pogs_amd import _lib

    (fst, gst), keep = s._coef(f, g)
    x = np.zeros(s.n, s.dtype)
    it = np.zeros(1, np.uint32)
    st = np.zeros(1, np.int32)
    rc = _lib.lib.PogsAmdSolveBatchFn(s._h, 1, ctypes.byref(fst), ctypes.byref(gst), None, 1e-4, 1e-4, 2500, 0, 1, 1,
                                      None if x_null else x.ctypes.data, None, None, None, None,
                                      None if it_null else it.ctypes.data, None if st_null else st.ctypes.data)
    return rc, _lib.last_error()


def test_batch_refusals_leave_the_handle_usable():
    pogs = _pogs()
    from pogs_amd import _lib

    A, b = _problem_200x100()
    n = A.shape[1]
    f, g = PROBLEMS["lasso"](b, n)
    want = ob.oracle_solve(A, soa(f), soa(g))
    with pogs.Solver(A, dtype=np.float64) as s:
        for k, cnt in ((0, 0), (17, 17), (-1, 0)):
            rc, msg = _raw_batch(s, k, [f] * cnt, [g] * cnt)
            assert rc == 6 and msg, (k, rc, msg)
        for nulls in ((True, False, False), (False, True, False), (False, False, True)):
            rc, msg = _call_with_nulls(s, f, g, *nulls)
            assert rc == 6 and msg, nulls
        _check(A, f, g, s.solve_batch([f], [g])[0], want, np.float64, tight=True)
        _check(A, f, g, s.solve(f, g), want, np.float64, tight=True)
    # wide (m <= n: transposed storage)
    Aw = np.random.default_rng(3).standard_normal((50, 90))
    fw, gw = PROBLEMS["lasso"](np.ones(50), 90)
    with pogs.Solver(Aw, dtype=np.float64) as s:
        rc, msg = _raw_batch(s, 1, [fw], [gw])
        assert rc == 6 and "m > n" in msg
        assert s.solve(fw, gw)["status"] == 0
    # CGLS projector on a dense matrix
    with pogs.Solver(A, dtype=np.float64, projector=_lib.PROJ_CGLS) as s:
        rc, msg = _raw_batch(s, 1, [f], [g])
        assert rc == 6 and "direct projector" in msg
        assert s.solve(f, g)["status"] == 0
    # sparse handle
    sp = pytest.importorskip("scipy.sparse")
    with pogs.Solver(sp.csr_matrix(A), dtype=np.float64) as s:
        rc, msg = _raw_batch(s, 1, [f], [g])
        assert rc == 6 and "dense" in msg
        assert s.solve(f, g)["status"] == 0
    # row shards: a one-rank communicator exercises the sharded handle
    uid = pogs.dist_unique_id()
    with pogs.Solver(A, dtype=np.float64, dist=(0, 1, A.shape[0], uid)) as s:
        rc, msg = _raw_batch(s, 1, [f], [g])
        assert rc == 6 and "single-GPU" in msg
        _check(A, f, g, s.solve(f, g), want, np.float64, tight=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_leaves_solo_state_alone(dtype):
    pogs = _pogs()
    A, b = _problem_200x100()
    m, n = A.shape
    f, g = PROBLEMS["lasso"](b, n)
    fq, gq = PROBLEMS["huber"](b, n)
    with pogs.Solver(A, dtype=dtype) as s:
        before = s.solve(f, g)
        st_before = s.stats()
        s.solve_batch([fq, f], [gq, g])
        st_after = s.stats()
        after = s.solve(f, g)
        _same_bytes(before, after)
        for k in ("exact_iters", "rho_updates", "rho_final", "nrmA", "t_init_s", "t_loop_s"):
            assert st_after[k] == st_before[k], k
        # a warm start set before a batch still applies to the next solo solve
        x0 = before["x"] * 0.9
        l0 = before["l"] * 0.9
        s.warm_start(x0, l0)
        s.solve_batch([fq], [gq])
        warm = s.solve(f, g)
        s.warm_start(x0, l0)
        warm_direct = s.solve(f, g)
    _same_bytes(warm, warm_direct)
    assert warm["x"].tobytes() != before["x"].tobytes()   # the warm start did apply


def test_batch_full_size_c2_lasso_path_fp32():
    pogs = _pogs()
    from pogs_amd import synth

    A, b, _ = synth.dense_lasso_rows(100000, 10000, seed=0)
    n = A.shape[1]
    lambdas = [0.05, 0.07, 0.1, 0.14, 0.2, 0.28, 0.4, 0.56]   # around C2's lambda = 0.1
    fgs = [pogs.graph.lasso_functions(b, lam, n) for lam in lambdas]
    with pogs.Solver(A, dtype=np.float32) as s:
        t0 = time.perf_counter()
        got = s.solve_batch([fg[0] for fg in fgs], [fg[1] for fg in fgs])
        t1 = time.perf_counter()
        solo = [s.solve(f, g) for f, g in fgs]
        t2 = time.perf_counter()
    print("C2 lasso path, 8 values: batch %.3f s, solo %.3f s; iterations batch %s, solo %s"
          % (t1 - t0, t2 - t1, [r["iterations"] for r in got], [r["iterations"] for r in solo]))
    for r, w in zip(got, solo):
        assert r["status"] == w["status"] == 0
        slack = max(3, int(0.1 * w["iterations"]))
        assert abs(r["iterations"] - w["iterations"]) <= slack, (r["iterations"], w["iterations"])
        assert relerr(r["x"], w["x"]) < _xtol32(r["iterations"], w["iterations"])
