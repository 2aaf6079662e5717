"""GPU tests of batched sparse solves (Solver.solve_batch on a sparse handle / PogsAmdSolveBatchSparseFn): k problems on
one sparse handle with every product with A or A^T shared.  Each member is checked against its own oracle solve on the
same CSR at the bars of test_gpu_batch._check, and a member's bytes must not depend on the other members of its batch,
on its slot or on K (the products split a row over lanes by the matrix only, every partial sum has a fixed order)."""
import ctypes
import os
import time

import numpy as np
import pytest

import oracle_binding as ob
from helpers import PROBLEMS, fn_arrays, relerr, soa
from test_gpu_batch import _check as _dense_check
from test_gpu_batch import _same_bytes, _xtol32

sp = pytest.importorskip("scipy.sparse")

pytestmark = pytest.mark.gpu


def _pogs():
    import pogs_amd

    return pogs_amd


def _check(A, f, g, got, want, dtype, tight):
    """fp64: test_gpu_batch._check on the dense copy of A.  fp32: the same bars at the cap of _xtol32 (2e-4, the bar
    for iteration counts one apart) whatever the counts, optval within 5e-4 (ridge: 2.2e-4 from the oracle, whose
    stopping rule holds the solve to 1e-4 relative), and the dual within 1e-2 of its scale -- with the CGLS
    projector every fp32 projection stops at a tolerance-bound CG step, and the fp32 oracle's own dual lies ~3e-3 from
    the fp64 oracle's on these problems, so the tighter bars would measure CG stopping decisions, not the engine."""
    if dtype == np.float64:
        _dense_check(A.toarray(), f, g, got, want, dtype, tight)
        return
    from helpers import _fsum, objective

    assert got["status"] == want["status"]
    if want["status"] != 0:
        assert got["iterations"] == want["iterations"]
        return
    assert abs(got["iterations"] - want["iterations"]) <= max(3, int(0.1 * want["iterations"]))
    assert relerr(got["x"], want["x"]) < 2e-4
    assert relerr(got["y"], want["y"]) < 2e-4
    l_scale = max(np.linalg.norm(want["l"]), 1e-2 * np.linalg.norm(want["y"]))
    assert np.linalg.norm(got["l"].astype(np.float64) - want["l"]) / l_scale < 1e-2
    assert got["optval"] == pytest.approx(want["optval"], rel=5e-4, abs=1e-6)
    obj = _fsum(f, got["y"].astype(np.float64)) + _fsum(g, got["x"].astype(np.float64))
    assert obj == pytest.approx(got["optval"], rel=1e-4, abs=1e-4)
    true_obj = objective(A.toarray(), f, g, got["x"].astype(np.float64))
    assert true_obj == pytest.approx(got["optval"], rel=0.05, abs=1e-2)


def _fp32_reference_is_sound(A, f, g):
    """The fp32 oracle solve ends like the fp64 one (same status, x within the fp32 bar): where it does not, the member
    sits on a knife edge of the reference's own fp32 arithmetic and is checked in fp64 only."""
    w64 = ob.oracle_solve(A, soa(f), soa(g), dtype=np.float64)
    w32 = ob.oracle_solve(A, soa(f), soa(g), dtype=np.float32)
    return w32["status"] == w64["status"] and relerr(w32["x"], w64["x"]) < 1e-4


def _rand_csr(m, n, per_row, seed, long_row=None, empty_rows=()):
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for i in range(m):
        if i in empty_rows:
            continue
        k = long_row[1] if (long_row and i == long_row[0]) else int(rng.integers(1, 2 * per_row))
        c = rng.choice(n, size=min(k, n), replace=False)
        rows += [i] * len(c)
        cols += list(c)
        vals += list(rng.standard_normal(len(c)))
    A = sp.csr_matrix((vals, (rows, cols)), shape=(m, n))
    A.sort_indices()
    return A


def _problem(shape):
    """A random CSR with some empty rows and one long row, and a sparse-signal right-hand side."""
    m, n = shape
    if m > n:
        A = _rand_csr(m, n, 8, seed=m + 3 * n, long_row=(m // 3, min(n, 120)), empty_rows=(5, 17, m - 2))
    else:   # (wide: denser rows, so that most families converge within max_iter)
        A = _rand_csr(m, n, 60, seed=77, long_row=(50, 300), empty_rows=(5, 17))
    rng = np.random.default_rng(m * n)
    b = A @ (rng.standard_normal(n) * (rng.random(n) < 0.2)) + 0.1 * rng.standard_normal(m)
    return A, b


TALL, WIDE = (400, 150), (150, 400)
FAMILIES = ["lasso", "ridge", "elastic_net", "huber", "logistic", "svm", "nonneg_ls"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [TALL, WIDE])
def test_sparse_batch_families(dtype, shape):
    pogs = _pogs()
    A, b = _problem(shape)
    n = A.shape[1]
    fgs = [PROBLEMS[p](b, n) for p in FAMILIES]
    with pogs.Solver(A, dtype=dtype) as s:
        got = s.solve_batch([fg[0] for fg in fgs], [fg[1] for fg in fgs])
    assert len(got) == len(FAMILIES)
    checked = 0
    for j, (f, g) in enumerate(fgs):
        if dtype == np.float32 and not _fp32_reference_is_sound(A, f, g):
            continue
        want = ob.oracle_solve(A, soa(f), soa(g), dtype=dtype)
        _check(A, f, g, got[j], want, dtype, tight=(dtype == np.float64))
        checked += 1
    assert checked >= 4, checked


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sparse_batch_member_bytes_do_not_depend_on_the_batch(dtype):
    pogs = _pogs()
    A, b = _problem(TALL)
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
def test_sparse_batch_frozen_members(dtype):
    pogs = _pogs()
    A, b = _problem(TALL)
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
    assert st["cg_iters"] > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sparse_batch_per_problem_rho(dtype):
    pogs = _pogs()
    A, b = _problem(TALL)
    n = A.shape[1]
    fgs = [PROBLEMS["lasso"](b, n), PROBLEMS["ridge"](b, n), PROBLEMS["huber"](b, n)]
    rhos = [0.5, 2.0, 3.0]
    with pogs.Solver(A, dtype=dtype) as s:
        got = s.solve_batch([fg[0] for fg in fgs], [fg[1] for fg in fgs], rho=rhos, adaptive_rho=False)
    for (f, g), r, res in zip(fgs, rhos, got):
        want = ob.oracle_solve(A, soa(f), soa(g), dtype=dtype, rho=r, adaptive_rho=False)
        _check(A, f, g, res, want, dtype, tight=(dtype == np.float64))


def _raw_sparse_solver(pogs, A, dtype, order):
    """A Solver around a handle built through PogsAmdCreateSparse from CSR (ROW_MAJ) or CSC (COL_MAJ) host arrays."""
    from pogs_amd import _lib

    M = sp.csr_matrix(A) if order == 1 else sp.csc_matrix(A)
    M.sort_indices()
    data = np.ascontiguousarray(M.data, dtype)
    ptr = np.ascontiguousarray(M.indptr, np.int32)
    ind = np.ascontiguousarray(M.indices, np.int32)
    h = ctypes.c_void_p()
    code = _lib.F64 if dtype == np.float64 else _lib.F32
    opt = _lib.PogsAmdOptions(device=-1, projector=_lib.PROJ_DEFAULT, profile=0)
    rc = _lib.lib.PogsAmdCreateSparse(ctypes.byref(h), code, order, A.shape[0], A.shape[1], M.nnz,
                                      data.ctypes.data, ptr.ctypes.data, ind.ctypes.data, _lib.HOST, ctypes.byref(opt),
                                      None)
    assert rc == 0, _lib.last_error()
    s = object.__new__(pogs.Solver)
    s._h, s.dtype, s.sparse = h, np.dtype(dtype).type, True
    s.m, s.n = A.shape
    return s


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sparse_batch_csc_and_device_csr_give_the_host_csr_bytes(dtype):
    import torch

    pogs = _pogs()
    A, b = _problem(WIDE)
    n = A.shape[1]
    fgs = [PROBLEMS[k](b, n) for k in ("lasso", "logistic", "huber")]
    fs, gs = [fg[0] for fg in fgs], [fg[1] for fg in fgs]
    with pogs.Solver(A, dtype=dtype) as s:
        host = s.solve_batch(fs, gs)
    for order in (1, 0):   # ROW_MAJ (CSR), COL_MAJ (CSC)
        s = _raw_sparse_solver(pogs, A, dtype, order)
        try:
            raw = s.solve_batch(fs, gs)
        finally:
            s.close()
        for r1, r2 in zip(host, raw):
            _same_bytes(r1, r2)
    dev = torch.device("cuda:0")
    data = torch.from_numpy(np.ascontiguousarray(A.data, dtype)).to(dev)
    ptr = torch.from_numpy(np.ascontiguousarray(A.indptr, np.int32)).to(dev)
    ind = torch.from_numpy(np.ascontiguousarray(A.indices, np.int32)).to(dev)
    with pogs.Solver((data.data_ptr(), ptr.data_ptr(), ind.data_ptr(), A.nnz), dtype=dtype, shape=A.shape,
                     device_ptr=True) as s:
        got = s.solve_batch(fs, gs)
    for r1, r2 in zip(host, got):
        _same_bytes(r1, r2)


def _raw_batch(s, k, fs, gs):
    """PogsAmdSolveBatchSparseFn with k as given (no splitting): (return code, last error)."""
    from pogs_amd import _lib

    fa, ga, keep = fn_arrays(fs, gs, s.dtype)
    x = np.zeros((max(len(fs), 1), s.n), s.dtype)
    it = np.zeros(max(len(fs), 1), np.uint32)
    st = np.zeros(max(len(fs), 1), np.int32)
    rc = _lib.lib.PogsAmdSolveBatchSparseFn(s._h, k, fa, ga, None, 1e-4, 1e-4, 2500, 0, 1, 1, x.ctypes.data, None, None,
                                            None, None, it.ctypes.data, st.ctypes.data)
    del keep
    return rc, _lib.last_error()


def _call_with_nulls(s, f, g, x_null, it_null, st_null):
    from pogs_amd import _lib

    (fst, gst), keep = s._coef(f, g)
    x = np.zeros(s.n, s.dtype)
    it = np.zeros(1, np.uint32)
    st = np.zeros(1, np.int32)
    rc = _lib.lib.PogsAmdSolveBatchSparseFn(s._h, 1, ctypes.byref(fst), ctypes.byref(gst), None, 1e-4, 1e-4, 2500, 0, 1,
                                            1, None if x_null else x.ctypes.data, None, None, None, None,
                                            None if it_null else it.ctypes.data, None if st_null else st.ctypes.data)
    del keep
    return rc, _lib.last_error()


def test_sparse_batch_refusals_leave_the_handle_usable():
    pogs = _pogs()
    A, b = _problem(TALL)
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
    # dense handle: refused by the sparse entry, still served by the dense one
    Ad = A.toarray()
    want_d = ob.oracle_solve(Ad, soa(f), soa(g))
    with pogs.Solver(Ad, dtype=np.float64) as s:
        rc, msg = _raw_batch(s, 1, [f], [g])
        assert rc == 6 and "needs a sparse handle" in msg
        _check(A, f, g, s.solve_batch([f], [g])[0], want_d, np.float64, tight=True)
    # row shards: a one-rank communicator exercises the sharded sparse handle
    uid = pogs.dist_unique_id()
    with pogs.Solver(A, dtype=np.float64, dist=(0, 1, A.shape[0], uid)) as s:
        rc, msg = _raw_batch(s, 1, [f], [g])
        assert rc == 6 and "single-GPU" in msg
        _check(A, f, g, s.solve(f, g), want, np.float64, tight=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sparse_batch_leaves_solo_state_alone(dtype):
    pogs = _pogs()
    A, b = _problem(TALL)
    n = A.shape[1]
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


@pytest.mark.parametrize("path", ["lasso", "logistic"])
def test_sparse_paths_match_per_lambda_oracle_solves(path):
    pogs = _pogs()
    A, b = _problem(TALL)
    n = A.shape[1]
    lambdas = list(np.geomspace(0.02, 0.5, 18))   # more than one batch of 16
    if path == "lasso":
        res = pogs.solve_lasso_path(A, b, lambdas, dtype=np.float64)
        make = pogs.graph.lasso_functions
        bb = b
    else:
        bb = np.sign(b) + (b == 0)
        res = pogs.solve_logistic_path(A, bb, lambdas, dtype=np.float64)
        make = pogs.graph.logistic_functions
    assert res["x"].shape == (len(lambdas), n)
    for j, lam in enumerate(lambdas):
        f, g = make(bb, lam, n)
        want = ob.oracle_solve(A, soa(f), soa(g), dtype=np.float64)
        got = {"x": res["x"][j], "optval": res["optval"][j], "iterations": int(res["iterations"][j]),
               "status": int(res["status"][j])}
        assert got["status"] == want["status"] == 0, lam
        assert abs(got["iterations"] - want["iterations"]) <= 2, (lam, got["iterations"], want["iterations"])
        assert relerr(got["x"], want["x"]) < 1e-6, lam
        assert got["optval"] == pytest.approx(want["optval"], rel=1e-7, abs=1e-9), lam


def test_sparse_batch_full_size_c4_lasso_path_fp32():
    """C4's matrix (2e6 x 5e5 CSR, 1e8 non-zeros, fp32) with 8 lambda values around the fixture's 0.1: that member meets
    test_c4_solution_matches_compiled_reference_fixture's bars against the compiled reference; the others match their
    own solo solves on the same handle within the fp32 bars."""
    pogs = _pogs()
    from pogs_amd import synth

    path = os.path.join(os.path.dirname(__file__), "golden", "c4_reference.npz")
    fx = np.load(path)
    m, n, k = (int(v) for v in fx["shape"])
    A, b, _ = synth.csr_lasso(m, n, k, seed=int(fx["seed"]), dtype=np.float32)
    chk = np.array([float(A.nnz), float(A.data[::1009].astype(np.float64).sum()),
                    float(A.indices[::1013].astype(np.float64).sum()), float(np.linalg.norm(b)), float(b[::101].sum())])
    np.testing.assert_allclose(chk, fx["checksums"], rtol=1e-12, err_msg="the generator no longer reproduces the inputs")
    lam = float(fx["lam"])
    lambdas = [0.05, 0.07, lam, 0.14, 0.2, 0.28, 0.4, 0.56]
    fgs = [pogs.graph.lasso_functions(b, v, n) for v in lambdas]
    with pogs.Solver(A, dtype=np.float32) as s:
        t0 = time.perf_counter()
        got = s.solve_batch([fg[0] for fg in fgs], [fg[1] for fg in fgs])
        t1 = time.perf_counter()
        solo = [s.solve(f, g) for f, g in fgs]
        t2 = time.perf_counter()
    print("C4 lasso path, 8 values: batch %.3f s, solo %.3f s; iterations batch %s, solo %s"
          % (t1 - t0, t2 - t1, [r["iterations"] for r in got], [r["iterations"] for r in solo]))
    r = got[2]
    it, itr = r["iterations"] + 1, int(fx["iterations"]) + 1
    x, xr = r["x"].astype(np.float64), fx["x"].astype(np.float64)
    rel_x = np.linalg.norm(x - xr) / np.linalg.norm(xr)
    obj = 0.5 * float(np.sum((A.astype(np.float64) @ x - b) ** 2)) + lam * float(np.abs(x).sum())
    print("C4 member lambda %.2f vs the reference: iterations %d / %d, rel_x %.3e, objective at x %.6f / %.6f"
          % (lam, it, itr, rel_x, obj, float(fx["objective_at_x"])))
    assert r["status"] == int(fx["status"]) == 0
    assert abs(it - itr) <= max(3, itr // 10)
    assert rel_x <= 1e-4
    assert abs(obj - float(fx["objective_at_x"])) <= 1e-4 * float(fx["objective_at_x"])
    for j, (rj, w) in enumerate(zip(got, solo)):
        if j == 2:
            continue
        assert rj["status"] == w["status"] == 0
        slack = max(3, int(0.1 * w["iterations"]))
        assert abs(rj["iterations"] - w["iterations"]) <= slack, (rj["iterations"], w["iterations"])
        assert relerr(rj["x"], w["x"]) < _xtol32(rj["iterations"], w["iterations"])
