"""GPU tests of warm-started batched solves (Solver.solve_batch with x0 / l0, PogsAmdSolveBatchWarmFn) and of the chained
regularisation path on top of them (Solver.solve_chain, solve_lasso_path(chain=True)), on a dense handle and on sparse
handles with the CGLS and the direct projector.

ADMM converges from any start, so the warm begin itself is pinned by the first one and two iterations against the
oracle's warm start (a cold start, a negated l0 or rho = 1 in place of the given rho each move x, y and l of the
203 x 101 case by >= 0.18 there); converged members are compared with the oracle run on the same schedule; and a
member's bytes must depend neither on its batch, nor on its slot, nor on which other members are warm."""
import ctypes
import math

import numpy as np
import pytest

import oracle_binding as ob
from helpers import PROBLEMS, _fsum, fn_arrays, objective, relerr, soa

pytestmark = pytest.mark.gpu

RATIOS = (0.5, 0.4, 0.3, 0.2, 0.1, 0.05)   # lambda / lambda_max of the path; slots = 2 cuts it into two segments of 3
CASES = ("dense", "sparse_tall_cgls", "sparse_wide_cgls", "sparse_tall_direct")
DTYPES = (np.float64, np.float32)


def _pogs():
    import pogs_amd

    return pogs_amd


def report(line):
    print("[batch warm] " + line)


# ---- bars, restated from tests/test_gpu_batch.py, tests/test_gpu_sparse_batch.py and tests/test_gpu_sparse_direct.py ----

def _tol(dtype, f64, f32):
    return f64 if dtype == np.float64 else f32


def _xtol32(got_iters, want_iters, loose=2e-4):
    """2e-5 at the same iteration count, else 1e-4 per iteration apart, capped at 2e-4."""
    d = abs(int(got_iters) - int(want_iters))
    return 2e-5 if d == 0 else min(loose, 1e-4 * (1 + d))


def _l_err(got, want):
    l_scale = max(np.linalg.norm(want["l"]), 1e-2 * np.linalg.norm(want["y"]))
    return np.linalg.norm(got["l"].astype(np.float64) - want["l"]) / l_scale


def _check(A, f, g, got, want, dtype, tight):
    """test_gpu_batch._check: same status; iterations within 2 (tight, fp64) or max(3, 10 %); x and y within 1e-6
    (tight) / 1e-4 (fp32: _xtol32); the dual within 10x that on the scale of y; optval within 1e-7 / 1e-4 relative
    (fp32: _xtol32), equal to sum f(y) + sum g(x) recomputed in numpy, and the true objective at x within 5 % of it."""
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
    assert _l_err(got, want) < 10 * xtol
    otol = 1e-7 if tight else (1e-4 if dtype == np.float64 else _xtol32(it_g, it_w))
    assert got["optval"] == pytest.approx(want["optval"], rel=otol, abs=1e-9 if tight else 1e-6)
    obj = _fsum(f, got["y"].astype(np.float64)) + _fsum(g, got["x"].astype(np.float64))
    assert obj == pytest.approx(got["optval"], rel=_tol(dtype, 1e-9, 1e-4), abs=_tol(dtype, 1e-9, 1e-4))
    true_obj = objective(np.asarray(A, np.float64), f, g, got["x"].astype(np.float64))
    assert true_obj == pytest.approx(got["optval"], rel=0.05, abs=1e-2)


def _check_cgls(A, f, g, got, want, dtype):
    """test_gpu_sparse_batch._check: fp64 as _check (tight) on the dense copy; fp32 at the cap of _xtol32 whatever the
    counts, optval within 5e-4 and the dual within 1e-2 of its scale (every fp32 projection stops at a tolerance-bound
    CG step)."""
    if dtype == np.float64:
        _check(A, f, g, got, want, dtype, True)
        return
    assert got["status"] == want["status"]
    if want["status"] != 0:
        assert got["iterations"] == want["iterations"]
        return
    assert abs(got["iterations"] - want["iterations"]) <= max(3, int(0.1 * want["iterations"]))
    assert relerr(got["x"], want["x"]) < 2e-4
    assert relerr(got["y"], want["y"]) < 2e-4
    assert _l_err(got, want) < 1e-2
    assert got["optval"] == pytest.approx(want["optval"], rel=5e-4, abs=1e-6)
    obj = _fsum(f, got["y"].astype(np.float64)) + _fsum(g, got["x"].astype(np.float64))
    assert obj == pytest.approx(got["optval"], rel=1e-4, abs=1e-4)
    true_obj = objective(A, f, g, got["x"].astype(np.float64))
    assert true_obj == pytest.approx(got["optval"], rel=0.05, abs=1e-2)


def _check_direct(got, want, dtype):
    """test_gpu_sparse_direct._follows (a direct sparse handle against the oracle's dense direct solve): solved,
    iterations within 1 (fp64) / 3 (fp32), x within 1e-6 / 1e-4, optval within 1e-6 / 2e-4; y as x, the dual at 10x."""
    f64 = dtype == np.float64
    assert got["status"] == want["status"] == 0
    assert abs(int(got["iterations"]) - int(want["iterations"])) <= (1 if f64 else 3), (got["iterations"], want["iterations"])
    xtol = 1e-6 if f64 else 1e-4
    assert relerr(got["x"], want["x"]) < xtol
    assert relerr(got["y"], want["y"]) < xtol
    assert _l_err(got, want) < 10 * xtol
    assert abs(got["optval"] - want["optval"]) / max(abs(want["optval"]), 1e-300) <= (1e-6 if f64 else 2e-4)


def _same_bytes(r1, r2):
    for k in ("x", "y", "l", "mu"):
        assert r1[k].tobytes() == r2[k].tobytes(), k
    assert np.float64(r1["optval"]).tobytes() == np.float64(r2["optval"]).tobytes()
    assert r1["iterations"] == r2["iterations"] and r1["status"] == r2["status"]
    if "rho" in r1 and "rho" in r2:
        assert np.float64(r1["rho"]).tobytes() == np.float64(r2["rho"]).tobytes()


# ---- the cases: made once, their oracle solves too ----------------------------------------------------------------------

_cases, _oracle = {}, {}


def _case(name):
    """(A for the handle, dense fp64 copy, b, lambda_max): dense 203 x 101 (padding in both dimensions for fp32 and fp64);
    sparse 203 x 101 and sparse 61 x 150, both at 10 % density (scipy is needed by the sparse cases only)."""
    key = "dense" if name == "dense" else ("wide" if "wide" in name else "tall")
    if key not in _cases:
        if key == "dense":
            rng = np.random.default_rng(11)
            m, n = 203, 101
            A = rng.standard_normal((m, n))
            Ad = A
        else:
            sp = pytest.importorskip("scipy.sparse")
            m, n, dens, seed = (203, 101, 0.10, 5) if key == "tall" else (61, 150, 0.10, 7)
            rng = np.random.default_rng(seed)
            A = sp.random(m, n, dens, random_state=rng, format="csr", dtype=np.float64)
            A.data[:] = rng.standard_normal(A.nnz)
            A.sort_indices()
            Ad = A.toarray()
        b = Ad @ (rng.standard_normal(n) * (rng.random(n) < 0.2)) + 0.1 * rng.standard_normal(m)
        _cases[key] = (A, Ad, b, float(np.max(np.abs(Ad.T @ b))))
    return _cases[key]


def _solver(name, dtype):
    from pogs_amd import _lib

    A = _case(name)[0]
    if name.endswith("direct"):
        return _pogs().Solver(A, dtype=dtype, projector=_lib.PROJ_DIRECT)
    return _pogs().Solver(A, dtype=dtype)


def _fg(name, ratio):
    _, Ad, b, lmax = _case(name)
    return _pogs().graph.lasso_functions(b, ratio * lmax, Ad.shape[1])


def _oracle_solve(name, dtype, ratio, start=None, max_iter=2500):
    """The oracle on a case's lasso at ratio * lambda_max: the CSR with CGLS for a CGLS handle, else the dense direct
    solve.  start: None (cold, rho 1) or (x0, l0, rho)."""
    warm = start is not None
    key = (name, np.dtype(dtype).name, ratio, max_iter) if not warm else None
    if key is not None and key in _oracle:
        return _oracle[key]
    A, Ad, _, _ = _case(name)
    f, g = _fg(name, ratio)
    kw = dict(dtype=dtype, max_iter=max_iter)
    if warm:
        kw.update(x0=start[0], l0=start[1], rho=start[2])
    r = ob.oracle_solve(A, soa(f), soa(g), use_cgls=True, **kw) if name.endswith("cgls") else \
        ob.oracle_solve(Ad, soa(f), soa(g), **kw)
    if key is not None:
        _oracle[key] = r
    return r


def _start_of(r):
    return r["x"], r["l"], r["info"]["rho_final"] if "info" in r else r["rho"]


def _oracle_chain(name, dtype, slots):
    """The oracle on the chain's schedule, fed its own predecessor's x, l and final rho."""
    key = (name, np.dtype(dtype).name, "chain", slots)
    if key not in _oracle:
        res = [None] * len(RATIOS)
        for rnd in _pogs().graph._chain_schedule(len(RATIOS), slots):
            for j, pred in rnd:
                res[j] = _oracle_solve(name, dtype, RATIOS[j], start=None if pred is None else _start_of(res[pred]))
        _oracle[key] = res
    return _oracle[key]


def _check_member(name, ratio, got, want, dtype):
    _, Ad, _, _ = _case(name)
    f, g = _fg(name, ratio)
    report("%s %s lambda %.2f: iterations %d (oracle %d), |dx|/|x| %.2e, |dy|/|y| %.2e, dual %.2e, optval %.2e"
           % (name, np.dtype(dtype).name, ratio, got["iterations"], want["iterations"], relerr(got["x"], want["x"]),
              relerr(got["y"], want["y"]), _l_err(got, want),
              abs(got["optval"] - want["optval"]) / max(abs(want["optval"]), 1e-300)))
    if name == "dense":
        _check(Ad, f, g, got, want, dtype, tight=(dtype == np.float64))
    elif name.endswith("cgls"):
        _check_cgls(Ad, f, g, got, want, dtype)
    else:
        _check_direct(got, want, dtype)


def _raw(s, fs, gs, rho=None, x0=None, l0=None, warm=None, want_rho=True, k=None, max_iter=2500):
    """PogsAmdSolveBatchWarmFn with the pointers as given (None: NULL) and k as given (no splitting).  The outputs
    start as a pattern, so that a refused call can be seen to have written nothing.
    Returns (return code, last error, list of result dicts, the output arrays)."""
    from pogs_amd import _lib

    cnt = len(fs)
    k = cnt if k is None else k
    fa, ga, keep = fn_arrays(fs, gs, s.dtype)
    rows = max(cnt, 1)
    out = {"x": np.full((rows, s.n), 7, s.dtype), "y": np.full((rows, s.m), 7, s.dtype),
           "l": np.full((rows, s.m), 7, s.dtype), "mu": np.full((rows, s.n), 7, s.dtype),
           "optval": np.full(rows, 7.0), "iterations": np.full(rows, 7, np.uint32), "status": np.full(rows, 7, np.int32),
           "rho": np.full(rows, 7.0)}
    arr = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)   # noqa: E731
    r, xs, ls, w = arr(rho, np.float64), arr(x0, s.dtype), arr(l0, s.dtype), arr(warm, np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    rc = _lib.lib.PogsAmdSolveBatchWarmFn(s._h, k, fa, ga, ptr(r), ptr(xs), ptr(ls), ptr(w), 1e-4, 1e-4, max_iter, 0, 1, 1,
                                          ptr(out["x"]), ptr(out["y"]), ptr(out["l"]), ptr(out["mu"]), ptr(out["optval"]),
                                          ptr(out["iterations"]), ptr(out["status"]),
                                          ptr(out["rho"]) if want_rho else None)
    msg = _lib.last_error()
    del keep
    res = [{"x": out["x"][j], "y": out["y"][j], "l": out["l"][j], "mu": out["mu"][j], "optval": float(out["optval"][j]),
            "iterations": int(out["iterations"][j]), "status": int(out["status"][j]), "rho": float(out["rho"][j])}
           for j in range(cnt)]
    return rc, msg, res, out


def _untouched(out):
    return all(np.all(a == 7) for a in out.values())


# ---- 1. the start itself -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", CASES)
def test_first_iterations_follow_the_oracles_warm_start(name, dtype):
    start = _start_of(_oracle_solve(name, dtype, 0.4))
    f, g = _fg(name, 0.3)
    f64 = dtype == np.float64
    if name.endswith("cgls"):
        xtol, ltol = (1e-6, 1e-5) if f64 else (2e-4, 1e-2)   # the bars of the sparse batch tests
    elif name.endswith("direct"):
        xtol, ltol = (1e-6, 1e-5) if f64 else (1e-4, 1e-3)   # the bars of the direct sparse handle's tests
    else:
        xtol, ltol = (1e-6, 1e-5) if f64 else (2e-5, 2e-4)   # fp32: the suite's bar at equal iteration counts
    with _solver(name, dtype) as s:
        for max_iter in (2, 1):
            got = s.solve_batch([f], [g], rho=[start[2]], x0=[start[0]], l0=[start[1]], max_iter=max_iter)[0]
            want = _oracle_solve(name, dtype, 0.3, start=start, max_iter=max_iter)
            ex, ey, el = relerr(got["x"], want["x"]), relerr(got["y"], want["y"]), _l_err(got, want)
            report("%s %s max_iter %d: status %d (oracle %d), iterations %d, |dx|/|x| %.2e, |dy|/|y| %.2e, dual %.2e"
                   % (name, np.dtype(dtype).name, max_iter, got["status"], want["status"], got["iterations"], ex, ey, el))
            assert want["status"] == 3 and want["iterations"] == max_iter - 1
            assert got["status"] == 3 and got["iterations"] == max_iter - 1
            assert ex < xtol and ey < xtol and el < ltol
            assert math.isfinite(got["rho"]) and got["rho"] > 0


# ---- 2. converged warm members against the oracle; 8. the path front end ---------------------------------------------

# (The wide matrix is 10 % dense: at 30 % the oracle's own fp32 solves of this shape are unsound -- cold, 876 to 2096
# iterations where its fp64 solves take about 100 -- and would be no reference.  On this one the oracle takes the same
# iteration counts in fp32 as in fp64, cold (133, 133, 149, 142, 103, 96) and chained (133, 36, 37 / 142, 52, 49), with
# its fp32 x within 8e-6 (cold) and 4e-7 (chained) of its fp64 x.  Measured on the device in fp32, against the 2e-4 bar
# of the sparse batch tests: the first four members within 5e-7, lambda 0.1 at 1.4e-4 with the oracle's count and 0.05 at
# 1.9e-4 with 51 iterations for 49 -- fp32 CG steps that stop on the other side of the tolerance; in fp64 all six lie
# within 2e-15 at the oracle's counts.)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", CASES)
def test_chain_follows_the_oracle_on_the_same_schedule(name, dtype):
    pogs = _pogs()
    fgs = [_fg(name, r) for r in RATIOS]
    fs, gs = [fg[0] for fg in fgs], [fg[1] for fg in fgs]
    with _solver(name, dtype) as s:
        cold = s.solve_batch(fs, gs)
        chain = s.solve_chain(fs, gs, rho=1.0, slots=2)
        st = s.stats()
    want = _oracle_chain(name, dtype, 2)
    total = sum(r["iterations"] + 1 for r in chain)
    total_cold = sum(r["iterations"] + 1 for r in cold)
    report("%s %s chain iterations %s (oracle %s), cold %s; rho %s" % (
        name, np.dtype(dtype).name, [r["iterations"] for r in chain], [w["iterations"] for w in want],
        [r["iterations"] for r in cold], ["%.4g" % r["rho"] for r in chain]))
    assert all(w["status"] == 0 for w in want)
    for j, ratio in enumerate(RATIOS):
        _check_member(name, ratio, chain[j], want[j], dtype)
        assert math.isfinite(chain[j]["rho"]) and chain[j]["rho"] > 0
        if dtype == np.float64 and chain[j]["iterations"] == want[j]["iterations"]:
            assert chain[j]["rho"] == pytest.approx(want[j]["info"]["rho_final"], rel=1e-6)
    assert total < total_cold, (total, total_cold)
    # the stats are those of the chain's last round: the third member of each segment
    assert st["batch_problem_iters"] == chain[2]["iterations"] + chain[5]["iterations"] + 2
    if name == "dense":
        # (the oracle: 116, 10, 9 / 100, 11, 10 iterations, 262 with the stopping iteration counted, against 601 cold)
        lambdas = [r * _case(name)[3] for r in RATIOS]
        A, _, b, _ = _case(name)
        path = pogs.solve_lasso_path(A, b, lambdas, dtype=dtype)
        for j, r in enumerate(cold):
            assert path["x"][j].tobytes() == r["x"].tobytes()
            assert path["optval"][j] == r["optval"] and path["iterations"][j] == r["iterations"]
            assert path["status"][j] == r["status"]
        chained = pogs.solve_lasso_path(A, b, lambdas, dtype=dtype, chain=True, slots=2)
        assert sorted(chained) == sorted(path)
        for j, r in enumerate(chain):
            assert chained["x"][j].tobytes() == r["x"].tobytes()
            assert chained["optval"][j] == r["optval"] and chained["iterations"][j] == r["iterations"]
            assert chained["status"][j] == r["status"]


# ---- 3. against the solo warm solve -------------------------------------------------------------------------------------

def test_warm_member_matches_the_solo_warm_solve():
    dtype = np.float64
    start = _start_of(_oracle_solve("dense", dtype, 0.4))
    f, g = _fg("dense", 0.3)
    with _solver("dense", dtype) as s:
        got = s.solve_batch([f], [g], rho=[start[2]], x0=[start[0]], l0=[start[1]])[0]
        s.warm_start(start[0], start[1])
        solo = s.solve(f, g, rho=start[2])
        cold = s.solve(f, g)
    report("dense warm member: iterations %d, solo warm %d, solo cold %d, |dx|/|x| %.2e"
           % (got["iterations"], solo["iterations"], cold["iterations"], relerr(got["x"], solo["x"])))
    assert got["status"] == solo["status"] == 0
    assert got["iterations"] == solo["iterations"] < cold["iterations"]
    assert relerr(got["x"], solo["x"]) < 1e-9


# ---- 4. independence, bytes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", CASES)
def test_member_bytes_do_not_depend_on_the_batch(name, dtype):
    _, Ad, b, _ = _case(name)
    m, n = Ad.shape
    x0, l0, rho = _start_of(_oracle_solve(name, dtype, 0.4))
    P = _fg(name, 0.3)                       # the warm member under test
    C = _fg(name, 0.2)                       # the cold member under test
    others = [PROBLEMS[k](b, n) for k in ("ridge", "elastic_net", "huber", "nonneg_ls", "logistic0")]
    nan_x, nan_l = np.full(n, np.nan), np.full(m, np.nan)
    cap = 150      # bytes are compared, so a member may as well stop here (status 3) as converge: some do either
    with _solver(name, dtype) as s:
        alone = s.solve_batch([P[0]], [P[1]], rho=[rho], x0=[x0], l0=[l0], max_iter=cap)[0]
        cold_old = s.solve_batch([C[0]], [C[1]], max_iter=cap)[0]                      # the cold entries
        # slot 1 of 3: a cold member before it, a warm one of another family after it
        mid = s.solve_batch([others[0][0], P[0], others[2][0]], [others[0][1], P[1], others[2][1]], rho=[1.0, rho, 2.0],
                            x0=[None, x0, 0.5 * x0], l0=[None, l0, 0.5 * l0], warm=[False, True, True], max_iter=cap)
        # slot 15 of 16 among mixed warm and cold members; the cold member under test in slot 4, NaN in its rows
        fs = [others[j % len(others)][0] for j in range(15)] + [P[0]]
        gs = [others[j % len(others)][1] for j in range(15)] + [P[1]]
        fs[4], gs[4] = C
        flags = [j % 3 == 1 for j in range(15)] + [True]
        flags[4] = False
        xs = np.stack([nan_x if not flags[j] else (x0 if j == 15 else (0.1 * j) * x0) for j in range(16)])
        ls = np.stack([nan_l if not flags[j] else (l0 if j == 15 else (0.1 * j) * l0) for j in range(16)])
        rhos = [1.0 + 0.1 * j for j in range(15)] + [rho]
        rhos[4] = 1.0
        rc, msg, sixteen, _ = _raw(s, fs, gs, rho=rhos, x0=xs, l0=ls, warm=flags, max_iter=cap)
        assert rc == 0, msg
        st = s.stats()
        rc, msg, again, _ = _raw(s, fs, gs, rho=rhos, x0=xs, l0=ls, warm=flags, max_iter=cap)
        assert rc == 0, msg
        # the cold member through the new entry with no start at all, and without rho_final
        rc, msg, cold_null, out = _raw(s, [C[0]], [C[1]], want_rho=False, max_iter=cap)
        assert rc == 0, msg
        st_cold_new = s.stats()
        s.solve_batch([C[0]], [C[1]], max_iter=cap)
        st_cold_old = s.stats()
        # a warm start from zero is the cold start, so the same iterations run: what differs is the two products
        zero = s.solve_batch([C[0]], [C[1]], x0=[np.zeros(n)], l0=[np.zeros(m)], max_iter=cap)[0]
        st_zero = s.stats()
    assert alone["status"] in (0, 3) and cold_old["status"] in (0, 3)
    assert len({r["iterations"] for r in sixteen}) > 2                  # members stop at different iterations
    _same_bytes(alone, mid[1])
    _same_bytes(alone, sixteen[15])
    for r1, r2 in zip(sixteen, again):
        _same_bytes(r1, r2)
    assert all(np.all(np.isfinite(r["x"])) for r in sixteen)
    cold_old = dict(cold_old)
    _same_bytes(cold_old, sixteen[4])
    _same_bytes(cold_old, cold_null[0])
    assert np.all(out["rho"] == 7)                                       # rho_final = NULL: nothing written there
    # an all-cold batch through the new entry counts what the cold entries count; a warm begin adds its two products
    assert st_cold_new["matvecs"] == st_cold_old["matvecs"] and st_cold_new["iterations"] == st_cold_old["iterations"]
    assert st["batch_problem_iters"] == sum(r["iterations"] + 1 for r in sixteen)
    assert zero["iterations"] == cold_old["iterations"] and np.array_equal(zero["x"], cold_old["x"])
    assert st_zero["matvecs"] == st_cold_old["matvecs"] + 2


# ---- 5. frozen members ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_a_warm_member_that_stops_at_once_next_to_a_long_cold_one(dtype):
    quick = _fg("dense", 0.3)
    slow = _fg("dense", 0.5)
    with _solver("dense", dtype) as s:
        own = s.solve_batch([quick[0]], [quick[1]], return_rho=True)[0]
        assert own["status"] == 0
        kw = dict(rho=[own["rho"]], x0=[own["x"]], l0=[own["l"]])
        warm_alone = s.solve_batch([quick[0]], [quick[1]], **kw)[0]
        cold_alone = s.solve_batch([slow[0]], [slow[1]])[0]
        both = s.solve_batch([quick[0], slow[0]], [quick[1], slow[1]], rho=[own["rho"], 1.0], x0=[own["x"], None],
                             l0=[own["l"], None], warm=[True, False])
        st = s.stats()
    report("dense %s: warm from its own solution stops at iteration %d (cold %d); the cold neighbour runs %d"
           % (np.dtype(dtype).name, warm_alone["iterations"], own["iterations"], cold_alone["iterations"]))
    assert warm_alone["status"] == 0 and warm_alone["iterations"] <= 1
    assert cold_alone["status"] == 0 and cold_alone["iterations"] >= 80
    _same_bytes(both[0], warm_alone)
    _same_bytes(both[1], cold_alone)
    assert st["iterations"] == cold_alone["iterations"] + 1
    assert st["batch_problem_iters"] == warm_alone["iterations"] + cold_alone["iterations"] + 2


# ---- 7. refusals on a live handle --------------------------------------------------------------------------------------

def test_refusals_write_nothing_and_leave_the_handle_usable():
    dtype = np.float64
    x0, l0, rho = _start_of(_oracle_solve("dense", dtype, 0.4))
    f, g = _fg("dense", 0.3)
    want = _oracle_solve("dense", dtype, 0.3, start=(x0, l0, rho))
    with _solver("dense", dtype) as s:
        refused = {
            "x0 alone": dict(fs=[f], gs=[g], x0=x0[None]),
            "l0 alone": dict(fs=[f], gs=[g], l0=l0[None]),
            "flags without x0": dict(fs=[f], gs=[g], warm=[1]),
            "k = 17": dict(fs=[f] * 17, gs=[g] * 17, x0=np.tile(x0, (17, 1)), l0=np.tile(l0, (17, 1))),
            "k = 0": dict(fs=[f], gs=[g], k=0),
        }
        for label, kw in refused.items():
            rc, msg, _, out = _raw(s, kw.pop("fs"), kw.pop("gs"), **kw)
            assert rc == 6 and msg, label
            assert _untouched(out), label
            rc, msg, res, _ = _raw(s, [f], [g], rho=[rho], x0=x0[None], l0=l0[None])
            assert rc == 0, (label, msg)
            _check_member("dense", 0.3, res[0], want, dtype)
            if res[0]["iterations"] == want["iterations"]:
                assert res[0]["rho"] == pytest.approx(want["info"]["rho_final"], rel=1e-6)
    # a wide dense handle (m <= n: transposed storage)
    Aw = np.random.default_rng(3).standard_normal((50, 90))
    fw, gw = PROBLEMS["lasso"](np.ones(50), 90)
    with _pogs().Solver(Aw, dtype=dtype) as s:
        rc, msg, _, out = _raw(s, [fw], [gw], x0=np.zeros((1, 90)), l0=np.zeros((1, 50)))
        assert rc == 6 and "m > n" in msg
        assert _untouched(out)
        assert s.solve(fw, gw)["status"] == 0


def test_sparse_handles_take_the_same_entry_and_refuse_alike():
    dtype = np.float64
    name = "sparse_wide_cgls"
    x0, l0, rho = _start_of(_oracle_solve(name, dtype, 0.4))
    f, g = _fg(name, 0.3)
    want = _oracle_solve(name, dtype, 0.3, start=(x0, l0, rho))
    with _solver(name, dtype) as s:
        for label, kw in {"x0 alone": dict(x0=x0[None]), "flags without x0": dict(warm=[1])}.items():
            rc, msg, _, out = _raw(s, [f], [g], **kw)
            assert rc == 6 and msg and _untouched(out), label
        rc, msg, res, _ = _raw(s, [f], [g], rho=[rho], x0=x0[None], l0=l0[None])
        assert rc == 0, msg
        _check_member(name, 0.3, res[0], want, dtype)
