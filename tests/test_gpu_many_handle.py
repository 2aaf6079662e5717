"""GPU tests of the persistent many-problem handle (pogs_amd.ManySolver / PogsAmdManyCreate, PogsAmdManySolveFn): k
problems set up once and re-solved cold, from a given (x0, l0) or from their own last solution and rho.  A cold solve
on the handle must return the one-shot call's bytes, a warm start must follow the oracle's SetInitX + SetInitLambda
trajectory, `last` must be `given` with the previous step's outputs, and a member's bytes must stay its own."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
from helpers import PROBLEMS, _fsum, fn_arrays, objective, relerr, soa

pytestmark = pytest.mark.gpu

SHAPES = [(120, 60), (50, 90)]
# Seeds whose fp32 oracle solves match the fp64 ones (tests/test_gpu_many.py: SEEDS).
SEEDS = {(120, 60): (1, 5, 8), (50, 90): (2, 3, 5)}
DTYPES = [np.float64, np.float32]
FIRST = ("lasso", "svm", "logistic")      # test 1: the families of each seed's three members
SECOND = ("huber", "lasso", "svm")        # test 2: what each of them is switched to


def _pogs():
    import pogs_amd

    return pogs_amd


# ---- the bars, restated (tests/test_gpu_many.py: _xtol32, _check, _same_bytes, _data) -----------------------------

def _xtol32(got_iters, want_iters, loose=2e-4):
    """The suite's fp32 bar against the oracle: 2e-5 at the same iteration count, else 1e-4 per iteration apart,
    capped at 2e-4."""
    d = abs(int(got_iters) - int(want_iters))
    return 2e-5 if d == 0 else min(loose, 1e-4 * (1 + d))


def _check(A, f, g, got, want, dtype):
    """Same status; iterations within 2 (fp64) or max(3, 10 %) (fp32); x and y within 1e-6 (fp64) or the fp32 bar;
    the dual within 10x that on the scale of y; optval, optval against sum f(y) + sum g(x) in numpy, and the true
    objective at x within 5 % of optval."""
    tight = dtype == np.float64
    assert got["status"] == want["status"]
    it_g, it_w = got["iterations"], want["iterations"]
    if want["status"] != 0:
        assert it_g == it_w
        return
    slack = 2 if tight else max(3, int(0.1 * it_w))
    assert abs(it_g - it_w) <= slack, (it_g, it_w)
    xtol = 1e-6 if tight else _xtol32(it_g, it_w)
    assert relerr(got["x"], want["x"]) < xtol
    assert relerr(got["y"], want["y"]) < xtol
    l_scale = max(np.linalg.norm(want["l"]), 1e-2 * np.linalg.norm(want["y"]))
    assert np.linalg.norm(got["l"].astype(np.float64) - want["l"]) / l_scale < 10 * xtol
    otol = 1e-7 if tight else _xtol32(it_g, it_w)
    assert got["optval"] == pytest.approx(want["optval"], rel=otol, abs=1e-9 if tight else 1e-6)
    obj = _fsum(f, got["y"].astype(np.float64)) + _fsum(g, got["x"].astype(np.float64))
    rtol = 1e-9 if tight else 1e-4
    assert obj == pytest.approx(got["optval"], rel=rtol, abs=rtol)
    true_obj = objective(np.asarray(A, np.float64), f, g, got["x"].astype(np.float64))
    assert true_obj == pytest.approx(got["optval"], rel=0.05, abs=1e-2)


def _check_warm(A, f, g, got, want, dtype):
    """A warm-started member against the oracle's warm start: fp64 by _check (iterations within 2); fp32 by the solo
    warm-start test's bars (test_gpu_dense.test_warm_start_lambda_path_matches_oracle): status equal, iterations
    within max(3, 10 %), x within 2e-3, l within 2e-2."""
    print("warm: iterations %d (oracle %d), x %.2e, l %.2e" % (got["iterations"], want["iterations"],
                                                              relerr(got["x"], want["x"]), relerr(got["l"], want["l"])))
    if dtype == np.float64:
        _check(A, f, g, got, want, dtype)
        return
    assert got["status"] == want["status"]
    assert abs(int(got["iterations"]) - int(want["iterations"])) <= max(3, int(want["iterations"]) // 10)
    assert relerr(got["x"], want["x"]) < 2e-3
    assert relerr(got["l"], want["l"]) < 2e-2


def _member(res, j):
    out = {"x": res["x"][j], "y": res["y"][j], "l": res["l"][j], "mu": res["mu"][j], "optval": float(res["optval"][j]),
           "iterations": int(res["iterations"][j]), "status": int(res["status"][j])}
    if "rho" in res:
        out["rho"] = float(res["rho"][j])
    return out


def _same_bytes(r1, r2):
    for k in ("x", "y", "l", "mu"):
        assert r1[k].tobytes() == r2[k].tobytes(), k
    assert np.float64(r1["optval"]).tobytes() == np.float64(r2["optval"]).tobytes()
    assert r1["iterations"] == r2["iterations"] and r1["status"] == r2["status"]
    if "rho" in r1 and "rho" in r2:
        assert np.float64(r1["rho"]).tobytes() == np.float64(r2["rho"]).tobytes()


def _same_call(res1, res2, k):
    for j in range(k):
        _same_bytes(_member(res1, j), _member(res2, j))


def _data(m, n, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    b = A @ (rng.standard_normal(n) * (rng.random(n) < 0.2)) + 0.1 * rng.standard_normal(m)
    return A, b


def _family_call(shape, names):
    """(A stack, fs, gs, per-member (A, f, g)) of len(SEEDS[shape]) x len(names) problems of one shape."""
    m, n = shape
    mats, fs, gs, members = [], [], [], []
    for s in SEEDS[shape]:
        A, b = _data(m, n, s)
        for name in names:
            f, g = PROBLEMS[name](b, n)
            mats.append(A)
            fs.append(f)
            gs.append(g)
            members.append((A, f, g))
    return np.stack(mats), fs, gs, members


def _lassos(shape, frac):
    """The lasso members of a shape at lambda = frac * max|A^T b|: (A stack, fs, gs, per-member (A, f, g))."""
    pogs = _pogs()
    m, n = shape
    mats, fs, gs, members = [], [], [], []
    for s in SEEDS[shape]:
        A, b = _data(m, n, s)
        f, g = pogs.graph.lasso_functions(b, frac * np.max(np.abs(A.T @ b)), n)
        mats.append(A)
        fs.append(f)
        gs.append(g)
        members.append((A, f, g))
    return np.stack(mats), fs, gs, members


# ---- tests 1, 2, 8: one handle per (shape, dtype), its solves computed once -----------------------------------------

@functools.lru_cache(maxsize=None)
def _cold_runs(shape, dtype):
    """The one-shot call on the nine members of test 1 and, on ONE handle: the same functions cold, every member
    switched to another family cold, and the first functions cold again."""
    pogs = _pogs()
    A, fs, gs, members = _family_call(shape, FIRST)
    _, fs2, gs2, members2 = _family_call(shape, SECOND)
    one_shot = pogs.solve_many(A, fs, gs, dtype=dtype)
    with pogs.ManySolver(A, dtype=dtype) as s:
        first = s.solve(fs, gs)
        other = s.solve(fs2, gs2)
        again = s.solve(fs, gs, start="cold")
        info = s.info()
    return dict(A=A, fs=fs, gs=gs, members=members, members2=members2, one_shot=one_shot, first=first, other=other,
                again=again, info=info)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_cold_on_the_handle_is_the_one_shot_call(shape, dtype):
    r = _cold_runs(shape, dtype)
    k = len(r["fs"])
    assert k == 9 and r["first"]["x"].shape == (k, shape[1]) and r["first"]["y"].shape == (k, shape[0])
    _same_call(r["one_shot"], r["first"], k)
    _same_call(r["one_shot"], r["again"], k)      # after a solve with other functions: the reset is complete
    assert np.all(r["first"]["rho"] > 0) and r["first"]["rho"].tobytes() == r["again"]["rho"].tobytes()
    info = r["info"]
    assert (info["k"], info["m"], info["n"]) == (k,) + shape
    assert info["dtype"] == (1 if dtype == np.float64 else 0)
    assert info["resident_bytes"] >= r["A"].size * np.dtype(dtype).itemsize and info["setup_s"] > 0
    assert info["problem_iters"] == int(np.sum(r["again"]["iterations"] + 1)) and info["launches"] >= 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_resolve_with_new_functions_against_the_oracle(shape, dtype):
    r = _cold_runs(shape, dtype)
    for j, (Aj, f, g) in enumerate(r["members2"]):
        want = ob.oracle_solve(Aj, soa(f), soa(g), dtype=dtype)
        _check(Aj, f, g, _member(r["other"], j), want, dtype)


# ---- test 3: warm, given, against the oracle's warm start ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_path(shape, dtype):
    """Per lasso member of the shape, the oracle's solves (CPU only): first at 0.3 lambda_max; second at 0.2
    lambda_max cold, warm from the first (x, l) at rho = 1, and warm at the first solve's final rho."""
    _, _, _, m1 = _lassos(shape, 0.3)
    _, _, _, m2 = _lassos(shape, 0.2)
    out = []
    for (A, f1, g1), (_, f2, g2) in zip(m1, m2):
        first = ob.oracle_solve(A, soa(f1), soa(g1), dtype=dtype)
        rho1 = first["info"]["rho_final"]
        out.append(dict(
            first=first, rho1=rho1, cold=ob.oracle_solve(A, soa(f2), soa(g2), dtype=dtype),
            warm=ob.oracle_solve(A, soa(f2), soa(g2), dtype=dtype, x0=first["x"], l0=first["l"]),
            warm_rho=ob.oracle_solve(A, soa(f2), soa(g2), dtype=dtype, x0=first["x"], l0=first["l"], rho=rho1)))
    return out


def _kept_members(shape):
    """The conditions on the inputs, on the CPU with the oracle alone: the fp32 and fp64 oracle iteration counts agree
    on every solve of the member, and the oracle's warm-and-rho count is below its cold count."""
    p64, p32 = _oracle_path(shape, np.float64), _oracle_path(shape, np.float32)
    kept = []
    for j, (a, b) in enumerate(zip(p64, p32)):
        agree = all(a[k]["iterations"] == b[k]["iterations"] and a[k]["status"] == b[k]["status"] == 0
                    for k in ("first", "cold", "warm", "warm_rho"))
        faster = all(p[j]["warm_rho"]["iterations"] < p[j]["cold"]["iterations"] for p in (p64, p32))
        print(shape, SEEDS[shape][j], {k: (a[k]["iterations"], b[k]["iterations"]) for k in ("first", "cold", "warm",
                                                                                              "warm_rho")})
        if agree and faster:
            kept.append(j)
    return kept


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_warm_given_follows_the_oracles_warm_start(shape, dtype):
    pogs = _pogs()
    kept = _kept_members(shape)
    assert kept == [0, 1, 2], kept          # all six lasso rows meet the conditions: no member may be dropped
    path = _oracle_path(shape, dtype)
    A, fs2, gs2, members = _lassos(shape, 0.2)
    x0 = np.stack([p["first"]["x"] for p in path])
    l0 = np.stack([p["first"]["l"] for p in path])
    rho1 = [p["rho1"] for p in path]
    with pogs.ManySolver(A, dtype=dtype) as s:
        cold = s.solve(fs2, gs2)
        warm = s.solve(fs2, gs2, start="warm", x0=x0, l0=l0, rho=1.0)
        warm_rho = s.solve(fs2, gs2, start="warm", x0=x0, l0=l0, rho=rho1)
        default_rho = s.solve(fs2, gs2, start="warm", x0=x0, l0=l0)       # rho = None means 1.0 each
    _same_call(warm, default_rho, len(fs2))
    for j, (Aj, f, g) in enumerate(members):
        print("member %d: cold %d, warm %d, warm and rho %d" % (j, cold["iterations"][j], warm["iterations"][j],
                                                              warm_rho["iterations"][j]))
        _check(Aj, f, g, _member(cold, j), path[j]["cold"], dtype)
        _check_warm(Aj, f, g, _member(warm, j), path[j]["warm"], dtype)
        _check_warm(Aj, f, g, _member(warm_rho, j), path[j]["warm_rho"], dtype)
        assert warm_rho["iterations"][j] < cold["iterations"][j]


# ---- tests 4, 5: chains -----------------------------------------------------------------------------------------------

FRACS = (0.3, 0.2, 0.1)


def _chain_last(s, steps):
    """steps: [(fs, gs)]; cold, then start="last" with rho=None."""
    out = []
    for i, (fs, gs) in enumerate(steps):
        out.append(s.solve(fs, gs) if i == 0 else s.solve(fs, gs, start="last"))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_last_is_given_with_the_previous_outputs(shape, dtype):
    pogs = _pogs()
    A = _lassos(shape, 0.3)[0]
    steps = [_lassos(shape, fr)[1:3] for fr in FRACS]
    k = len(steps[0][0])
    with pogs.ManySolver(A, dtype=dtype) as s:
        last = _chain_last(s, steps)
        given = [s.solve(*steps[0])]
        for fs, gs in steps[1:]:
            prev = given[-1]
            given.append(s.solve(fs, gs, start="warm", x0=prev["x"], l0=prev["l"], rho=prev["rho"]))
    for a, b in zip(last, given):
        assert np.all(a["status"] == 0)
        _same_call(a, b, k)
    # the chain is warm: fewer problem-iterations in its second and third steps than in its cold first step
    assert int(np.sum(last[1]["iterations"])) < int(np.sum(last[0]["iterations"]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_members_bytes_are_its_own_through_a_chain(dtype):
    pogs = _pogs()
    shape = (120, 60)
    m, n = shape
    A, b = _data(m, n, 1)
    lam_max = np.max(np.abs(A.T @ b))
    mine = [pogs.graph.lasso_functions(b, fr * lam_max, n) for fr in FRACS]
    names = [nm for nm in PROBLEMS if nm != "lasso"]
    others = []
    for j in range(11):
        Aj, bj = _data(m, n, 700 + j)
        others.append((Aj,) + tuple(PROBLEMS[names[j % len(names)]](bj, n)))

    def run(pos, with_others):
        rest = others if with_others else []
        mats = [o[0] for o in rest]
        mats.insert(pos, A)
        steps = []
        for f, g in mine:
            fs, gs = [o[1] for o in rest], [o[2] for o in rest]
            fs.insert(pos, f)
            gs.insert(pos, g)
            steps.append((fs, gs))
        with pogs.ManySolver(np.stack(mats), dtype=dtype) as s:
            return [_member(r, pos) for r in _chain_last(s, steps)]

    alone, first, mid = run(0, False), run(0, True), run(7, True)
    for a, b1, b2 in zip(alone, first, mid):
        assert a["status"] == 0
        _same_bytes(a, b1)
        _same_bytes(a, b2)


# ---- test 6: per-member stopping when warm ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_per_member_stopping_when_warm(dtype):
    pogs = _pogs()
    shape = (120, 60)
    path = _oracle_path(shape, dtype)
    A, fs2, gs2, members = _lassos(shape, 0.2)
    # member 0 from its own converged (x, l, rho) at this lambda; members 1 and 2 from the other lambda's solution
    done = path[0]["cold"]
    x0 = np.stack([done["x"], path[1]["first"]["x"], path[2]["first"]["x"]])
    l0 = np.stack([done["l"], path[1]["first"]["l"], path[2]["first"]["l"]])
    rho = [done["info"]["rho_final"], path[1]["rho1"], path[2]["rho1"]]
    want0 = ob.oracle_solve(members[0][0], soa(fs2[0]), soa(gs2[0]), dtype=dtype, x0=done["x"], l0=done["l"], rho=rho[0])
    assert want0["status"] == 0 and want0["iterations"] <= 1
    with pogs.ManySolver(A, dtype=dtype) as s:
        got = s.solve(fs2, gs2, start="warm", x0=x0, l0=l0, rho=rho)
    print("iterations", got["iterations"], "oracle", want0["iterations"], [p["warm_rho"]["iterations"] for p in path[1:]])
    assert got["status"][0] == 0 and got["iterations"][0] <= 1
    for j in (1, 2):
        Aj, f, g = members[j]
        _check_warm(Aj, f, g, _member(got, j), path[j]["warm_rho"], dtype)


# ---- test 7: the handle owns its copy --------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("colmajor", [False, True])
def test_the_handle_owns_its_copy_of_a_device_tensor(dtype, colmajor):
    import torch

    pogs = _pogs()
    shape = (120, 60)
    r = _cold_runs(shape, dtype)
    k = len(r["fs"])
    A = r["A"].astype(dtype)
    if colmajor:
        At = torch.from_numpy(np.ascontiguousarray(A.transpose(0, 2, 1))).to("cuda").transpose(1, 2)
        assert not At.is_contiguous() and At.stride() == (shape[0] * shape[1], 1, shape[0])
    else:
        At = torch.from_numpy(A.copy()).to("cuda")
    before = At.clone()
    with pogs.ManySolver(At, dtype=dtype) as s:
        torch.cuda.synchronize()
        assert torch.equal(At, before)            # read, never written
        At.zero_()                                # never referenced afterwards
        torch.cuda.synchronize()
        got = s.solve(r["fs"], r["gs"])
    _same_call(r["one_shot"], got, k)


# ---- test 8: refusals -------------------------------------------------------------------------------------------------

def _raw_solve(s, fs, gs, start, x0=None, l0=None, x_null=False, it_null=False, st_null=False, f_null=False):
    """PogsAmdManySolveFn as given (no Python checks) with sentinel-filled outputs: (return code, last error, outputs)."""
    from pogs_amd import _lib

    k, m, n, dt = s.k, s.m, s.n, s.dtype
    fa, ga, keep = fn_arrays(fs, gs, dt)
    out = dict(x=np.full((k, n), 7.0, dt), y=np.full((k, m), 7.0, dt), l=np.full((k, m), 7.0, dt),
               mu=np.full((k, n), 7.0, dt), optval=np.full(k, 7.0), it=np.full(k, 77, np.uint32),
               st=np.full(k, 55, np.int32), rho=np.full(k, 7.0))
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = _lib.lib.PogsAmdManySolveFn(s._h, None if f_null else fa, ga, None, start, p(x0), p(l0), 1e-4, 1e-4, 2500, 0, 1,
                                     1, None if x_null else p(out["x"]), p(out["y"]), p(out["l"]), p(out["mu"]),
                                     p(out["optval"]), None if it_null else p(out["it"]),
                                     None if st_null else p(out["st"]), p(out["rho"]))
    return rc, _lib.last_error(), out


def _untouched(out):
    return all(np.all(out[k] == 7.0) for k in ("x", "y", "l", "mu", "optval", "rho")) and np.all(out["it"] == 77) and \
        np.all(out["st"] == 55)


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_the_handle_as_it_was(dtype, capfd):
    pogs = _pogs()
    shape = (120, 60)
    r = _cold_runs(shape, dtype)
    k = len(r["fs"])
    x0, l0 = np.zeros((k, shape[1]), dtype), np.zeros((k, shape[0]), dtype)
    with pogs.ManySolver(r["A"], dtype=dtype) as s:
        rc, msg, out = _raw_solve(s, r["fs"], r["gs"], 2)                      # "last" before any solve
        assert rc == 6 and "first solve" in msg and _untouched(out)
        with pytest.raises(RuntimeError, match="first solve"):
            s.solve(r["fs"], r["gs"], start="last")
        for _ in range(2):                                                     # before and after the handle's first solve
            for kw in (dict(start=1, x0=x0), dict(start=1, l0=l0), dict(start=1), dict(start=3), dict(start=-1),
                       dict(start=0, x_null=True), dict(start=0, it_null=True), dict(start=0, st_null=True),
                       dict(start=0, f_null=True)):
                rc, msg, out = _raw_solve(s, r["fs"], r["gs"], **kw)
                assert rc == 6 and msg, kw
                assert _untouched(out), kw
            got = s.solve(r["fs"], r["gs"])
            _same_call(r["one_shot"], got, k)
        # a refused call between a solve and a "last" solve does not disturb the kept solution
        fs3, gs3 = r["fs"], r["gs"]
        a = s.solve(fs3, gs3, start="last")
        s.solve(fs3, gs3)
        assert _raw_solve(s, fs3, gs3, 1, x0=x0)[0] == 6
        b = s.solve(fs3, gs3, start="last")
        _same_call(a, b, k)
    capfd.readouterr()


# ---- test 9: the envelope's edge --------------------------------------------------------------------------------------

def test_envelope_edge_fp32():
    """min(m, n) = POGS_AMD_MANY_MIN_DIM_MAX, two members: create plus a cold solve against solve_many's bytes."""
    pogs = _pogs()
    members = []
    for j, name in enumerate(("lasso", "ridge")):
        A, b = _data(700, 512, 31 + j)
        members.append((A,) + tuple(PROBLEMS[name](b, 512)))
    A = np.stack([p[0] for p in members])
    fs, gs = [p[1] for p in members], [p[2] for p in members]
    want = pogs.solve_many(A, fs, gs, dtype=np.float32)
    with pogs.ManySolver(A, dtype=np.float32) as s:
        got = s.solve(fs, gs)
    assert np.all(want["status"] == 0)
    _same_call(want, got, 2)
