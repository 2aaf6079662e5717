"""GPU tests of many-problem solves (pogs_amd.solve_many / PogsAmdSolveManyFn): k independent problems, each with its
own matrix, solved on the device in one call.  Every member is checked against its own oracle solve, and a member's
bytes must not depend on k, its position, the other problems or the chunking of the call."""
import ctypes
import os

import numpy as np
import pytest

import oracle_binding as ob
from helpers import PROBLEMS, _fsum, fn_arrays, objective, relerr, soa
from pogs_amd import synth

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_outputs.npz"))


def _pogs():
    import pogs_amd

    return pogs_amd


def _xtol32(got_iters, want_iters, loose=2e-4):
    """The suite's fp32 bar against the oracle: 2e-5 at the same iteration count, else 1e-4 per iteration apart,
    capped at 2e-4."""
    d = abs(int(got_iters) - int(want_iters))
    return 2e-5 if d == 0 else min(loose, 1e-4 * (1 + d))


def _check(A, f, g, got, want, dtype):
    """The bars of test_gpu_batch._check, restated: same status; iterations within 2 (fp64) or max(3, 10 %) (fp32);
    x and y within 1e-6 (fp64) or the fp32 bar; the dual within 10x that on the scale of y; optval, optval against
    sum f(y) + sum g(x) in numpy, and the true objective at x within 5 % of optval."""
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


def _member(res, j):
    return {"x": res["x"][j], "y": res["y"][j], "l": res["l"][j], "mu": res["mu"][j], "optval": float(res["optval"][j]),
            "iterations": int(res["iterations"][j]), "status": int(res["status"][j])}


def _same_bytes(r1, r2):
    for k in ("x", "y", "l", "mu"):
        assert r1[k].tobytes() == r2[k].tobytes(), k
    assert np.float64(r1["optval"]).tobytes() == np.float64(r2["optval"]).tobytes()
    assert r1["iterations"] == r2["iterations"] and r1["status"] == r2["status"]


def _data(m, n, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    b = A @ (rng.standard_normal(n) * (rng.random(n) < 0.2)) + 0.1 * rng.standard_normal(m)
    return A, b


def _family_call(shape, seeds, names):
    """(A stack, fs, gs, per-member (A, f, g)) of len(seeds) x len(names) problems of one shape."""
    m, n = shape
    mats, fs, gs, members = [], [], [], []
    for s in seeds:
        A, b = _data(m, n, s)
        for name in names:
            f, g = PROBLEMS[name](b, n)
            mats.append(A)
            fs.append(f)
            gs.append(g)
            members.append((A, f, g))
    return np.stack(mats), fs, gs, members


# Seeds whose fp32 oracle solves match the fp64 ones (same iteration counts, x within 1e-5): a member on a knife edge
# of the stopping rule in fp32 (seed 1 at 50 x 90: 7 iterations apart) measures rounding chaos, not the engine.
SEEDS = {(120, 60): (1, 5, 8), (50, 90): (2, 3, 5)}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(120, 60), (50, 90)])
def test_many_families_against_the_oracle(shape, dtype):
    pogs = _pogs()
    A, fs, gs, members = _family_call(shape, SEEDS[shape], list(PROBLEMS))
    got = pogs.solve_many(A, fs, gs, dtype=dtype)
    assert got["x"].shape == (len(fs), shape[1]) and got["y"].shape == (len(fs), shape[0])
    for j, (Aj, f, g) in enumerate(members):
        want = ob.oracle_solve(Aj, soa(f), soa(g), dtype=dtype)
        _check(Aj, f, g, _member(got, j), want, dtype)


@pytest.mark.parametrize("tag,dtype", [("f64", np.float64), ("f32", np.float32)])
def test_many_c1_against_the_compiled_reference(tag, dtype):
    """C1 (np.random.seed(0); A = randn(500, 300); the README lasso) as one member of a 6-problem call."""
    pogs = _pogs()
    A, b, lam = synth.readme_lasso()
    f, g = pogs.graph.lasso_functions(b, lam, 300)
    mats, fs, gs = [], [], []
    for s in range(5):
        As, bs = _data(500, 300, 100 + s)
        fq, gq = PROBLEMS["lasso"](bs, 300)
        mats.append(As)
        fs.append(fq)
        gs.append(gq)
    mats.insert(3, A)
    fs.insert(3, f)
    gs.insert(3, g)
    got = _member(pogs.solve_many(np.stack(mats), fs, gs, dtype=dtype), 3)
    want = {k: GOLD["c1_%s_%s" % (tag, k)] for k in ("x", "y", "l", "optval", "iterations", "status")}
    assert got["status"] == int(want["status"]) == 0
    if dtype == np.float64:
        assert abs(got["iterations"] - 100) <= 2
        assert relerr(got["x"], want["x"]) < 1e-6 and relerr(got["y"], want["y"]) < 1e-6
        assert got["optval"] == pytest.approx(91.76711931681265, rel=1e-7)
    else:
        assert abs(got["iterations"] - int(want["iterations"])) <= 10
        xtol = _xtol32(got["iterations"], want["iterations"])
        assert relerr(got["x"], want["x"]) < xtol and relerr(got["y"], want["y"]) < xtol
        assert got["optval"] == pytest.approx(float(want["optval"]), rel=xtol)


def _mixed(count, m, n, seed0):
    names = list(PROBLEMS)
    mats, fs, gs = [], [], []
    for j in range(count):
        A, b = _data(m, n, seed0 + j)
        f, g = PROBLEMS[names[j % len(names)]](b, n)
        mats.append(A)
        fs.append(f)
        gs.append(g)
    return mats, fs, gs


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_many_member_bytes_are_its_own(dtype, monkeypatch):
    pogs = _pogs()
    m, n = 90, 40
    A, b = _data(m, n, 4242)
    P = PROBLEMS["huber"](b, n)
    mats, fs, gs = _mixed(36, m, n, 500)
    alone = _member(pogs.solve_many(A[None], [P[0]], [P[1]], dtype=dtype), 0)
    first = _member(pogs.solve_many(np.stack([A] + mats), [P[0]] + fs, [P[1]] + gs, dtype=dtype), 0)
    mid_mats = mats[:20] + [A] + mats[20:]
    mid_fs, mid_gs = fs[:20] + [P[0]] + fs[20:], gs[:20] + [P[1]] + gs[20:]
    mid = pogs.solve_many(np.stack(mid_mats), mid_fs, mid_gs, dtype=dtype)
    rev = pogs.solve_many(np.stack(mid_mats[::-1]), mid_fs[::-1], mid_gs[::-1], dtype=dtype)
    # a workspace cap of 1 MB: the 37 problems run in several chunks
    monkeypatch.setenv("POGS_AMD_MANY_WORKSPACE_MB", "1")
    chunked = pogs.solve_many(np.stack(mid_mats), mid_fs, mid_gs, dtype=dtype)
    monkeypatch.delenv("POGS_AMD_MANY_WORKSPACE_MB")
    _same_bytes(alone, first)
    _same_bytes(alone, _member(mid, 20))
    _same_bytes(alone, _member(rev, 16))
    for j in range(37):
        _same_bytes(_member(mid, j), _member(chunked, j))
        _same_bytes(_member(mid, j), _member(rev, 36 - j))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_many_stopping_per_member(dtype):
    pogs = _pogs()
    m, n = 80, 40
    mats = [_data(m, n, 11 + j) for j in range(3)]
    fgs = [PROBLEMS[name](b, n) for (_, b), name in zip(mats, ("ridge", "svm", "lasso"))]
    F = pogs.Function
    # minimize |x|^2 / 2 over y = A x: stops within a few iterations
    quick = (pogs.FunctionVector(m, F.kZero), pogs.FunctionVector(n, F.kSquare))
    # minimize sum y subject to y = A x: unbounded below, so it runs into max_iter
    capped = (pogs.FunctionVector(m, F.kIdentity), pogs.FunctionVector(n, F.kZero))
    wants = [ob.oracle_solve(A, soa(f), soa(g), dtype=dtype) for (A, _), (f, g) in zip(mats, fgs)]
    want_quick = ob.oracle_solve(mats[0][0], soa(quick[0]), soa(quick[1]), dtype=dtype)
    max_iter = max(w["iterations"] for w in wants) + 30
    A = np.stack([a for a, _ in mats] + [mats[0][0], mats[1][0]])
    got = pogs.solve_many(A, [p[0] for p in fgs] + [quick[0], capped[0]], [p[1] for p in fgs] + [quick[1], capped[1]],
                          max_iter=max_iter, dtype=dtype)
    assert list(got["status"]) == [0, 0, 0, 0, 3]
    assert got["iterations"][4] == max_iter - 1
    assert got["iterations"][3] == want_quick["iterations"] < 5
    for j, ((Aj, _), (f, g)) in enumerate(zip(mats, fgs)):
        _check(Aj, f, g, _member(got, j), wants[j], dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_many_rho_adaptive_and_gap_stop(dtype):
    pogs = _pogs()
    m, n = 100, 50
    mats, fs, gs = _mixed(3, m, n, 77)
    rhos = [0.5, 1.0, 3.0]
    A = np.stack(mats)
    for kw in ({"rho": rhos, "adaptive_rho": False}, {"rho": rhos}, {"gap_stop": False}, {"gap_stop": True}):
        got = pogs.solve_many(A, fs, gs, dtype=dtype, **kw)
        for j in range(3):
            want = ob.oracle_solve(mats[j], soa(fs[j]), soa(gs[j]), dtype=dtype,
                                   rho=rhos[j] if "rho" in kw else 1.0, adaptive_rho=kw.get("adaptive_rho", True),
                                   gap_stop=kw.get("gap_stop", True))
            _check(mats[j], fs[j], gs[j], _member(got, j), want, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(70, 33), (45, 45), (37, 101), (200, 1), (1, 30), (130, 65)])
def test_many_shapes(shape, dtype):
    pogs = _pogs()
    m, n = shape
    mats, fs, gs = [], [], []
    for s in range(3):
        A, b = _data(m, n, 900 + s)
        f, g = PROBLEMS[("lasso", "ridge", "huber")[s]](b, n)
        mats.append(A)
        fs.append(f)
        gs.append(g)
    got = pogs.solve_many(np.stack(mats), fs, gs, dtype=dtype)
    for j in range(3):
        want = ob.oracle_solve(mats[j], soa(fs[j]), soa(gs[j]), dtype=dtype)
        _check(mats[j], fs[j], gs[j], _member(got, j), want, dtype)


def test_many_envelope_edge_fp32():
    """min(m, n) = POGS_AMD_MANY_MIN_DIM_MAX, two problems."""
    pogs = _pogs()
    members = []
    for j, name in enumerate(("lasso", "ridge")):
        A, b = _data(700, 512, 31 + j)
        members.append((A,) + tuple(PROBLEMS[name](b, 512)))
    got = pogs.solve_many(np.stack([p[0] for p in members]), [p[1] for p in members], [p[2] for p in members],
                          dtype=np.float32)
    for j, (A, f, g) in enumerate(members):
        want = ob.oracle_solve(A, soa(f), soa(g), dtype=np.float32)
        _check(A, f, g, _member(got, j), want, np.float32)


def _raw_many(k, m, n, A, fs, gs, dtype_code=1, projector=1, x_null=False, it_null=False, st_null=False,
              mem=0):
    """PogsAmdSolveManyFn as given (no Python checks): (return code, last error, x, iterations, status)."""
    from pogs_amd import _lib

    cnt = max(len(fs), 1)
    dt = np.float64 if dtype_code == 1 else np.float32
    fa, ga, keep = fn_arrays(fs, gs, dt)
    x = np.full((cnt, max(n, 1)), 7.0, dt)
    it = np.full(cnt, 77, np.uint32)
    st = np.full(cnt, 55, np.int32)
    opt = _lib.PogsAmdOptions(device=-1, projector=projector)
    a_ptr = A.ctypes.data if isinstance(A, np.ndarray) else A
    rc = _lib.lib.PogsAmdSolveManyFn(dtype_code, 1, k, m, n, a_ptr, mem, ctypes.byref(opt), fa, ga, None, 1e-4, 1e-4,
                                     2500, 0, 1, 1, None if x_null else x.ctypes.data, None, None, None, None,
                                     None if it_null else it.ctypes.data, None if st_null else st.ctypes.data)
    return rc, _lib.last_error(), x, it, st


def test_many_refusals_leave_the_process_usable():
    pogs = _pogs()
    from pogs_amd import FunctionVector

    def fg(m, n):
        return FunctionVector(m, pogs.Function.kSquare, 1.0, 1.0), FunctionVector(n, pogs.Function.kAbs, 1.0, 0.0, 0.1)

    tiny = np.zeros(1)
    for m, n in ((600, 513), (513, 513), (16385, 2), (3, 16385)):
        f, g = fg(m, n)
        rc, msg, x, it, st = _raw_many(1, m, n, tiny, [f], [g])
        assert rc == 6 and msg, (m, n)
        assert np.all(x == 7.0) and np.all(it == 77) and np.all(st == 55)
    A, b = _data(40, 20, 5)
    f, g = PROBLEMS["lasso"](b, 20)
    for kw in ({"x_null": True}, {"it_null": True}, {"st_null": True}, {"dtype_code": 7}, {"projector": 2}):
        rc, msg, x, it, st = _raw_many(1, 40, 20, A, [f], [g], **kw)
        assert rc == 6 and msg, kw
        assert np.all(it == 77) and np.all(st == 55)
    for k in (0, -1):
        rc, msg, x, it, st = _raw_many(k, 40, 20, A, [f], [g])
        assert rc == 6 and msg, k
    assert "direct projector" in _raw_many(1, 40, 20, A, [f], [g], projector=2)[1]
    rc, msg, x, it, st = _raw_many(1, 40, 20, A, [f], [g])
    assert rc == 0 and st[0] == 0
    want = ob.oracle_solve(A, soa(f), soa(g))
    _check(A, f, g, _member(pogs.solve_many(A[None], [f], [g]), 0), want, np.float64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_many_input_layouts_give_the_same_bytes(dtype):
    import torch

    pogs = _pogs()
    mats, fs, gs = _mixed(5, 60, 35, 321)
    A = np.stack(mats).astype(dtype)
    base = pogs.solve_many(A, fs, gs, dtype=dtype)
    fortran = np.asarray(np.moveaxis(np.asfortranarray(np.moveaxis(A, 0, -1)), -1, 0))
    assert not fortran.flags.c_contiguous and fortran.strides[1] == A.itemsize
    as_list = pogs.solve_many(list(A), fs, gs, dtype=dtype)
    col = pogs.solve_many(fortran, fs, gs, dtype=dtype)
    At = torch.from_numpy(A.copy()).to("cuda")
    before = At.clone()
    dev = pogs.solve_many(At, fs, gs, dtype=dtype)
    torch.cuda.synchronize()
    assert torch.equal(At, before)
    for j in range(5):
        for other in (as_list, col, dev):
            _same_bytes(_member(base, j), _member(other, j))


def test_many_scale_512_c1_shaped_fp32():
    """512 C1-shaped problems (the README recipe, seed j for problem j) in one call."""
    pogs = _pogs()
    k, m, n = 512, 500, 300
    A = np.empty((k, m, n), np.float32)
    B = np.empty((k, m))
    for j in range(k):
        rs = np.random.RandomState(j)
        A[j] = rs.randn(m, n)
        B[j] = rs.randn(m)
    fgs = [pogs.graph.lasso_functions(B[j], 0.1, n) for j in range(k)]
    got = pogs.solve_many(A, [p[0] for p in fgs], [p[1] for p in fgs], dtype=np.float32)
    assert np.all(got["status"] == 0)
    for j in (0, 1, 77, 200, 255, 256, 400, 511):
        f, g = fgs[j]
        want = ob.oracle_solve(A[j], soa(f), soa(g), dtype=np.float32)
        _check(A[j], f, g, _member(got, j), want, np.float32)
