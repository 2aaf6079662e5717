"""GPU tests of ragged many-problem solves (pogs_amd.solve_many_ragged / PogsAmdSolveManyRaggedFn and
ManySolver.from_ragged / PogsAmdManyCreateRagged): k problems, each with its own shape, in one call.  The yardstick is
the uniform entry: problem j solved alone by solve_many(A_j[None], ...) is what problem j must return byte for byte,
whatever its position, its neighbours, the input layout and the chunking of the call."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
from helpers import PROBLEMS, _fsum, fn_arrays, objective, relerr, soa

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]

# (shape, family, seed): the README recipe (RandomState(seed): A = randn(m, n), b = randn(m)) with one seed per member.
# Every member stops with status 0 at the default tolerances in the CPU oracle, in fp64 and in fp32 with the same
# iteration count (checked for seeds 0..7 of each shape before these were fixed).
MEMBERS = [
    ((7, 3), "lasso", 1),          # tall; m n = 21 is odd: the next matrix starts at an odd element offset
    ((3, 7), "lasso", 4),          # wide
    ((5, 5), "lasso", 5),          # square: the wide branch
    ((1, 4), "lasso", 5),          # one row
    ((4, 1), "lasso", 1),          # one column
    ((130, 64), "lasso", 1),       # one Gram tile next to ...
    ((64, 130), "lasso", 4),       # ... problems with more: the early return of the Gram grid
    ((300, 129), "huber", 1),      # three Gram tiles (129 > 128), past the n <= 128 column sums
    ((200, 128), "logistic", 1),   # n = 128: the interleaved column sums
    ((70, 257), "lasso", 2),       # wide, a ragged last tile
]
ORACLE_MEMBERS = (5, 6, 2)         # tall, wide, square


def _pogs():
    import pogs_amd

    return pogs_amd


@functools.lru_cache(maxsize=None)
def _problems():
    """[(A, f, g)] of MEMBERS, fp64 data; never modified."""
    out = []
    for (m, n), name, seed in MEMBERS:
        rs = np.random.RandomState(seed)
        A = rs.randn(m, n)
        b = rs.randn(m)
        f, g = PROBLEMS[name](b, n)
        A.setflags(write=False)
        out.append((A, f, g))
    return out


def _lists():
    P = _problems()
    return [p[0] for p in P], [p[1] for p in P], [p[2] for p in P]


def _packed(mats, order, dtype):
    """(one packed host array with every matrix in `order`, the shapes): `ord` is stated, never inferred."""
    return np.concatenate([a.ravel(order=order) for a in mats]).astype(dtype), [a.shape for a in mats]


def _member(res, j):
    out = {"x": res["x"][j], "y": res["y"][j], "l": res["l"][j], "mu": res["mu"][j], "optval": float(res["optval"][j]),
           "iterations": int(res["iterations"][j]), "status": int(res["status"][j])}
    if "rho" in res:
        out["rho"] = float(res["rho"][j])
    return out


def _same_bytes(r1, r2):
    for k in ("x", "y", "l", "mu"):
        assert r1[k].dtype == r2[k].dtype and r1[k].shape == r2[k].shape, k
        assert r1[k].tobytes() == r2[k].tobytes(), k
    assert np.float64(r1["optval"]).tobytes() == np.float64(r2["optval"]).tobytes()
    assert r1["iterations"] == r2["iterations"] and r1["status"] == r2["status"]
    if "rho" in r1 and "rho" in r2:
        assert np.float64(r1["rho"]).tobytes() == np.float64(r2["rho"]).tobytes()


@functools.lru_cache(maxsize=None)
def _alone(dtype):
    """Each member alone through the uniform entry: the bytes every ragged result is held to."""
    pogs = _pogs()
    out = []
    for A, f, g in _problems():
        out.append(_member(pogs.solve_many(A[None], [f], [g], dtype=dtype), 0))
    for r in out:
        assert r["status"] == 0
    return out


@functools.lru_cache(maxsize=None)
def _ragged(dtype):
    mats, fs, gs = _lists()
    return _pogs().solve_many_ragged(mats, fs, gs, dtype=dtype)


# ---- 1: bytes, one-shot -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_bytes_are_each_member_alone(dtype, order, monkeypatch):
    pogs = _pogs()
    mats, fs, gs = _lists()
    k = len(mats)
    want = _alone(dtype)
    seen = []
    real = pogs.graph.lib.PogsAmdSolveManyRaggedFn
    monkeypatch.setattr(pogs.graph.lib, "PogsAmdSolveManyRaggedFn", lambda *a: (seen.append(a[1]), real(*a))[1])
    want_ord = int(pogs.Ordering.ROW_MAJ if order == "C" else pogs.Ordering.COL_MAJ)
    flat, shapes = _packed(mats, order, dtype)
    got = pogs.solve_many_ragged(flat, fs, gs, dtype=dtype, shapes=shapes, order=order)
    assert len(got) == k
    for j in range(k):
        m, n = MEMBERS[j][0]
        assert got[j]["x"].shape == (n,) and got[j]["y"].shape == (m,) and got[j]["x"].dtype == dtype
        _same_bytes(got[j], want[j])
    flat_r, shapes_r = _packed(mats[::-1], order, dtype)
    rev = pogs.solve_many_ragged(flat_r, fs[::-1], gs[::-1], dtype=dtype, shapes=shapes_r, order=order)
    for j in range(k):
        _same_bytes(rev[k - 1 - j], want[j])
    # a workspace cap of 1 MB: the call splits into chunks packed by each problem's own footprint
    monkeypatch.setenv("POGS_AMD_MANY_WORKSPACE_MB", "1")
    chunked = pogs.solve_many_ragged(flat, fs, gs, dtype=dtype, shapes=shapes, order=order)
    monkeypatch.delenv("POGS_AMD_MANY_WORKSPACE_MB")
    for j in range(k):
        _same_bytes(chunked[j], want[j])
    # the list form: C-ordered members go row-major, Fortran-ordered ones column-major, and the one-row and
    # one-column members (contiguous both ways) do not turn the list row-major
    as_list = [np.asfortranarray(a) for a in mats] if order == "F" else mats
    assert as_list[3].flags.c_contiguous and as_list[3].flags.f_contiguous
    listed = pogs.solve_many_ragged(as_list, fs, gs, dtype=dtype)
    for j in range(k):
        _same_bytes(listed[j], want[j])
    assert seen == [want_ord] * 4, seen


# ---- 2: device-resident A -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_device_resident_input(dtype):
    import torch

    pogs = _pogs()
    mats, fs, gs = _lists()
    host = _ragged(dtype)
    flat = np.concatenate([a.ravel() for a in mats]).astype(dtype)
    At = torch.from_numpy(flat.copy()).to("cuda")
    before = At.clone()
    dev = pogs.solve_many_ragged(At, fs, gs, dtype=dtype, shapes=[a.shape for a in mats])
    torch.cuda.synchronize()
    assert torch.equal(At, before)
    # column-major members in one packed tensor
    flat_f = np.concatenate([a.ravel(order="F") for a in mats]).astype(dtype)
    Af = torch.from_numpy(flat_f).to("cuda")
    dev_f = pogs.solve_many_ragged(Af, fs, gs, dtype=dtype, shapes=[a.shape for a in mats], order="F")
    # a list of device tensors is packed on the device
    tens = [torch.from_numpy(a.astype(dtype)).to("cuda") for a in mats]
    dev_l = pogs.solve_many_ragged(tens, fs, gs, dtype=dtype)
    for j in range(len(mats)):
        for other in (dev, dev_f, dev_l):
            _same_bytes(other[j], host[j])


# ---- 3: oracle ------------------------------------------------------------------------------------------------------

def _xtol32(got_iters, want_iters, loose=2e-4):
    """tests/test_gpu_many.py: the suite's fp32 bar against the oracle."""
    d = abs(int(got_iters) - int(want_iters))
    return 2e-5 if d == 0 else min(loose, 1e-4 * (1 + d))


def _check(A, f, g, got, want, dtype):
    """tests/test_gpu_many.py: _check, restated with its tolerances."""
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


@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_members_against_the_oracle(dtype):
    got = _ragged(dtype)
    P = _problems()
    for j in ORACLE_MEMBERS:
        A, f, g = P[j]
        want = ob.oracle_solve(A, soa(f), soa(g), dtype=dtype)
        print("member %d %s: iterations %d (oracle %d), x %.2e" % (j, MEMBERS[j][0], got[j]["iterations"],
                                                                   want["iterations"], relerr(got[j]["x"], want["x"])))
        _check(A, f, g, got[j], want, dtype)


# ---- 4: the handle --------------------------------------------------------------------------------------------------

def _second(P):
    """The second solve's functions: every member a lasso at lambda = 0.3 on its own b (f's b of the first solve)."""
    pogs = _pogs()
    fs, gs = [], []
    for (A, f, g), ((m, n), _, seed) in zip(P, MEMBERS):
        rs = np.random.RandomState(seed)
        rs.randn(m, n)
        f2, g2 = pogs.graph.lasso_functions(rs.randn(m), 0.3, n)
        fs.append(f2)
        gs.append(g2)
    return fs, gs


@functools.lru_cache(maxsize=None)
def _handle_sequence(dtype):
    """cold (first functions) -> last (second functions) on a ragged handle, run twice on one handle, then `given`
    with the cold step's outputs: (cold, last, cold again, last again, given)."""
    pogs = _pogs()
    mats, fs, gs = _lists()
    fs2, gs2 = _second(_problems())
    with pogs.ManySolver.from_ragged(mats, dtype=dtype) as s:
        cold = s.solve(fs, gs)
        last = s.solve(fs2, gs2, start="last")
        cold2 = s.solve(fs, gs)
        last2 = s.solve(fs2, gs2, start="last")
        given = s.solve(fs2, gs2, start="warm", x0=cold["x"], l0=cold["l"], rho=cold["rho"])
    return cold, last, cold2, last2, given


@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_handle_cold_is_the_one_shot_call(dtype):
    cold = _handle_sequence(dtype)[0]
    want = _ragged(dtype)
    alone = _alone(dtype)
    assert isinstance(cold["x"], list) and len(cold["x"]) == len(MEMBERS)
    for j in range(len(MEMBERS)):
        got = _member(cold, j)
        got.pop("rho")
        _same_bytes(got, want[j])
        _same_bytes(got, alone[j])


@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_handle_last_is_each_member_on_its_own_handle(dtype):
    pogs = _pogs()
    cold, last, cold2, last2, given = _handle_sequence(dtype)
    P = _problems()
    fs2, gs2 = _second(P)
    for j, (A, f, g) in enumerate(P):
        with pogs.ManySolver(A[None], dtype=dtype) as u:
            u_cold = u.solve([f], [g])
            u_last = u.solve([fs2[j]], [gs2[j]], start="last")
        _same_bytes(_member(cold, j), _member(u_cold, 0))
        _same_bytes(_member(last, j), _member(u_last, 0))
    for j in range(len(P)):
        # two identical sequences, identical bytes; `given` with the cold step's x, l and rho is `last`
        _same_bytes(_member(cold2, j), _member(cold, j))
        _same_bytes(_member(last2, j), _member(last, j))
        _same_bytes(_member(given, j), _member(last, j))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_handle_from_column_major_input(dtype, monkeypatch):
    """from_ragged over column-major host input (packed with order="F", and a list of Fortran-ordered members), the
    first created in upload chunks of 0.25 MB: cold and last return the row-major handle's bytes."""
    pogs = _pogs()
    mats, fs, gs = _lists()
    fs2, gs2 = _second(_problems())
    cold, last = _handle_sequence(dtype)[:2]
    seen = []
    real = pogs.graph.lib.PogsAmdManyCreateRagged
    monkeypatch.setattr(pogs.graph.lib, "PogsAmdManyCreateRagged", lambda *a: (seen.append(a[2]), real(*a))[1])
    flat, shapes = _packed(mats, "F", dtype)
    monkeypatch.setenv("POGS_AMD_MANY_WORKSPACE_MB", "0.25")
    s1 = pogs.ManySolver.from_ragged(flat, dtype=dtype, shapes=shapes, order="F")
    monkeypatch.delenv("POGS_AMD_MANY_WORKSPACE_MB")
    s2 = pogs.ManySolver.from_ragged([np.asfortranarray(a) for a in mats], dtype=dtype)
    assert seen == [int(pogs.Ordering.COL_MAJ)] * 2, seen
    for s in (s1, s2):
        with s:
            c = s.solve(fs, gs)
            la = s.solve(fs2, gs2, start="last")
        for j in range(len(mats)):
            _same_bytes(_member(c, j), _member(cold, j))
            _same_bytes(_member(la, j), _member(last, j))


def test_ragged_handle_created_in_upload_chunks(monkeypatch):
    """A staging cap of 0.25 MB: create uploads the fp64 members in four chunks (the 300 x 129 member alone is larger
    than the cap and still gets its chunk); the cold solve is unchanged."""
    pogs = _pogs()
    mats, fs, gs = _lists()
    monkeypatch.setenv("POGS_AMD_MANY_WORKSPACE_MB", "0.25")
    s = pogs.ManySolver.from_ragged(mats, dtype=np.float64)
    monkeypatch.delenv("POGS_AMD_MANY_WORKSPACE_MB")
    with s:
        got = s.solve(fs, gs)
    want = _alone(np.float64)
    for j in range(len(mats)):
        r = _member(got, j)
        r.pop("rho")
        _same_bytes(r, want[j])


# ---- 5: handle metadata ---------------------------------------------------------------------------------------------

def test_handle_shapes_and_info():
    pogs = _pogs()
    mats, fs, gs = _lists()
    shapes = [s for s, _, _ in MEMBERS]
    with pogs.ManySolver.from_ragged(mats, dtype=np.float32) as s:
        assert s.get_shapes() == shapes and s.shapes == shapes
        info = s.info()
        assert (info["k"], info["m"], info["n"]) == (len(shapes), 300, 257)
        assert (s.k, s.m, s.n) == (len(shapes), 300, 257)
        assert info["resident_bytes"] > 4 * sum(m * n for m, n in shapes)
    with pogs.ManySolver(np.ones((3, 6, 4)) + np.arange(24).reshape(6, 4) % 5, dtype=np.float32) as u:
        assert u.get_shapes() == [(6, 4)] * 3
        info = u.info()
        assert (info["k"], info["m"], info["n"]) == (3, 6, 4)


# ---- 6: refusals ----------------------------------------------------------------------------------------------------

def _raw_handle_solve(s, fs, gs, start, x_null=False):
    """PogsAmdManySolveFn on the handle of `s` as given: (return code, last error, x, iterations, status)."""
    from pogs_amd import _lib

    k = s.k
    fa, ga, keep = fn_arrays(fs, gs, s.dtype)
    x = np.full(sum(n for _, n in s.shapes), 7.0, s.dtype)
    y = np.full(sum(m for m, _ in s.shapes), 7.0, s.dtype)
    it = np.full(k, 77, np.uint32)
    st = np.full(k, 55, np.int32)
    rc = _lib.lib.PogsAmdManySolveFn(s._h, fa, ga, None, start, None, None, 1e-4, 1e-4, 2500, 0, 1, 1,
                                     None if x_null else x.ctypes.data, y.ctypes.data, None, None, None, it.ctypes.data,
                                     st.ctypes.data, None)
    return rc, _lib.last_error(), x, y, it, st


def test_refused_handle_solves_write_nothing():
    pogs = _pogs()
    dtype = np.float64
    mats, fs, gs = _lists()
    want = _alone(dtype)
    with pogs.ManySolver.from_ragged(mats, dtype=dtype) as s:
        for start, x_null, msg in ((2, False, "before the handle's first solve"), (0, True, "must not be NULL"),
                                   (9, False, "unknown start")):
            rc, err, x, y, it, st = _raw_handle_solve(s, fs, gs, start, x_null)
            assert rc == 6 and msg in err, err
            assert np.all(x == 7.0) and np.all(y == 7.0) and np.all(it == 77) and np.all(st == 55)
        with pytest.raises(RuntimeError, match="before the handle's first solve"):
            s.solve(fs, gs, start="last")
        got = s.solve(fs, gs)
        for j in range(len(mats)):
            r = _member(got, j)
            r.pop("rho")
            _same_bytes(r, want[j])
        # refusals after a solve leave the kept solution as it was: `last` still follows the cold step
        fs2, gs2 = _second(_problems())
        for start, x_null in ((0, True), (9, False)):
            rc, err, x, y, it, st = _raw_handle_solve(s, fs2, gs2, start, x_null)
            assert rc == 6 and np.all(x == 7.0) and np.all(it == 77)
        last = s.solve(fs2, gs2, start="last")
    ref = _handle_sequence(dtype)[1]
    for j in range(len(mats)):
        _same_bytes(_member(last, j), _member(ref, j))


# ---- 7: a uniform list through the ragged entry ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_uniform_problems_through_the_ragged_entry(dtype):
    pogs = _pogs()
    mats, fs, gs = [], [], []
    for seed in range(4):
        rs = np.random.RandomState(40 + seed)
        A = rs.randn(20, 10)
        f, g = PROBLEMS["lasso"](rs.randn(20), 10)
        mats.append(A)
        fs.append(f)
        gs.append(g)
    want = pogs.solve_many(np.stack(mats), fs, gs, dtype=dtype)
    got = pogs.solve_many_ragged(mats, fs, gs, dtype=dtype)
    for j in range(4):
        w = _member(want, j)
        assert w["status"] == 0
        _same_bytes(got[j], w)
