"""CPU tests of what the Python boundary hands to the library (pogs_amd/graph.py -> include/pogs_amd.h): every entry
of a multi-problem call is replaced by a recorder that fills plausible outputs and returns 0, and each recorded call is
compared argument by argument: count and order, every scalar, the rho / x0 / l0 / warm arrays read back through the
recorded pointers, each PogsAmdFn field as a pointer or a broadcast value in the solve's dtype, and the containers and
dtypes in which the outputs come back.  Shapes: k = 3; uniform 5 x 3; ragged (3, 2), (1, 4), (5, 5)."""
import ctypes

import numpy as np
import pytest

from pogs_amd import _lib, graph
from pogs_amd.graph import Function, FunctionObj, FunctionVector

DTYPES = [np.float32, np.float64]
K, M, N = 3, 5, 3
RAGGED = [(3, 2), (1, 4), (5, 5)]
OPTS = dict(abs_tol=3e-5, rel_tol=7e-6, max_iter=123, verbose=2, adaptive_rho=False, gap_stop=True)
TAIL = (3e-5, 7e-6, 123, 2, 0, 1)            # OPTS as every entry takes them
FIELDS = "habcde"


# ---- function vectors that mix per-element and broadcast fields ------------------------------------------------------

def _f_spec(m, j):
    return dict(h=int(Function.kSquare), a=1.0, b=np.linspace(-1.0, 1.0, m) + j, c=1.0 + j, d=0.25, e=0.0)


def _g_spec(n, j):
    return dict(h=np.array([int(Function.kAbs), int(Function.kSquare)] * n, np.int32)[:n], a=1.0, b=0.0,
                c=0.1 * (j + 1) + np.arange(n), d=0.0, e=0.5)


def _objs_spec(n):
    """a list of FunctionObj: every field arrives per element"""
    return dict(h=np.full(n, int(Function.kHuber), np.int32), a=np.full(n, 2.0), b=np.arange(n) / 3.0, c=np.full(n, 1.5),
                d=np.zeros(n), e=np.full(n, 0.125))


def _vector(spec, n):
    return FunctionVector(n, **spec)


def _objs(spec, n):
    return [FunctionObj(Function(int(spec["h"][i])), *(spec[k][i] for k in "abcde")) for i in range(n)]


def _pairs(shapes):
    """(fs, gs, f specs, g specs) of len(shapes) problems; the last g is a list of FunctionObj"""
    fsp = [_f_spec(m, j) for j, (m, n) in enumerate(shapes)]
    gsp = [_g_spec(n, j) for j, (m, n) in enumerate(shapes)]
    gsp[-1] = _objs_spec(shapes[-1][1])
    fs = [_vector(s, m) for s, (m, n) in zip(fsp, shapes)]
    gs = [_vector(s, n) for s, (m, n) in zip(gsp[:-1], shapes)] + [_objs(gsp[-1], shapes[-1][1])]
    return fs, gs, fsp, gsp


# ---- reading recorded arguments ---------------------------------------------------------------------------------------

_CT = {np.dtype(np.float32): ctypes.c_float, np.dtype(np.float64): ctypes.c_double, np.dtype(np.int32): ctypes.c_int,
       np.dtype(np.uint32): ctypes.c_uint, np.dtype(np.uintp): ctypes.c_size_t}


def _view(p, dt, count):
    """the `count` elements of `dt` at a recorded pointer (c_void_p or an address), as a writable view"""
    addr = p.value if isinstance(p, ctypes.c_void_p) else int(p)
    assert addr
    return np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(_CT[np.dtype(dt)])), shape=(count,))


def _check_fn(st, spec, count, dt):
    """one PogsAmdFn against its spec: array fields are pointers to `count` typed elements, scalars broadcast values"""
    assert isinstance(st, _lib.PogsAmdFn)
    for k in FIELDS:
        want, fdt = spec[k], (np.int32 if k == "h" else dt)
        if np.ndim(want) == 0:
            assert getattr(st, k) is None, k                       # NULL: the value is broadcast
            got = getattr(st, k + "0")
            assert got == (int(want) if k == "h" else float(want)), (k, got, want)
        else:
            got = _view(getattr(st, k), fdt, count)
            assert np.array_equal(got, np.asarray(want).astype(fdt)), (k, got, want)


def _check_fns(fa, ga, fsp, gsp, shapes, dt):
    for j, (m, n) in enumerate(shapes):
        _check_fn(fa[j], fsp[j], m, dt)
        _check_fn(ga[j], gsp[j], n, dt)


def _scalars(got, want):
    """equal values of equal types (an int stays an int, a float a float)"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert type(g) is type(w) and g == w, (got, want)


def _fill(ptrs, ms, ns, dt):
    """write recognisable outputs through the seven (or eight, with rho_final) output pointers, ABI order"""
    k, Mt, Nt = len(ms), sum(ms), sum(ns)
    want = {"x": 1.0 + 0.5 * np.arange(Nt), "y": 2.0 + np.arange(Mt), "l": -1.0 - np.arange(Mt),
            "mu": 0.25 * np.arange(Nt), "optval": 10.0 + np.arange(k), "iterations": 100 + np.arange(k),
            "status": np.array([0, 3, 0, 1] * k)[:k], "rho": 5.0 + np.arange(k)}
    types = [dt, dt, dt, dt, np.float64, np.uint32, np.int32, np.float64]
    for p, (name, v), t in zip(ptrs, want.items(), types):
        _view(p, t, len(v))[:] = v
    return want


def _pieces(flat, lens):
    ends = np.cumsum(lens)
    return [np.asarray(flat[e - n:e]) for e, n in zip(ends, lens)]


class Recorder:
    """Stands in for one library entry: counts the arguments, has `check(args, call number)` compare them while the
    call is in flight (the inputs behind the pointers live no longer than that) and report the problems' shapes, fills
    the outputs found at `outs` (the index of the x pointer) for those shapes, returns 0."""

    def __init__(self, nargs, outs, check, dt, nout=7):
        self.nargs, self.outs, self.check, self.dt, self.nout = nargs, outs, check, dt, nout
        self.calls, self.filled = [], []

    def __call__(self, *a):
        assert len(a) == self.nargs, (len(a), self.nargs)
        shapes = self.check(a, len(self.calls))
        self.calls.append(a)
        self.filled.append(_fill(a[self.outs:self.outs + self.nout], [s[0] for s in shapes], [s[1] for s in shapes],
                                 self.dt))
        return 0


_BARE = []


def _bare_solver(m, n, dt, sparse=False):
    s = object.__new__(graph.Solver)
    s._h = ctypes.c_void_p(1)
    s.m, s.n, s.dtype, s.sparse = m, n, np.dtype(dt), sparse
    _BARE.append(s)
    return s


def _bare_many(dt, shapes=None):
    s = object.__new__(graph.ManySolver)
    s._h = ctypes.c_void_p(1)
    _BARE.append(s)
    if shapes is None:
        s.k, s.m, s.n, s.dtype = K, M, N, np.dtype(dt)
    else:
        s.k, s.m, s.n, s.dtype = len(shapes), max(p[0] for p in shapes), max(p[1] for p in shapes), np.dtype(dt)
        s.shapes = list(shapes)
    return s


@pytest.fixture(autouse=True)
def _no_destroy():
    # the bare handles are non-NULL dummies: they are NULL again before anything can close them
    yield
    while _BARE:
        _BARE.pop()._h = ctypes.c_void_p()


def _uniform_dict(res, want, k, m, n, dt, with_rho):
    """the dict of arrays of solve_many / ManySolver.solve on a uniform handle"""
    assert list(res) == ["x", "y", "l", "mu", "optval", "iterations", "status"] + (["rho"] if with_rho else [])
    for key, cols in (("x", n), ("y", m), ("l", m), ("mu", n)):
        assert res[key].dtype == np.dtype(dt) and res[key].shape == (k, cols)
        assert np.array_equal(res[key], want[key].astype(dt).reshape(k, cols))
    assert res["optval"].dtype == np.float64 and np.array_equal(res["optval"], want["optval"])
    for key in ("iterations", "status"):
        assert res[key].dtype == np.int64 and np.array_equal(res[key], want[key])
    if with_rho:
        assert res["rho"].dtype == np.float64 and np.array_equal(res["rho"], want["rho"])


def _problem_dicts(res, want, shapes, dt, with_rho, copies):
    """the list of per-problem dicts of solve_batch / solve_many_ragged"""
    ms, ns = [s[0] for s in shapes], [s[1] for s in shapes]
    assert isinstance(res, list) and len(res) == len(shapes)
    parts = {key: _pieces(want[key].astype(dt), ns if key in ("x", "mu") else ms) for key in ("x", "y", "l", "mu")}
    for j, r in enumerate(res):
        assert list(r) == ["x", "y", "l", "mu", "optval", "iterations", "status"] + (["rho"] if with_rho else [])
        for key in ("x", "y", "l", "mu"):
            assert r[key].dtype == np.dtype(dt) and r[key].ndim == 1 and np.array_equal(r[key], parts[key][j])
            assert (r[key].base is None) == copies, key        # ragged pieces are copies, batch rows are views
        assert type(r["optval"]) is float and r["optval"] == want["optval"][j]
        assert type(r["iterations"]) is int and r["iterations"] == want["iterations"][j]
        assert type(r["status"]) is int and r["status"] == want["status"][j]
        if with_rho:
            assert type(r["rho"]) is float and r["rho"] == want["rho"][j]


# ---- 1, 2: Solver.solve and Solver.begin_run --------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES)
def test_solve_and_begin_run(monkeypatch, dt):
    calls = []
    s = _bare_solver(M, N, dt)
    fsp, gsp = _f_spec(M, 1), _objs_spec(N)
    f, g = _vector(fsp, M), _objs(gsp, N)
    x0, l0 = np.arange(N) + 0.5, np.arange(M) - 0.5

    def solve_fn(*a):
        assert len(a) == 16 and a[0] is s._h
        calls.append("solve")
        _check_fn(a[1]._obj, fsp, M, dt)
        _check_fn(a[2]._obj, gsp, N, dt)
        _scalars(a[3:10], (1.75,) + TAIL)
        assert isinstance(a[14]._obj, ctypes.c_double) and isinstance(a[15]._obj, ctypes.c_uint)
        for i, v in zip(range(10, 14), (1.5, 2.5, 3.5, 4.5)):
            _view(a[i], dt, N if i in (10, 13) else M)[:] = v
        a[14]._obj.value, a[15]._obj.value = 12.5, 9
        return 3

    def begin_fn(*a):
        assert len(a) == 9 and a[0] is s._h
        calls.append("begin")
        _check_fn(a[1]._obj, fsp, M, dt)
        _check_fn(a[2]._obj, gsp, N, dt)
        _scalars(a[3:], (0.6, 3e-5, 7e-6, 123, 0, 1))
        return 0

    def warm_fn(*a):
        assert len(a) == 3 and a[0] is s._h
        calls.append("warm")
        assert np.array_equal(_view(a[1], dt, N), x0.astype(dt)) and np.array_equal(_view(a[2], dt, M), l0.astype(dt))
        return 0

    monkeypatch.setattr(graph.lib, "PogsAmdSolveFn", solve_fn)
    monkeypatch.setattr(graph.lib, "PogsAmdBeginRunFn", begin_fn)
    monkeypatch.setattr(graph.lib, "PogsAmdSetWarmStart", warm_fn)
    res = s.solve(f, g, rho=1.75, x0=x0, l0=l0, **OPTS)
    s.begin_run(f, g, rho=0.6, **{k: v for k, v in OPTS.items() if k != "verbose"})
    assert calls == ["warm", "solve", "begin"]
    assert list(res) == ["x", "y", "l", "mu", "optval", "iterations", "status"]
    for key, v, n in (("x", 1.5, N), ("y", 2.5, M), ("l", 3.5, M), ("mu", 4.5, N)):
        assert res[key].dtype == np.dtype(dt) and res[key].shape == (n,) and np.all(res[key] == v)
    assert (res["optval"], res["iterations"], res["status"]) == (12.5, 9, 3)
    assert type(res["optval"]) is float and type(res["iterations"]) is int


def test_solve_asserts_the_lengths(monkeypatch):
    def boom(*a):
        raise RuntimeError("the library was called")

    monkeypatch.setattr(graph.lib, "PogsAmdSolveFn", boom)
    monkeypatch.setattr(graph.lib, "PogsAmdBeginRunFn", boom)
    s = _bare_solver(M, N, np.float64)
    f, g = _vector(_f_spec(M, 0), M), _vector(_g_spec(N, 0), N)
    for bad in ((_vector(_f_spec(M + 1, 0), M + 1), g), (f, _vector(_g_spec(N - 1, 0), N - 1))):
        with pytest.raises(AssertionError):
            s.solve(*bad)
        with pytest.raises(AssertionError):
            s.begin_run(*bad)


# ---- 3: Solver.solve_batch, plain -------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
def test_solve_batch_plain(monkeypatch, dt, sparse):
    def boom(*a):
        raise AssertionError("the wrong entry was called")

    s = _bare_solver(M, N, dt, sparse)
    shapes = [(M, N)] * K
    fs, gs, fsp, gsp = _pairs(shapes)

    def check(a, call):
        assert a[0] is s._h
        _scalars((a[1],), (K,))
        _check_fns(a[2], a[3], fsp, gsp, shapes, dt)
        assert np.array_equal(_view(a[4], np.float64, K), ([0.5, 1.5, 2.5], [0.75] * K)[call])
        _scalars(a[5:11], TAIL)
        return shapes

    rec = Recorder(18, 11, check, dt)
    monkeypatch.setattr(graph.lib, "PogsAmdSolveBatchSparseFn", rec if sparse else boom)
    monkeypatch.setattr(graph.lib, "PogsAmdSolveBatchFn", boom if sparse else rec)
    monkeypatch.setattr(graph.lib, "PogsAmdSolveBatchWarmFn", boom)
    res = s.solve_batch(fs, gs, rho=[0.5, 1.5, 2.5], **OPTS)
    _problem_dicts(res, rec.filled[0], shapes, dt, with_rho=False, copies=False)
    s.solve_batch(fs, gs, rho=0.75, **OPTS)                           # one value for all
    assert len(rec.calls) == 2


# ---- 4: Solver.solve_batch with starts / return_rho, two chunks -------------------------------------------------------

@pytest.mark.parametrize("mode", ["return_rho", "starts"])
@pytest.mark.parametrize("dt", DTYPES)
def test_solve_batch_warm_in_two_chunks(monkeypatch, dt, mode):
    def boom(*a):
        raise AssertionError("the wrong entry was called")

    s = _bare_solver(M, N, dt)
    k = _lib.BATCH_MAX + 3
    shapes = [(M, N)] * k
    fs, gs, fsp, gsp = _pairs(shapes)
    rho = [0.5 + j for j in range(k)]
    kw = {}
    if mode == "starts":
        # the first chunk mixes warm and cold members (a cold one may have no start); the second is all cold
        warm = [j % 2 == 0 for j in range(_lib.BATCH_MAX)] + [False] * 3
        x0 = [np.arange(N) + j if warm[j] else None for j in range(k)]
        l0 = [np.arange(M) - j if warm[j] else None for j in range(k)]
        kw = dict(x0=x0, l0=l0, warm=warm)

    def check(a, call):
        lo, kb = ((0, _lib.BATCH_MAX), (_lib.BATCH_MAX, 3))[call]
        assert a[0] is s._h
        _scalars((a[1],), (kb,))
        _check_fns(a[2], a[3], fsp[lo:lo + kb], gsp[lo:lo + kb], shapes[lo:lo + kb], dt)
        assert np.array_equal(_view(a[4], np.float64, kb), rho[lo:lo + kb])
        if mode == "starts" and call == 0:
            xs, ls = _view(a[5], dt, kb * N).reshape(kb, N), _view(a[6], dt, kb * M).reshape(kb, M)
            assert np.array_equal(_view(a[7], np.int32, kb), np.array(warm[:kb], np.int32))
            for j in range(kb):
                assert np.array_equal(xs[j], (x0[j] if warm[j] else np.zeros(N)).astype(dt))
                assert np.array_equal(ls[j], (l0[j] if warm[j] else np.zeros(M)).astype(dt))
        else:
            assert a[5] is None and a[6] is None and a[7] is None
        _scalars(a[8:14], TAIL)
        return shapes[lo:lo + kb]

    rec = Recorder(22, 14, check, dt, nout=8)
    monkeypatch.setattr(graph.lib, "PogsAmdSolveBatchSparseFn", boom)
    monkeypatch.setattr(graph.lib, "PogsAmdSolveBatchFn", boom)
    monkeypatch.setattr(graph.lib, "PogsAmdSolveBatchWarmFn", rec)
    res = s.solve_batch(fs, gs, rho=rho, return_rho=mode == "return_rho", **kw, **OPTS)
    assert len(rec.calls) == 2
    _problem_dicts(res[:_lib.BATCH_MAX], rec.filled[0], shapes[:_lib.BATCH_MAX], dt, with_rho=True, copies=False)
    _problem_dicts(res[_lib.BATCH_MAX:], rec.filled[1], shapes[_lib.BATCH_MAX:], dt, with_rho=True, copies=False)


# ---- 5: solve_many ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES)
def test_solve_many(monkeypatch, dt):
    shapes = [(M, N)] * K
    fs, gs, fsp, gsp = _pairs(shapes)
    A = np.arange(K * M * N, dtype=np.float64).reshape(K, M, N) / 7.0

    def check(a, call):
        _scalars(a[:5], (_lib.F64 if dt == np.float64 else _lib.F32, int(graph.Ordering.ROW_MAJ), K, M, N))
        assert np.array_equal(_view(a[5], dt, K * M * N), A.astype(dt).ravel())
        assert a[6] == _lib.HOST
        assert (a[7]._obj.device, a[7]._obj.projector) == ((2, -1)[call], _lib.PROJ_DIRECT)
        _check_fns(a[8], a[9], fsp, gsp, shapes, dt)
        assert np.array_equal(_view(a[10], np.float64, K), ([0.5, 1.5, 2.5], [2.0] * K)[call])
        _scalars(a[11:17], TAIL)
        return shapes

    rec = Recorder(24, 17, check, dt)
    monkeypatch.setattr(graph.lib, "PogsAmdSolveManyFn", rec)
    res = graph.solve_many(A, fs, gs, rho=[0.5, 1.5, 2.5], dtype=dt, device=2, **OPTS)
    _uniform_dict(res, rec.filled[0], K, M, N, dt, with_rho=False)
    graph.solve_many(A, fs, gs, rho=2.0, dtype=dt, **OPTS)                    # one value for all
    assert len(rec.calls) == 2


# ---- 6: solve_many_ragged ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES)
def test_solve_many_ragged(monkeypatch, dt):
    total = sum(m * n for m, n in RAGGED)
    fs, gs, fsp, gsp = _pairs(RAGGED)
    As = [np.arange(m * n, dtype=np.float64).reshape(m, n) / 3.0 + j for j, (m, n) in enumerate(RAGGED)]
    packed = np.concatenate([m.ravel(order="F") for m in As])             # the second call: column-major, with shapes

    def check(a, call):
        order = (graph.Ordering.ROW_MAJ, graph.Ordering.COL_MAJ)[call]
        _scalars(a[:3], (_lib.F64 if dt == np.float64 else _lib.F32, int(order), K))
        assert list(a[3]) == [s[0] for s in RAGGED] and list(a[4]) == [s[1] for s in RAGGED]
        assert ctypes.sizeof(a[3]) == K * ctypes.sizeof(ctypes.c_size_t) == ctypes.sizeof(a[4])
        want = (np.concatenate([m.ravel() for m in As]), packed)[call]
        assert np.array_equal(_view(a[5], dt, total), want.astype(dt))
        assert a[6] == _lib.HOST
        assert (a[7]._obj.device, a[7]._obj.projector) == ((1, -1)[call], _lib.PROJ_DIRECT)
        _check_fns(a[8], a[9], fsp, gsp, RAGGED, dt)
        assert np.array_equal(_view(a[10], np.float64, K), ([0.5, 1.5, 2.5], [3.0] * K)[call])
        _scalars(a[11:17], TAIL)
        return RAGGED

    rec = Recorder(24, 17, check, dt)
    monkeypatch.setattr(graph.lib, "PogsAmdSolveManyRaggedFn", rec)
    res = graph.solve_many_ragged(As, fs, gs, rho=[0.5, 1.5, 2.5], dtype=dt, device=1, **OPTS)
    _problem_dicts(res, rec.filled[0], RAGGED, dt, with_rho=False, copies=True)
    res = graph.solve_many_ragged(packed, fs, gs, rho=3.0, dtype=dt, shapes=RAGGED, order="F", **OPTS)
    _problem_dicts(res, rec.filled[1], RAGGED, dt, with_rho=False, copies=True)


# ---- 7, 8: ManySolver.solve on a uniform and on a ragged bare handle --------------------------------------------------

@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
def test_many_solver_solve(monkeypatch, dt, ragged):
    shapes = RAGGED if ragged else [(M, N)] * K
    ms, ns = [s[0] for s in shapes], [s[1] for s in shapes]
    s = _bare_many(dt, RAGGED if ragged else None)
    fs, gs, fsp, gsp = _pairs(shapes)
    x0 = [np.arange(n) + 0.5 + j for j, n in enumerate(ns)]
    l0 = [np.arange(m) - 0.25 * j for j, m in enumerate(ms)]
    given = dict(x0=x0, l0=l0) if ragged else dict(x0=np.stack(x0), l0=np.stack(l0))
    codes = (_lib.MANY_COLD, _lib.MANY_WARM_GIVEN, _lib.MANY_WARM_LAST)
    rhos = (None, [0.5, 1.5, 2.5], [0.25] * K)

    def check(a, call):
        assert a[0] is s._h
        _check_fns(a[1], a[2], fsp, gsp, shapes, dt)
        assert a[3] is None if rhos[call] is None else np.array_equal(_view(a[3], np.float64, K), rhos[call])
        _scalars((a[4],), (codes[call],))
        if codes[call] == _lib.MANY_WARM_GIVEN:
            assert np.array_equal(_view(a[5], dt, sum(ns)), np.concatenate(x0).astype(dt))
            assert np.array_equal(_view(a[6], dt, sum(ms)), np.concatenate(l0).astype(dt))
        else:
            assert a[5] is None and a[6] is None
        _scalars(a[7:13], TAIL)
        return shapes

    rec = Recorder(21, 13, check, dt, nout=8)
    monkeypatch.setattr(graph.lib, "PogsAmdManySolveFn", rec)
    out = [s.solve(fs, gs, **OPTS),                                           # cold, rho None
           s.solve(fs, gs, rho=[0.5, 1.5, 2.5], start="warm", **given, **OPTS),
           s.solve(fs, gs, rho=0.25, start="last", **OPTS)]
    assert len(rec.calls) == 3
    for res, want in zip(out, rec.filled):
        if not ragged:
            _uniform_dict(res, want, K, M, N, dt, with_rho=True)
            continue
        assert list(res) == ["x", "y", "l", "mu", "optval", "iterations", "status", "rho"]
        for key in ("x", "y", "l", "mu"):
            parts = _pieces(want[key].astype(dt), ns if key in ("x", "mu") else ms)
            assert isinstance(res[key], list) and len(res[key]) == K
            for got, piece in zip(res[key], parts):
                assert got.dtype == np.dtype(dt) and got.base is None and np.array_equal(got, piece)    # copies
        assert res["optval"].dtype == np.float64 and np.array_equal(res["optval"], want["optval"])
        assert res["rho"].dtype == np.float64 and np.array_equal(res["rho"], want["rho"])
        for key in ("iterations", "status"):
            assert res[key].dtype == np.int64 and np.array_equal(res[key], want[key])


# ---- refusals: the first failing check names the message --------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")

    for name in ("PogsAmdSolveBatchFn", "PogsAmdSolveBatchSparseFn", "PogsAmdSolveBatchWarmFn", "PogsAmdSolveManyFn",
                 "PogsAmdSolveManyRaggedFn", "PogsAmdManySolveFn"):
        monkeypatch.setattr(graph.lib, name, boom)


def _raises(text, call, *a, **kw):
    with pytest.raises(ValueError) as e:
        call(*a, **kw)
    assert str(e.value) == text, str(e.value)


def test_solve_batch_refusal_order(no_library):
    s = _bare_solver(M, N, np.float64)
    fs, gs, _, _ = _pairs([(M, N)] * K)
    long_f = _vector(_f_spec(M + 1, 0), M + 1)
    x0, l0 = [np.zeros(N)] * K, [np.zeros(M)] * K
    # counts, then rho, then every length (the last problem's too), then the starts
    _raises("solve_batch: 3 f and 2 g function vectors", s.solve_batch, fs, gs[:2], rho=[1.0], x0=x0)
    _raises("solve_batch: 3 problems and 2 rho values", s.solve_batch, [long_f] + fs[1:], gs, rho=[1.0, 2.0], x0=x0)
    _raises("solve_batch: f must have length 5 and g length 3, got 6 and 3", s.solve_batch, fs[:2] + [long_f], gs, x0=x0)
    _raises("solve_batch: a warm start needs both x0 and l0", s.solve_batch, fs, gs, x0=x0)
    _raises("solve_batch: 3 problems, 3 x0, 2 l0 and 3 warm flags", s.solve_batch, fs, gs, x0=x0, l0=l0[:2])
    # a wrong length in the second chunk is found before the first chunk is sent
    k = _lib.BATCH_MAX + 3
    fk, gk, _, _ = _pairs([(M, N)] * k)
    _raises("solve_batch: f must have length 5 and g length 3, got 6 and 3", s.solve_batch, fk[:-1] + [long_f], gk)


def test_solve_many_refusal_order(no_library):
    fs, gs, _, _ = _pairs([(M, N)] * K)
    A = np.ones((K, M, N))
    short_g = _vector(_g_spec(N - 1, 0), N - 1)
    # the counts, then rho, then the lengths
    _raises("solve_many: 3 matrices, 2 f and 3 g function vectors", graph.solve_many, A, fs[:2], [short_g] + gs[1:])
    _raises("solve_many: 3 matrices, 2 f and 3 g function vectors", graph.solve_many, A, fs[:2], gs, rho=[1.0, 2.0])
    _raises("solve_many: 3 matrices, 3 f and 4 g function vectors", graph.solve_many, A, fs, gs + gs[:1], rho=[1.0])
    _raises("solve_many: 3 problems and 2 rho values", graph.solve_many, A, fs, [short_g] + gs[1:], rho=[1.0, 2.0])
    _raises("solve_many: f must have length 5 and g length 3, got 5 and 2", graph.solve_many, A, fs, gs[:2] + [short_g])
    _raises("solve_many: A must be (k, m, n), got shape (5, 3)", graph.solve_many, A[0], fs[:2], gs, rho=[1.0])


def test_solve_many_ragged_refusal_order(no_library):
    fs, gs, _, _ = _pairs(RAGGED)
    As = [np.ones(s) for s in RAGGED]
    who = "solve_many_ragged"
    _raises(who + ": order must be 'C' or 'F', got 'K'", graph.solve_many_ragged, As, fs[:2], gs, rho=[1.0], order="K")
    _raises(who + ": 3 problems and 2 rho values", graph.solve_many_ragged, As, fs[:2], gs, rho=[1.0, 2.0])
    _raises(who + ": 3 matrices, 2 f and 3 g function vectors", graph.solve_many_ragged, As, fs[:2], [gs[1]] + gs[1:])
    _raises(who + ": problem 1: f must have length 1 and g length 4, got 3 and 4", graph.solve_many_ragged, As,
            [fs[0], fs[0], fs[2]], gs)
    _raises(who + ": problem 2: f must have length 5 and g length 5, got 5 and 2", graph.solve_many_ragged, As, fs,
            [gs[0], gs[1], gs[0]])


@pytest.mark.parametrize("ragged", [False, True])
def test_many_solver_refusal_order(no_library, ragged):
    shapes = RAGGED if ragged else [(M, N)] * K
    s = _bare_many(np.float64, RAGGED if ragged else None)
    fs, gs, _, _ = _pairs(shapes)
    x0, l0 = [np.zeros(n) for _, n in shapes], [np.zeros(m) for m, _ in shapes]
    if not ragged:
        x0, l0 = np.stack(x0), np.stack(l0)
    wrong_f = [fs[0], _vector(_f_spec(7, 0), 7), fs[2]]
    lengths = ("ManySolver: problem 1: f must have length 1 and g length 4, got 7 and 4" if ragged else
               "ManySolver: f must have length 5 and g length 3, got 7 and 3")
    both = ("ManySolver: start='warm' needs both x0 and l0 (lists of k per-problem arrays)" if ragged else
            "ManySolver: start='warm' needs both x0 (k x n) and l0 (k x m)")
    shape = ("ManySolver: l0 must be a list of 3 per-problem arrays, got 2" if ragged else
             "ManySolver: x0 must be 3 x 3 and l0 3 x 5, got (3, 3) and (2, 5)")
    # the start name first; then a uniform handle counts fs / gs, a ragged one after the starts and rho; the starts before
    # rho, rho before the lengths, the counts before the lengths
    count = "ManySolver: 3 matrices, 2 f and 3 g function vectors"
    stray = "ManySolver: x0 / l0 are read with start='warm' only"
    _raises("ManySolver: 3 problems and 2 rho values" if ragged else count, s.solve, fs[:2], gs, rho=[1.0, 2.0])
    _raises(both if ragged else count, s.solve, fs[:2], gs, start="warm", x0=x0)
    _raises(shape if ragged else count, s.solve, fs[:2], gs, start="warm", x0=x0, l0=l0[:2])
    _raises(stray if ragged else count, s.solve, fs[:2], gs, x0=x0)
    _raises(stray if ragged else count, s.solve, fs[:2], gs, start="last", l0=l0)
    _raises("ManySolver: start must be 'cold', 'warm' or 'last', got 'hot'", s.solve, fs[:2], gs, start="hot", x0=x0)
    _raises(both, s.solve, fs, gs, rho=[1.0], start="warm", x0=x0)
    _raises(shape, s.solve, fs, gs, rho=[1.0], start="warm", x0=x0, l0=l0[:2])
    _raises("ManySolver: x0 / l0 are read with start='warm' only", s.solve, wrong_f, gs, rho=[1.0], x0=x0)
    _raises("ManySolver: 3 problems and 2 rho values", s.solve, wrong_f, gs, rho=[1.0, 2.0])
    _raises("ManySolver: 3 matrices, 2 f and 3 g function vectors", s.solve, wrong_f[:2], gs)
    _raises(lengths, s.solve, wrong_f, gs)
    if ragged:
        _raises("ManySolver: x0[1] must have length 4, got shape (2,)", s.solve, wrong_f, gs, rho=[1.0], start="warm",
                x0=[x0[0], x0[0], x0[2]], l0=l0)
    # a closed handle is refused before anything else is read
    s._h = ctypes.c_void_p()
    _raises("ManySolver: the handle is closed", s.solve, fs[:2], gs, start="hot")
