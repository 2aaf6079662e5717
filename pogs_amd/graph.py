"""Graph-form POGS interface backed by the MI355X HIP engine.

Host-side mirror of the reference's ``python/pogs/graph.py``: the same seven
``solve_*`` entry points with the same signatures, defaults, function encodings
and return dictionary (``x, y, l, optval, iterations, status``), talking to
``libpogs_amd.so`` through the same C ABI the reference exposes
(``PogsD`` / ``PogsSparseD``; reference ``python/pogs/graph.py:167-233``), plus
what the reference's Python layer lacks for a GPU (SURVEY.md finding 6):

* ``dtype=`` to route to the fp32 entry points ``PogsS`` / ``PogsSparseS``
  (the reference wrapper forces float64, ``graph.py:281-288``);
* vectorised coefficient construction (``FunctionVector``) instead of m + n
  Python objects (``graph.py:428,431`` builds them one by one);
* ``Solver``: a persistent handle that keeps the equilibrated matrix and its
  factorisation on the GPU across solves, accepts device-resident matrices and
  row-shards over several GPUs (one process per GPU, RCCL).

Solves problems of the form

    minimize    sum_i f_i(y_i) + sum_j g_j(x_j)
    subject to  y = A x

with ``f_i(v) = c h(a v - b) + d v + e v^2 / 2`` and ``h`` one of `Function`.
"""
import atexit
import ctypes
import weakref
from enum import IntEnum

import numpy as np

from . import _lib
from ._lib import lib

try:
    import scipy.sparse as sp

    HAS_SCIPY = True
except ImportError:  # pragma: no cover
    HAS_SCIPY = False


class Ordering(IntEnum):
    """Matrix ordering (reference: python/pogs/graph.py:107-111)."""

    COL_MAJ = 0
    ROW_MAJ = 1


class Function(IntEnum):
    """Function types for f_i and g_j (reference: python/pogs/graph.py:114-132)."""

    kAbs = 0  # f(x) = |x|
    kExp = 1  # f(x) = e^x
    kHuber = 2  # f(x) = huber(x)
    kIdentity = 3  # f(x) = x
    kIndBox01 = 4  # f(x) = I(0 <= x <= 1)
    kIndEq0 = 5  # f(x) = I(x = 0)
    kIndGe0 = 6  # f(x) = I(x >= 0)
    kIndLe0 = 7  # f(x) = I(x <= 0)
    kLogistic = 8  # f(x) = log(1 + e^x)
    kMaxNeg0 = 9  # f(x) = max(0, -x)
    kMaxPos0 = 10  # f(x) = max(0, x)
    kNegEntr = 11  # f(x) = x log(x)
    kNegLog = 12  # f(x) = -log(x)
    kRecipr = 13  # f(x) = 1/x
    kSquare = 14  # f(x) = (1/2) x^2
    kZero = 15  # f(x) = 0


# Status codes (reference: src/include/pogs.h:31-37).  3, not 1, is "max_iter".
POGS_SUCCESS, POGS_INFEASIBLE, POGS_UNBOUNDED, POGS_MAX_ITER, POGS_NAN_FOUND, POGS_INVALID_CONE, POGS_ERROR = range(7)


class FunctionObj:
    """One function ``c * h(a * x - b) + d * x + e * x^2`` (reference: graph.py:135-164)."""

    def __init__(self, h=Function.kZero, a=1.0, b=0.0, c=1.0, d=0.0, e=0.0):
        self.h = h
        self.a = float(a)
        self.b = float(b)
        self.c = float(c)
        self.d = float(d)
        self.e = float(e)


class FunctionVector:
    """Struct-of-arrays of ``n`` function objects; every field broadcasts from a scalar.

    A field given as a scalar STAYS a scalar until somebody reads it as an array (``fv.c``, ``fv.c = ...``):
    `arrays()` -- what a solve hands to the C ABI -- then fills the typed array directly instead of converting
    a float64 copy.  A lasso on 2e6 rows has one per-element field out of twelve; building and marshalling
    its two vectors costs a few milliseconds this way instead of ~0.1 s (the reference builds m + n Python
    objects, python/pogs/graph.py:428,431)."""

    _FIELDS = ("h", "a", "b", "c", "d", "e")

    def __init__(self, n, h=Function.kZero, a=1.0, b=0.0, c=1.0, d=0.0, e=0.0):
        object.__setattr__(self, "n", int(n))
        object.__setattr__(self, "_v", {})
        object.__setattr__(self, "_typed", {})   # (field, dtype) -> the filled array of a SCALAR field (cannot go stale:
                                                 # a scalar has no elements to edit in place; dropped when the field is set)
        for k, v in zip(self._FIELDS, (h, a, b, c, d, e)):
            self._store(k, v)

    def _store(self, k, v):
        dt = np.int32 if k == "h" else np.float64
        for key in [key for key in self._typed if key[0] == k]:
            del self._typed[key]
        if np.ndim(v) == 0:
            self._v[k] = int(v) if k == "h" else float(v)          # scalar: materialised on demand
        else:
            self._v[k] = np.broadcast_to(np.asarray(v, dtype=dt), (self.n,)).copy()

    def _materialise(self, k):
        v = self._v[k]
        if not isinstance(v, np.ndarray):
            v = np.full(self.n, v, dtype=np.int32 if k == "h" else np.float64)
            self._v[k] = v                      # from here on an array the caller may edit: converted per call
            for key in [key for key in self._typed if key[0] == k]:
                del self._typed[key]
        return v

    def __getattr__(self, k):        # only reached for names that are not instance attributes: the six fields
        if k in FunctionVector._FIELDS:
            return self._materialise(k)
        raise AttributeError(k)

    def __setattr__(self, k, v):
        if k in self._FIELDS:
            self._store(k, v)
        else:
            object.__setattr__(self, k, v)

    def __len__(self):
        return self.n

    @staticmethod
    def from_objs(objs):
        fv = FunctionVector(len(objs))
        fv.h = np.array([int(o.h) for o in objs], dtype=np.int32)
        for k in "abcde":
            setattr(fv, k, np.array([getattr(o, k) for o in objs], dtype=np.float64))
        return fv

    def arrays(self, dtype):
        """The six contiguous arrays the C ABI takes (reference: graph.py:296-308)."""
        out = {}
        for k in self._FIELDS:
            v, dt = self._v[k], (np.int32 if k == "h" else dtype)
            if isinstance(v, np.ndarray):
                out[k] = np.ascontiguousarray(v, dtype=dt)
            else:
                key = (k, np.dtype(dt).str)
                if key not in self._typed:
                    # (zeros come as untouched zero pages: no fill, no page faults until somebody writes)
                    self._typed[key] = np.zeros(self.n, dtype=dt) if v == 0 else np.full(self.n, v, dtype=dt)
                out[k] = self._typed[key]       # read-only to the library (the ABI never writes its inputs)
        return out

    def slice(self, lo, hi):
        fv = FunctionVector(hi - lo)
        for k in self._FIELDS:
            v = self._v[k]
            fv._v[k] = v[lo:hi].copy() if isinstance(v, np.ndarray) else v
        return fv


def _as_vector(f):
    return f if isinstance(f, FunctionVector) else FunctionVector.from_objs(list(f))


def _resolve_dtype(dtype):
    dt = np.dtype(np.float64 if dtype is None else dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("dtype must be float32 or float64")
    return dt


STORE_SAME, STORE_F32 = _lib.STORE_SAME, _lib.STORE_F32


def _resolve_storage(storage, dtype):
    """Solver(storage=...) as STORE_SAME / STORE_F32: None, np.float64, np.float32 or one of the two constants."""
    if storage is None:
        return STORE_SAME
    if isinstance(storage, (int, np.integer)) and not isinstance(storage, bool):
        if int(storage) not in (STORE_SAME, STORE_F32):
            raise ValueError("storage must be None, np.float64, np.float32, STORE_SAME or STORE_F32")
        code = int(storage)
    else:
        try:
            sdt = np.dtype(storage)
        except TypeError:
            raise ValueError("storage must be None, np.float64, np.float32, STORE_SAME or STORE_F32") from None
        if sdt == np.dtype(np.float32):
            code = STORE_F32
        elif sdt == np.dtype(np.float64) and dtype == np.dtype(np.float64):
            code = STORE_SAME
        else:
            raise ValueError("storage must be None, np.float64, np.float32, STORE_SAME or STORE_F32")
    if code == STORE_F32 and dtype != np.dtype(np.float64):
        raise ValueError("storage=float32 needs dtype=float64 (a float32 solver already stores float32)")
    return code


def _resolve_values(values, dtype):
    """Solver(values=...): True for float32 non-zeros under a float64 sparse solver.  None, np.float64 or np.float32."""
    if values is None:
        return False
    try:
        vdt = np.dtype(values) if isinstance(values, (type, np.dtype, str)) else None
    except TypeError:
        vdt = None
    # (compared through `is None` first: numpy reads None as float64)
    if vdt is not None and vdt == np.dtype(np.float64) and dtype == np.dtype(np.float64):
        return False
    if vdt is None or vdt != np.dtype(np.float32):
        raise ValueError("values must be None, np.float64 (on a float64 solver) or np.float32")
    if dtype != np.dtype(np.float64):
        raise ValueError("values=float32 needs dtype=float64 (a float32 solver already stores float32)")
    return True


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _solve_graph_form(A, f, g, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0, rho=1.0,
                      adaptive_rho=True, gap_stop=True, dtype=None):
    """Solve one graph-form problem through the one-shot C ABI (reference: graph.py:236-390).

    ``f`` / ``g``: lists of `FunctionObj` (as in the reference) or a `FunctionVector`.
    Returns dict with 'x', 'y', 'l', 'optval', 'iterations', 'status'.
    """
    dt = _resolve_dtype(dtype)
    real = ctypes.c_double if dt == np.float64 else ctypes.c_float
    is_sparse = HAS_SCIPY and sp.issparse(A)
    if is_sparse:
        A_csr = sp.csr_matrix(A, dtype=dt)
        m, n = A_csr.shape
        nnz = A_csr.nnz
        data = np.ascontiguousarray(A_csr.data, dtype=dt)
        ptr = np.ascontiguousarray(A_csr.indptr, dtype=np.int32)
        ind = np.ascontiguousarray(A_csr.indices, dtype=np.int32)
    else:
        A = np.asarray(A, dtype=dt, order="C")
        m, n = A.shape

    assert len(f) == m, f"f should have length {m}, got {len(f)}"
    assert len(g) == n, f"g should have length {n}, got {len(g)}"
    fa = _as_vector(f).arrays(dt)
    ga = _as_vector(g).arrays(dt)

    x = np.zeros(n, dtype=dt)
    y = np.zeros(m, dtype=dt)
    dual = np.zeros(m, dtype=dt)
    optval = real()
    final_iter = ctypes.c_uint()
    tail = [_ptr(fa["a"]), _ptr(fa["b"]), _ptr(fa["c"]), _ptr(fa["d"]), _ptr(fa["e"]), _ptr(fa["h"]),
            _ptr(ga["a"]), _ptr(ga["b"]), _ptr(ga["c"]), _ptr(ga["d"]), _ptr(ga["e"]), _ptr(ga["h"]),
            real(rho), real(abs_tol), real(rel_tol), int(max_iter), int(verbose), int(adaptive_rho), int(gap_stop),
            _ptr(x), _ptr(y), _ptr(dual), ctypes.cast(ctypes.byref(optval), ctypes.c_void_p),
            ctypes.cast(ctypes.byref(final_iter), ctypes.c_void_p)]
    if is_sparse:
        fn = lib.PogsSparseD if dt == np.float64 else lib.PogsSparseS
        status = fn(int(Ordering.ROW_MAJ), m, n, nnz, _ptr(data), _ptr(ptr), _ptr(ind), *tail)
    else:
        fn = lib.PogsD if dt == np.float64 else lib.PogsS
        status = fn(int(Ordering.ROW_MAJ), m, n, _ptr(A), *tail)
    return {"x": x, "y": y, "l": dual, "optval": optval.value, "iterations": final_iter.value, "status": status}


# ---------------------------------------------------------------------------
# Function encodings of the seven solve_* problems (reference: graph.py:428-705)
# ---------------------------------------------------------------------------
def lasso_functions(b, lambd, n):
    """f_i = 0.5 (y_i - b_i)^2 ; g_j = lambda |x_j|   (graph.py:428,431)"""
    b = np.asarray(b, dtype=np.float64).ravel()
    return (FunctionVector(len(b), Function.kSquare, 1.0, b, 1.0),
            FunctionVector(n, Function.kAbs, 1.0, 0.0, lambd))


def ridge_functions(b, lambd, n):
    """g_j = 0.5 lambda x_j^2 as kSquare with c = lambda   (graph.py:471,474)"""
    b = np.asarray(b, dtype=np.float64).ravel()
    return (FunctionVector(len(b), Function.kSquare, 1.0, b, 1.0),
            FunctionVector(n, Function.kSquare, 1.0, 0.0, lambd))


def elastic_net_functions(b, lambda1, lambda2, n):
    """g_j = kAbs with c = lambda1, e = lambda2 / 2   (graph.py:518,522; quirk kept:
    the engine's quadratic term is e x^2 / 2, so this penalises lambda2/4 x^2)"""
    b = np.asarray(b, dtype=np.float64).ravel()
    return (FunctionVector(len(b), Function.kSquare, 1.0, b, 1.0),
            FunctionVector(n, Function.kAbs, 1.0, 0.0, lambda1, 0.0, lambda2 / 2))


def logistic_functions(b, lambd, n):
    """f_i = log(1 + exp(-b_i y_i)) as kLogistic with a = -b_i   (graph.py:562-568)"""
    b = np.asarray(b, dtype=np.float64).ravel()
    f = FunctionVector(len(b), Function.kLogistic, -b, 0.0, 1.0)
    g = FunctionVector(n, Function.kAbs, 1.0, 0.0, lambd) if lambd > 0 else FunctionVector(n, Function.kZero)
    return f, g


def huber_functions(b, delta, lambd, n):
    """f_i = delta^2 huber((y_i - b_i) / delta)   (graph.py:614-620)"""
    b = np.asarray(b, dtype=np.float64).ravel()
    f = FunctionVector(len(b), Function.kHuber, 1.0 / delta, b / delta, delta * delta)
    g = FunctionVector(n, Function.kAbs, 1.0, 0.0, lambd) if lambd > 0 else FunctionVector(n, Function.kZero)
    return f, g


def svm_functions(b, lambd, n):
    """f_i = max(0, 1 - b_i y_i) as kMaxPos0 with a = -b_i, b = -1   (graph.py:660,663)"""
    b = np.asarray(b, dtype=np.float64).ravel()
    return (FunctionVector(len(b), Function.kMaxPos0, -b, -1.0, 1.0),
            FunctionVector(n, Function.kSquare, 1.0, 0.0, lambd))


def nonneg_ls_functions(b, n):
    """g_j = I(x_j >= 0)   (graph.py:702,705)"""
    b = np.asarray(b, dtype=np.float64).ravel()
    return (FunctionVector(len(b), Function.kSquare, 1.0, b, 1.0), FunctionVector(n, Function.kIndGe0))


def _shape(A):
    if HAS_SCIPY and sp.issparse(A):
        return A.shape
    return np.asarray(A).shape


def solve_lasso(A, b, lambd, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0, rho=1.0, dtype=None):
    """minimize 0.5 ||A x - b||^2 + lambda ||x||_1   (reference: graph.py:393-433)"""
    m, n = _shape(A)
    f, g = lasso_functions(b, lambd, n)
    return _solve_graph_form(A, f, g, abs_tol, rel_tol, max_iter, verbose, rho, dtype=dtype)


def _chain_schedule(P, slots=None):
    """The rounds of `Solver.solve_chain` for P problems: with slots = min(BATCH_MAX, slots or BATCH_MAX) (so None
    and 0 both mean BATCH_MAX; a negative value is a ValueError) and L = ceil(P / slots), segment s is the indices [s L, min((s + 1) L, P)) and round r holds element r of every
    segment that has one.  Returns a list of rounds, each a list of (index, predecessor): the predecessor is
    index - 1, solved one round earlier in the same segment, or None for the first element of a segment."""
    slots = min(_lib.BATCH_MAX, int(slots) if slots else _lib.BATCH_MAX)
    if slots < 1:
        raise ValueError("solve_chain: slots must be >= 1")
    if P <= 0:
        return []
    L = -(-P // slots)
    return [[(s0 + r, s0 + r - 1 if r else None) for s0 in range(0, P, L) if s0 + r < min(s0 + L, P)]
            for r in range(L)]


def _solve_path(A, b, lambdas, make_fg, abs_tol, rel_tol, max_iter, verbose, rho, dtype, chain=False, slots=None):
    lambdas = [float(v) for v in np.atleast_1d(lambdas)]
    m, n = _shape(A)
    pairs = [make_fg(b, lam, n) for lam in lambdas]
    with Solver(A, dtype=dtype) as s:
        if chain:
            res = s.solve_chain([p[0] for p in pairs], [p[1] for p in pairs], rho=rho, slots=slots, abs_tol=abs_tol,
                                rel_tol=rel_tol, max_iter=max_iter, verbose=verbose)
        else:
            res = s.solve_batch([p[0] for p in pairs], [p[1] for p in pairs], rho=rho, abs_tol=abs_tol,
                                rel_tol=rel_tol, max_iter=max_iter, verbose=verbose)
    return {"x": np.stack([r["x"] for r in res]) if res else np.zeros((0, n), _resolve_dtype(dtype)),
            "optval": np.array([r["optval"] for r in res]),
            "iterations": np.array([r["iterations"] for r in res], dtype=np.int64),
            "status": np.array([r["status"] for r in res], dtype=np.int64)}


def solve_lasso_path(A, b, lambdas, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0, rho=1.0, dtype=None,
                     chain=False, slots=None):
    """The lasso for every lambda of `lambdas` on one matrix, as batched solves (Solver.solve_batch).
    ``chain``: solve them as warm-started batches instead (Solver.solve_chain over at most ``slots`` segments of
    the list as given: pass the lambdas sorted), each lambda but the first of its segment started from its neighbour.
    Returns {'x': K x n, 'optval', 'iterations', 'status': length K}."""
    return _solve_path(A, b, lambdas, lasso_functions, abs_tol, rel_tol, max_iter, verbose, rho, dtype, chain, slots)


def solve_logistic_path(A, b, lambdas, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0, rho=1.0, dtype=None,
                        chain=False, slots=None):
    """L1-regularised logistic regression for every lambda of `lambdas`, as batched solves (see solve_lasso_path)."""
    return _solve_path(A, b, lambdas, logistic_functions, abs_tol, rel_tol, max_iter, verbose, rho, dtype, chain, slots)


def _fn_struct(f, count, dtype, keep):
    """A function vector as a PogsAmdFn: per-element fields as typed host arrays (kept alive in `keep`), fields
    that are still scalars as broadcast values (include/pogs_amd.h: PogsAmdSolveFn)."""
    fv = _as_vector(f)
    if len(fv) != count:
        raise ValueError("function vector of length %d where %d is needed" % (len(fv), count))
    st = _lib.PogsAmdFn()
    for k in FunctionVector._FIELDS:
        v = fv._v[k]
        if isinstance(v, np.ndarray):
            arr = np.ascontiguousarray(v, dtype=np.int32 if k == "h" else dtype)
            keep.append(arr)
            setattr(st, k, arr.ctypes.data)
        else:
            setattr(st, k, None)
            setattr(st, k + "0", int(v) if k == "h" else float(v))
    return st


def _counted(who, k, fs, gs):
    """``fs`` and ``gs`` as lists, after the check that each holds one function vector per problem."""
    fs, gs = list(fs), list(gs)
    if len(fs) != k or len(gs) != k:
        raise ValueError("%s: %d matrices, %d f and %d g function vectors" % (who, k, len(fs), len(gs)))
    return fs, gs


def _fn_arrays(who, fs, gs, shapes, dtype, each=False):
    """The function pairs of the len(shapes) problems of a call as two PogsAmdFn arrays plus their keep-alive list,
    after the count check and every length check.  ``shapes``: the pairs (m_j, n_j); ``each``: they differ from
    problem to problem, and a length message names its problem."""
    k = len(shapes)
    fs, gs = _counted(who, k, fs, gs)
    keep = []
    fa = (_lib.PogsAmdFn * k)()
    ga = (_lib.PogsAmdFn * k)()
    for j, (m, n) in enumerate(shapes):
        if len(fs[j]) != m or len(gs[j]) != n:
            raise ValueError("%s: %sf must have length %d and g length %d, got %d and %d"
                             % (who, "problem %d: " % j if each else "", m, n, len(fs[j]), len(gs[j])))
        fa[j] = _fn_struct(fs[j], m, dtype, keep)
        ga[j] = _fn_struct(gs[j], n, dtype, keep)
    return fa, ga, keep


def _rho_vector(who, rho, k):
    """``rho``, one value or k values, as k float64 values."""
    rhos = np.full(k, float(rho)) if np.ndim(rho) == 0 else np.ascontiguousarray(rho, dtype=np.float64).ravel()
    if len(rhos) != k:
        raise ValueError("%s: %d problems and %d rho values" % (who, k, len(rhos)))
    return rhos


def _tail(abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop):
    """The scalars every solve entry takes after rho (and the starts), as the ABI takes them."""
    return abs_tol, rel_tol, int(max_iter), int(verbose), int(adaptive_rho), int(gap_stop)


def _code(dt):
    return _lib.F64 if dt == np.float64 else _lib.F32


def _direct_options(tdev, device):
    """The options of a many-problem call: the direct projector on ``device``, -1 meaning a device tensor's own."""
    return _lib.PogsAmdOptions(device=tdev if (device == -1 and tdev is not None) else device,
                               projector=_lib.PROJ_DIRECT)


def _ragged_split(flat, lens):
    """The per-problem pieces (copies) of a packed output."""
    ends = np.cumsum(lens)
    return [flat[e - n:e].copy() for e, n in zip(ends, lens)]


class _Outputs:
    """The output buffers of a k-problem call.  ``m``, ``n``: the one shape of a uniform call, whose x, mu are k x n
    and y, l k x m arrays, or the k m_j and n_j of a ragged call, whose outputs are packed problem after problem."""

    def __init__(self, dt, k, m, n, rho=False):
        self.ragged, self.k, self.m, self.n = np.ndim(m) > 0, k, m, n
        rows, cols = (int(sum(m)), int(sum(n))) if self.ragged else ((k, m), (k, n))
        self.x, self.mu = np.zeros(cols, dt), np.zeros(cols, dt)
        self.y, self.l = np.zeros(rows, dt), np.zeros(rows, dt)
        self.optval = np.zeros(k, np.float64)
        self.final_iter = np.zeros(k, np.uint32)
        self.status = np.zeros(k, np.int32)
        self.rho = np.zeros(k, np.float64) if rho else None      # the final rho, of an entry that returns it

    def pointers(self):
        """The seven output pointers in ABI order, then rho_final where the entry has one."""
        out = [self.x, self.y, self.l, self.mu, self.optval, self.final_iter, self.status]
        return [_ptr(a) for a in (out if self.rho is None else out + [self.rho])]

    def _vectors(self):
        """x, y, l, mu, each indexed by problem: the k x n / k x m arrays, or lists of copies of the ragged pieces."""
        if not self.ragged:
            return self.x, self.y, self.l, self.mu
        return (_ragged_split(self.x, self.n), _ragged_split(self.y, self.m), _ragged_split(self.l, self.m),
                _ragged_split(self.mu, self.n))

    def arrays(self):
        """One dictionary for the call: arrays with a row per problem (ragged: lists with a piece per problem)."""
        x, y, l, mu = self._vectors()
        res = {"x": x, "y": y, "l": l, "mu": mu, "optval": self.optval, "iterations": self.final_iter.astype(np.int64),
               "status": self.status.astype(np.int64)}
        if self.rho is not None:
            res["rho"] = self.rho
        return res

    def problems(self):
        """One dictionary per problem, with the keys `Solver.solve` returns (and "rho")."""
        x, y, l, mu = self._vectors()
        res = [{"x": x[j], "y": y[j], "l": l[j], "mu": mu[j], "optval": float(self.optval[j]),
                "iterations": int(self.final_iter[j]), "status": int(self.status[j])} for j in range(self.k)]
        if self.rho is not None:
            for j, r in enumerate(res):
                r["rho"] = float(self.rho[j])
        return res


def _is_tensor(a):
    return hasattr(a, "data_ptr") and hasattr(a, "is_cuda")


def _tensor_dtype(who, A, dtype):
    """The solve's dtype for a torch tensor, which is read in place: the tensor's own; ``dtype`` may only repeat it."""
    import torch

    tdt = {torch.float32: np.float32, torch.float64: np.float64}.get(A.dtype)
    if tdt is None:
        raise ValueError("%s: A must be float32 or float64" % who)
    dt = _resolve_dtype(tdt if dtype is None else dtype)
    if dt != np.dtype(tdt):
        raise ValueError("%s: a device tensor is read in place: its dtype must be the solve's dtype" % who)
    return dt


def _many_matrices(A, dtype):
    """(k, m, n, pointer, mem, ord, dtype, device, keep-alive) of the k matrices of `solve_many`."""
    if _is_tensor(A):
        if A.dim() != 3:
            raise ValueError("solve_many: A must be a (k, m, n) tensor, got %d dimensions" % A.dim())
        dt = _tensor_dtype("solve_many", A, dtype)
        k, m, n = A.shape
        if not A.is_cuda:
            return _many_matrices(A.numpy(), dt)
        if A.is_contiguous():
            order = Ordering.ROW_MAJ
        elif A.stride() == (m * n, 1, m):
            order = Ordering.COL_MAJ
        else:
            raise ValueError("solve_many: each matrix of a device tensor must be row- or column-major and packed")
        _lib.check_device_pointer_interop()
        return k, m, n, ctypes.c_void_p(A.data_ptr()), _lib.DEVICE, order, dt, A.device.index, A
    if isinstance(A, (list, tuple)):
        mats = [np.asarray(a) for a in A]
        if not mats or any(a.ndim != 2 for a in mats) or any(a.shape != mats[0].shape for a in mats):
            raise ValueError("solve_many: A as a list must hold k >= 1 two-dimensional arrays of one shape")
        dt = _resolve_dtype(dtype)
        arr = np.ascontiguousarray(np.stack([np.asarray(a, dtype=dt) for a in mats]))
    else:
        dt = _resolve_dtype(dtype)
        arr = np.asarray(A)
        if arr.ndim != 3:
            raise ValueError("solve_many: A must be (k, m, n), got shape %s" % (arr.shape,))
        arr = np.asarray(arr, dtype=dt)
    k, m, n = arr.shape
    isz = arr.itemsize
    if arr.flags.c_contiguous:
        order = Ordering.ROW_MAJ
    elif arr.strides == (m * n * isz, isz, m * isz):      # every matrix Fortran-ordered, packed back to back
        order = Ordering.COL_MAJ
    else:
        arr = np.ascontiguousarray(arr)
        order = Ordering.ROW_MAJ
    return k, m, n, _ptr(arr), _lib.HOST, order, dt, None, arr


def solve_many(A, fs, gs, rho=1.0, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0, adaptive_rho=True,
               gap_stop=True, dtype=None, device=-1):
    """Solve k independent graph-form problems, problem j with its own matrix A_j and functions (fs[j], gs[j]), in
    one call on the GPU (include/pogs_amd.h: PogsAmdSolveManyFn).  Each is solved as the one-shot solve would solve
    it; a problem's results do not depend on the other problems.

    ``A``: a (k, m, n) ndarray (each matrix C- or Fortran-ordered), a list of k equal-shape 2-D arrays, or a
    (k, m, n) torch tensor on a ROCm device (read in place, never written).  ``fs``, ``gs``: k function vectors /
    lists of `FunctionObj`.  ``rho``: one value or k values.  ``device``: -1 = the tensor's device, else the
    current one.  Returns {'x': k x n, 'y': k x m, 'l': k x m, 'mu': k x n, 'optval', 'iterations', 'status':
    length k}.  verbose > 0 prints one summary for the call."""
    k, m, n, aptr, mem, order, dt, tdev, keep_a = _many_matrices(A, dtype)
    fs, gs = _counted("solve_many", k, fs, gs)          # (before rho; a ragged call checks rho first)
    rhos = _rho_vector("solve_many", rho, k)
    fa, ga, keep = _fn_arrays("solve_many", fs, gs, [(m, n)] * k, dt)
    opt = _direct_options(tdev, device)
    out = _Outputs(dt, k, m, n)
    st = lib.PogsAmdSolveManyFn(_code(dt), int(order), k, m, n, aptr, mem, ctypes.byref(opt), fa, ga, _ptr(rhos),
                                *_tail(abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop), *out.pointers())
    del keep, keep_a
    if st != 0:
        raise RuntimeError("pogs_amd: many-problem solve failed: " + _lib.last_error())
    return out.arrays()


def _ragged_matrices(As, dtype, shapes, order, who):
    """(k, ms, ns, pointer, mem, ord, dtype, device, keep-alive) of the matrices of a ragged call: ``As`` a sequence
    of 2-D arrays / tensors, or (with ``shapes``) one packed 1-D array / tensor holding them back to back."""
    if order not in ("C", "F"):
        raise ValueError("%s: order must be 'C' or 'F', got %r" % (who, order))

    if shapes is not None:                                        # one packed buffer
        shp = [tuple(int(v) for v in s) for s in shapes]
        if not shp or any(len(s) != 2 or s[0] < 1 or s[1] < 1 for s in shp):
            raise ValueError("%s: shapes must be k >= 1 pairs (m_j, n_j) of positive sizes" % who)
        total = sum(m * n for m, n in shp)
        ordc = Ordering.ROW_MAJ if order == "C" else Ordering.COL_MAJ
        if _is_tensor(As):
            dt = _tensor_dtype(who, As, dtype)
            if As.dim() != 1 or As.numel() != total or not As.is_contiguous():
                raise ValueError("%s: a packed A must be one contiguous 1-D tensor of sum m_j n_j = %d elements"
                                 % (who, total))
            if not As.is_cuda:
                return _ragged_matrices(As.numpy(), dt, shp, order, who)
            _lib.check_device_pointer_interop()
            return (len(shp), [s[0] for s in shp], [s[1] for s in shp], ctypes.c_void_p(As.data_ptr()), _lib.DEVICE,
                    ordc, dt, As.device.index, As)
        dt = _resolve_dtype(dtype)
        arr = np.asarray(As)
        if arr.ndim != 1 or arr.size != total:
            raise ValueError("%s: a packed A must be one 1-D array of sum m_j n_j = %d elements" % (who, total))
        arr = np.ascontiguousarray(arr, dtype=dt)
        return len(shp), [s[0] for s in shp], [s[1] for s in shp], _ptr(arr), _lib.HOST, ordc, dt, None, arr

    if _is_tensor(As) or isinstance(As, np.ndarray) or not hasattr(As, "__len__"):
        raise ValueError("%s: As must be a sequence of 2-D arrays (or one packed array with shapes=...)" % who)
    mats = list(As)
    if not mats:
        raise ValueError("%s: As must hold k >= 1 matrices" % who)
    if all(_is_tensor(a) for a in mats) and all(a.is_cuda for a in mats):
        import torch

        if any(a.dim() != 2 for a in mats):
            raise ValueError("%s: every member of As must be two-dimensional" % who)
        if any(a.dtype != mats[0].dtype or a.device != mats[0].device for a in mats):
            raise ValueError("%s: device tensors must share one dtype and one device" % who)
        shp = [tuple(a.shape) for a in mats]
        if any(m < 1 or n < 1 for m, n in shp):
            raise ValueError("%s: every member of As must have at least one row and one column" % who)
        packed = torch.cat([a.contiguous().reshape(-1) for a in mats])   # packed on the device, row-major
        return _ragged_matrices(packed, dtype, shp, "C", who)
    mats = [a.detach().cpu().numpy() if _is_tensor(a) else np.asarray(a) for a in mats]
    if any(a.ndim != 2 for a in mats):
        raise ValueError("%s: every member of As must be two-dimensional, got %s"
                         % (who, [a.ndim for a in mats if a.ndim != 2]))
    if any(a.shape[0] < 1 or a.shape[1] < 1 for a in mats):
        raise ValueError("%s: every member of As must have at least one row and one column" % who)
    dt = _resolve_dtype(dtype)
    # column-major when every member is Fortran-ordered; a member that is both (one row, one column) fits either
    # order and does not decide
    fortran = all(a.flags.f_contiguous for a in mats) and not all(a.flags.c_contiguous for a in mats)
    flat = np.concatenate([np.asarray(a, dtype=dt).ravel(order="F" if fortran else "C") for a in mats])
    return (len(mats), [a.shape[0] for a in mats], [a.shape[1] for a in mats], _ptr(flat), _lib.HOST,
            Ordering.COL_MAJ if fortran else Ordering.ROW_MAJ, dt, None, flat)


def solve_many_ragged(As, fs, gs, rho=1.0, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0, adaptive_rho=True,
                      gap_stop=True, dtype=None, device=-1, shapes=None, order="C"):
    """`solve_many` for problems of unequal shapes: problem j has its own m_j x n_j matrix ``As[j]`` and functions
    (fs[j]: length m_j, gs[j]: length n_j), all solved in one call (include/pogs_amd.h: PogsAmdSolveManyRaggedFn).
    Problem j's results are the bytes `solve_many` returns for it alone.

    ``As``: a sequence of 2-D arrays: host arrays (packed on the host; a list whose members are all Fortran-ordered
    is passed column-major, one-row and one-column members fit either order), or torch tensors on one ROCm device
    (packed on the device).  CPU tensors, and a list that mixes them with device tensors, are taken as host arrays.  With ``shapes`` (k pairs (m_j, n_j)),
    ``As`` is instead ONE packed 1-D array or device tensor holding the matrices back to back, each in ``order``
    ('C' or 'F'); a device tensor is read in place and never written.  ``rho``: one value or k values.
    Returns a list of k dictionaries {'x': n_j, 'y': m_j, 'l': m_j, 'mu': n_j, 'optval', 'iterations', 'status'}."""
    who = "solve_many_ragged"
    k, ms, ns, aptr, mem, ordc, dt, tdev, keep_a = _ragged_matrices(As, dtype, shapes, order, who)
    rhos = _rho_vector(who, rho, k)
    fa, ga, keep = _fn_arrays(who, fs, gs, list(zip(ms, ns)), dt, each=True)
    opt = _direct_options(tdev, device)
    out = _Outputs(dt, k, ms, ns)
    marr = (ctypes.c_size_t * k)(*ms)
    narr = (ctypes.c_size_t * k)(*ns)
    st = lib.PogsAmdSolveManyRaggedFn(_code(dt), int(ordc), k, marr, narr, aptr, mem, ctypes.byref(opt), fa, ga,
                                      _ptr(rhos), *_tail(abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop),
                                      *out.pointers())
    del keep, keep_a
    if st != 0:
        raise RuntimeError("pogs_amd: ragged many-problem solve failed: " + _lib.last_error())
    return out.problems()


def solve_ridge(A, b, lambd, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0, rho=1.0, dtype=None):
    """minimize 0.5 ||A x - b||^2 + 0.5 lambda ||x||^2   (reference: graph.py:436-476)"""
    m, n = _shape(A)
    f, g = ridge_functions(b, lambd, n)
    return _solve_graph_form(A, f, g, abs_tol, rel_tol, max_iter, verbose, rho, dtype=dtype)


def solve_elastic_net(A, b, lambda1, lambda2, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0, rho=1.0,
                      dtype=None):
    """minimize 0.5 ||A x - b||^2 + lambda1 ||x||_1 + 0.5 lambda2 ||x||^2   (reference: graph.py:479-524)"""
    m, n = _shape(A)
    f, g = elastic_net_functions(b, lambda1, lambda2, n)
    return _solve_graph_form(A, f, g, abs_tol, rel_tol, max_iter, verbose, rho, dtype=dtype)


def solve_logistic(A, b, lambd=0.0, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0, rho=1.0, dtype=None):
    """minimize sum_i log(1 + exp(-b_i a_i' x)) + lambda ||x||_1   (reference: graph.py:527-570)"""
    m, n = _shape(A)
    f, g = logistic_functions(b, lambd, n)
    return _solve_graph_form(A, f, g, abs_tol, rel_tol, max_iter, verbose, rho, dtype=dtype)


def solve_huber(A, b, delta=1.0, lambd=0.0, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0, rho=1.0,
                dtype=None):
    """minimize sum_i huber(A x - b, delta) + lambda ||x||_1   (reference: graph.py:573-622)"""
    m, n = _shape(A)
    f, g = huber_functions(b, delta, lambd, n)
    return _solve_graph_form(A, f, g, abs_tol, rel_tol, max_iter, verbose, rho, dtype=dtype)


def solve_svm(A, b, lambd=1.0, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0, rho=1.0, dtype=None):
    """minimize sum_i max(0, 1 - b_i a_i' x) + 0.5 lambda ||x||^2   (reference: graph.py:625-665)"""
    m, n = _shape(A)
    f, g = svm_functions(b, lambd, n)
    return _solve_graph_form(A, f, g, abs_tol, rel_tol, max_iter, verbose, rho, dtype=dtype)


def solve_nonneg_ls(A, b, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0, rho=1.0, dtype=None):
    """minimize 0.5 ||A x - b||^2 subject to x >= 0   (reference: graph.py:668-707)"""
    m, n = _shape(A)
    f, g = nonneg_ls_functions(b, n)
    return _solve_graph_form(A, f, g, abs_tol, rel_tol, max_iter, verbose, rho, dtype=dtype)


# ---------------------------------------------------------------------------
# Persistent handle (no counterpart in the reference's Python layer; its C++ API
# reuses the factorisation through _done_init, src/cpu/pogs.cpp:113-114)
# ---------------------------------------------------------------------------
# Handles still alive when the interpreter shuts down are destroyed by an atexit callback -- while the
# HIP runtime is certainly still there -- instead of by whatever order garbage collection and the C
# runtime's own exit handlers happen to take (a handle's destructor synchronises its stream).
_LIVE_SOLVERS = weakref.WeakSet()


def _close_live_solvers():
    for s in list(_LIVE_SOLVERS):
        try:
            s.close()
        except Exception:
            pass


atexit.register(_close_live_solvers)


class Solver:
    """Keeps the equilibrated matrix and its factorisation on the GPU across solves.

    ``A``: numpy array / scipy sparse matrix (host), an integer device pointer (dense), or a tuple
    (data_ptr, indptr_ptr, indices_ptr, nnz) of device addresses of a CSR matrix (sparse)
    with ``shape=(m, n)`` and ``device_ptr=True`` (e.g. ``tensor.data_ptr()``).
    ``dist``: None, or ``(rank, world, m_global, unique_id_bytes)`` for a
    row-sharded solve where this process holds ``m`` consecutive rows.
    ``projector``: PROJ_DEFAULT (dense: direct, sparse: CGLS), PROJ_CGLS, or PROJ_DIRECT -- on a sparse matrix with
    min(m, n) <= SPARSE_DIRECT_MAX on one GPU the exact projector: two products and two triangular mat-vecs per
    iteration instead of a CGLS loop (the one-shot ``solve_*`` calls keep CGLS).  PROJ_CGLS_FUSED (dense, one GPU):
    CGLS with one pass over A per CG step and one host poll per iteration (include/pogs_amd.h: PogsAmdCreateDense).
    ``storage``: None / np.float64 on a float64 solver / STORE_SAME: the matrix is stored in ``dtype``.  np.float32 or
    STORE_F32 with ``dtype=np.float64`` (dense, m > n, direct projector, one GPU, n <= 10240): mixed storage -- the
    equilibrated matrix is rounded to float32 and the handle solves, in float64 arithmetic, the problem of that rounded
    matrix; ``solve`` and ``iterate`` read the float32 copy (1.5 x the matrix memory; PogsAmdCreateDense).  The same
    with ``projector=PROJ_CGLS_FUSED`` (dense, ANY shape -- tall or wide --, one GPU, n <= 10240; a host array or a
    device pointer with ``shape=``): the projector's recurring launches -- A^T r at the start of a projection, the one
    pass of every CG step, the y-sync product -- read the float32 copy (PogsAmdCreateDenseMixed).  With any other
    projector ``storage`` keeps needing m > n.  The attribute ``storage`` holds STORE_SAME or STORE_F32.
    ``values``: None / np.float64: as ``dtype``.  np.float32 with ``dtype=np.float64`` on a SPARSE matrix (scipy, or the
    device-CSR tuple; one GPU, projector DEFAULT / CGLS / DIRECT): mixed storage -- the equilibrated non-zeros are
    rounded to float32 and the handle solves, in float64 arithmetic, the problem of that rounded matrix; every solo
    product streams float32 values, bit for bit the float64 product over the rounded values, and the handle holds 4
    bytes less per stored element on each tiled copy (PogsAmdCreateSparseMixed).  ``storage`` then reads STORE_F32.
    ``storage=`` itself stays a dense option (a sparse matrix refuses it); the two keywords do not combine.
    """

    def __init__(self, A, dtype=None, shape=None, device_ptr=False, order=Ordering.ROW_MAJ, device=-1,
                 profile=False, projector=_lib.PROJ_DEFAULT, dist=None, storage=None, values=None):
        self.dtype = _resolve_dtype(dtype)
        self.storage = _resolve_storage(storage, self.dtype)   # (ValueError before the library is called)
        mixed_values = _resolve_values(values, self.dtype)   # (the same)
        if mixed_values:
            if storage is not None:
                raise ValueError("values=float32 (sparse) and storage= (dense) do not combine: give one of them")
            if dist is not None:
                raise ValueError("values=float32 is single-GPU (row shards are not supported)")
            if not ((device_ptr and isinstance(A, (tuple, list))) or ((not device_ptr) and HAS_SCIPY and sp.issparse(A))):
                raise ValueError("values=float32 is the sparse option; a dense matrix takes storage=np.float32")
            self.storage = STORE_F32
        self._h = ctypes.c_void_p()
        code = _code(self.dtype)
        opt = _lib.PogsAmdOptions(device=device, projector=projector, profile=int(profile), storage=self.storage)
        dist_s = None
        self._m_global = None   # row shards: the rows of the whole matrix
        if dist is not None:
            rank, world, m_global, uid = dist
            self._m_global = int(m_global)
            dist_s = _lib.PogsAmdDist(rank=rank, world=world, m_global=m_global)
            uid = bytes(uid)
            assert len(uid) == _lib.UNIQUE_ID_BYTES
            # (a c_char array field reads back as an immutable bytes copy: write through the address)
            ctypes.memmove(ctypes.addressof(dist_s) + _lib.PogsAmdDist.unique_id.offset, uid, _lib.UNIQUE_ID_BYTES)
        dist_p = ctypes.byref(dist_s) if dist_s is not None else None
        if device_ptr:
            _lib.check_device_pointer_interop()
        self.sparse = (not device_ptr) and HAS_SCIPY and sp.issparse(A)
        if device_ptr and isinstance(A, (tuple, list)):
            # CSR already resident in HBM: (data_ptr, indptr_ptr, indices_ptr, nnz) device addresses
            # (data of the solver's dtype, int32 indices), with shape=(m, n)
            self.sparse = True
            self.m, self.n = shape
            dptr, pptr, iptr, nnz = (int(v) for v in A)
            csr, mem = (ctypes.c_void_p(dptr), ctypes.c_void_p(pptr), ctypes.c_void_p(iptr)), _lib.DEVICE
        elif self.sparse:
            A_csr = sp.csr_matrix(A, dtype=self.dtype)
            self.m, self.n = A_csr.shape
            data = np.ascontiguousarray(A_csr.data, dtype=self.dtype)
            ptr = np.ascontiguousarray(A_csr.indptr, dtype=np.int32)
            ind = np.ascontiguousarray(A_csr.indices, dtype=np.int32)
            csr, nnz, mem = (_ptr(data), _ptr(ptr), _ptr(ind)), A_csr.nnz, _lib.HOST
        if self.sparse:
            matrix = (int(Ordering.ROW_MAJ), self.m, self.n, nnz, *csr, mem, ctypes.byref(opt))
            if mixed_values:
                st = lib.PogsAmdCreateSparseMixed(ctypes.byref(self._h), *matrix)
            else:
                st = lib.PogsAmdCreateSparse(ctypes.byref(self._h), code, *matrix, dist_p)
        else:
            if device_ptr:
                self.m, self.n = shape
                ptr_val, mem = ctypes.c_void_p(int(A)), _lib.DEVICE
            else:
                A = np.asarray(A, dtype=self.dtype, order="C" if order == Ordering.ROW_MAJ else "F")
                self.m, self.n = A.shape
                ptr_val, mem = _ptr(A), _lib.HOST
            if self.storage == STORE_F32 and projector == _lib.PROJ_CGLS_FUSED and self.dtype == np.float64 and dist is None:
                # mixed storage with the one-pass CGLS projector (any shape) has an entry of its own; every other
                # combination goes to PogsAmdCreateDense, which honours or refuses it as before
                st = lib.PogsAmdCreateDenseMixed(ctypes.byref(self._h), int(order), self.m, self.n, ptr_val, mem, ctypes.byref(opt))
            else:
                st = lib.PogsAmdCreateDense(ctypes.byref(self._h), code, int(order), self.m, self.n, ptr_val, mem,
                                            ctypes.byref(opt), dist_p)
        if st != 0:
            raise RuntimeError("pogs_amd: solver creation failed: " + _lib.last_error())
        _LIVE_SOLVERS.add(self)

    def _coef(self, f, g):
        """(f, g) as two PogsAmdFn structures: per-element fields as typed host arrays, fields that are still scalars
        as broadcast values (filled on the device; include/pogs_amd.h: PogsAmdSolveFn).  Returns (structs, keep-alive)."""
        assert len(f) == self.m and len(g) == self.n
        keep = []
        return [_fn_struct(f, self.m, self.dtype, keep), _fn_struct(g, self.n, self.dtype, keep)], keep

    def warm_start(self, x0, l0):
        """Start the next solve from (x0, lambda0) instead of zero (reference: SetInitX /
        SetInitLambda, src/include/pogs.h:112-119; both are required, pogs.cpp:159-179)."""
        x0 = np.ascontiguousarray(x0, self.dtype)
        l0 = np.ascontiguousarray(l0, self.dtype)
        assert x0.shape == (self.n,) and l0.shape == (self.m,)
        if lib.PogsAmdSetWarmStart(self._h, _ptr(x0), _ptr(l0)) != 0:
            raise RuntimeError("pogs_amd: " + _lib.last_error())

    def solve(self, f, g, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0, rho=1.0, adaptive_rho=True,
              gap_stop=True, x0=None, l0=None):
        if x0 is not None or l0 is not None:
            self.warm_start(x0, l0)
        args, keep = self._coef(f, g)
        x = np.zeros(self.n, self.dtype)
        y = np.zeros(self.m, self.dtype)
        l = np.zeros(self.m, self.dtype)
        mu = np.zeros(self.n, self.dtype)
        optval = ctypes.c_double()
        final_iter = ctypes.c_uint()
        status = lib.PogsAmdSolveFn(self._h, ctypes.byref(args[0]), ctypes.byref(args[1]), rho,
                                    *_tail(abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop),
                                    _ptr(x), _ptr(y), _ptr(l), _ptr(mu), ctypes.byref(optval), ctypes.byref(final_iter))
        del keep
        if status == POGS_ERROR:
            raise RuntimeError("pogs_amd: solve failed: " + _lib.last_error())
        return {"x": x, "y": y, "l": l, "mu": mu, "optval": optval.value, "iterations": final_iter.value,
                "status": status}

    def solve_batch(self, fs, gs, rho=1.0, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0, adaptive_rho=True,
                    gap_stop=True, x0=None, l0=None, warm=None, return_rho=False):
        """Solve len(fs) problems (f_j, g_j, rho_j) on this handle's matrix, every pass over A shared by up to
        BATCH_MAX of them (include/pogs_amd.h: PogsAmdSolveBatchFn on a dense handle -- m > n, direct projector,
        one GPU; PogsAmdSolveBatchSparseFn on a sparse one -- any shape, one GPU).
        ``rho``: one value for all or a sequence.  Longer lists run as consecutive batches.  Returns a list of
        dicts with the keys `solve` returns.  The handle's solo state (a pending warm start included) is kept.
        ``x0`` / ``l0``: sequences of len(fs) starts (length n / m), both or neither; problem j starts from
        (x0[j], l0[j]) at rho_j as a solo solve does after `warm_start` (PogsAmdSolveBatchWarmFn).  ``warm``: len(fs)
        flags, the problems that do so (default: all of them); an entry of x0 / l0 may be None where its flag is
        false.  With a start or ``return_rho`` each dict also carries "rho", the problem's rho when it stopped."""
        fs, gs = list(fs), list(gs)
        k = len(fs)
        if len(gs) != k:
            raise ValueError("solve_batch: %d f and %d g function vectors" % (k, len(gs)))
        rhos = _rho_vector("solve_batch", rho, k)
        fa, ga, keep = _fn_arrays("solve_batch", fs, gs, [(self.m, self.n)] * k, self.dtype)   # every length, first
        starts = self._batch_starts(k, x0, l0, warm)
        plain = starts is None and not return_rho
        entry = lib.PogsAmdSolveBatchSparseFn if self.sparse else lib.PogsAmdSolveBatchFn
        tail = _tail(abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop)
        res = []
        for lo in range(0, k, _lib.BATCH_MAX):
            hi = min(k, lo + _lib.BATCH_MAX)
            kb = hi - lo
            # this chunk's structures, in place
            fb = (_lib.PogsAmdFn * kb).from_buffer(fa, lo * ctypes.sizeof(_lib.PogsAmdFn))
            gb = (_lib.PogsAmdFn * kb).from_buffer(ga, lo * ctypes.sizeof(_lib.PogsAmdFn))
            out = _Outputs(self.dtype, kb, self.m, self.n, rho=not plain)
            if plain:
                st = entry(self._h, kb, fb, gb, _ptr(rhos[lo:hi]), *tail, *out.pointers())
            else:
                xs = ls = flags = None
                if starts is not None and any(starts[2][lo:hi]):
                    xs = np.ascontiguousarray(starts[0][lo:hi])
                    ls = np.ascontiguousarray(starts[1][lo:hi])
                    flags = np.ascontiguousarray(starts[2][lo:hi], dtype=np.int32)
                st = lib.PogsAmdSolveBatchWarmFn(self._h, kb, fb, gb, _ptr(rhos[lo:hi]),
                                                 None if xs is None else _ptr(xs), None if ls is None else _ptr(ls),
                                                 None if flags is None else _ptr(flags), *tail, *out.pointers())
            if st != 0:
                raise RuntimeError("pogs_amd: batched solve failed: " + _lib.last_error())
            res += out.problems()
        del keep
        return res

    def _batch_starts(self, k, x0, l0, warm):
        """The starts of `solve_batch` as (k x n array, k x m array, k flags), or None when every problem is cold;
        ValueError for a start that does not fit.  Rows of cold problems are zero (they are never read)."""
        if x0 is None and l0 is None:
            if warm is not None and any(bool(w) for w in warm):
                raise ValueError("solve_batch: warm flags without x0 and l0")
            return None
        if x0 is None or l0 is None:
            raise ValueError("solve_batch: a warm start needs both x0 and l0")
        x0, l0 = list(x0), list(l0)
        flags = [True] * k if warm is None else [bool(w) for w in warm]
        if len(x0) != k or len(l0) != k or len(flags) != k:
            raise ValueError("solve_batch: %d problems, %d x0, %d l0 and %d warm flags" % (k, len(x0), len(l0), len(flags)))
        xs = np.zeros((k, self.n), self.dtype)
        ls = np.zeros((k, self.m), self.dtype)
        for j in range(k):
            if not flags[j]:
                continue
            if x0[j] is None or l0[j] is None:
                raise ValueError("solve_batch: problem %d is warm and has no x0 / l0" % j)
            xj, lj = np.asarray(x0[j], self.dtype), np.asarray(l0[j], self.dtype)
            if xj.shape != (self.n,) or lj.shape != (self.m,):
                raise ValueError("solve_batch: x0[%d] must have length %d and l0[%d] length %d" % (j, self.n, j, self.m))
            xs[j], ls[j] = xj, lj
        return xs, ls, flags

    def solve_chain(self, fs, gs, rho=1.0, slots=None, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, verbose=0,
                    adaptive_rho=True, gap_stop=True):
        """Solve problems whose neighbours in list order are similar (a sorted regularisation path) as warm-started
        batches: the list is cut into at most ``slots`` (default and at most BATCH_MAX) consecutive segments, round r
        solves element r of every segment in one batch (`_chain_schedule`), and each problem but the first of its
        segment starts from its predecessor's x, l and final rho.  The first of a segment, and the successor of a
        problem that ended neither solved nor at max_iter, starts cold at ``rho``.  Returns the list of dicts of
        `solve_batch` (with "rho") in problem order."""
        fs, gs = list(fs), list(gs)
        P = len(fs)
        if len(gs) != P:
            raise ValueError("solve_chain: %d f and %d g function vectors" % (P, len(gs)))
        res = [None] * P
        for rnd in _chain_schedule(P, slots):
            idx = [j for j, _ in rnd]
            x0, l0, warm, rhos = [], [], [], []
            for j, pred in rnd:
                prev = res[pred] if pred is not None else None
                ok = prev is not None and prev["status"] in (POGS_SUCCESS, POGS_MAX_ITER)
                warm.append(ok)
                x0.append(prev["x"] if ok else None)
                l0.append(prev["l"] if ok else None)
                rhos.append(prev["rho"] if ok else float(rho))
            kw = dict(rho=rhos, abs_tol=abs_tol, rel_tol=rel_tol, max_iter=max_iter, verbose=verbose,
                      adaptive_rho=adaptive_rho, gap_stop=gap_stop, return_rho=True)
            if any(warm):
                kw.update(x0=x0, l0=l0, warm=warm)
            got = self.solve_batch([fs[j] for j in idx], [gs[j] for j in idx], **kw)
            for j, r in zip(idx, got):
                res[j] = r
        return res

    def begin_run(self, f, g, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500, rho=1.0, adaptive_rho=True, gap_stop=True):
        args, keep = self._coef(f, g)
        st = lib.PogsAmdBeginRunFn(self._h, ctypes.byref(args[0]), ctypes.byref(args[1]), rho, abs_tol, rel_tol,
                                   int(max_iter), int(adaptive_rho), int(gap_stop))
        del keep
        if st != 0:
            raise RuntimeError("pogs_amd: begin_run failed: " + _lib.last_error())

    def iterate(self, iters):
        """Advance exactly `iters` ADMM iterations; returns (seconds, solves_completed)."""
        sec = ctypes.c_double()
        solves = ctypes.c_uint()
        st = lib.PogsAmdIterate(self._h, int(iters), ctypes.byref(sec), ctypes.byref(solves))
        if st != 0:
            raise RuntimeError("pogs_amd: iterate failed: " + _lib.last_error())
        return sec.value, solves.value

    def stats(self):
        s = _lib.PogsAmdStats()
        lib.PogsAmdGetStats(self._h, ctypes.byref(s))
        return s.as_dict()

    def reset_stats(self):
        lib.PogsAmdResetStats(self._h)

    def equilibrated(self, want_matrix=True):
        """(A_eq, d, e, nrmA) as the engine holds them (dense solvers)."""
        A_eq = np.zeros((self.m, self.n), self.dtype) if want_matrix else None
        d = np.zeros(self.m, self.dtype)
        e = np.zeros(self.n, self.dtype)
        nrm = ctypes.c_double()
        st = lib.PogsAmdGetEquil(self._h, _ptr(A_eq) if want_matrix else None, _ptr(d), _ptr(e), ctypes.byref(nrm))
        if st != 0:
            raise RuntimeError("pogs_amd: " + _lib.last_error())
        return A_eq, d, e, nrm.value

    def factor(self):
        """(W, U): W = L^-1 and U = W^T of the direct projector, L L^T = I + A_eq^T A_eq (m > n) or I + A_eq A_eq^T,
        each k x k with k = min(m, n): dense solvers, and sparse ones created with projector=PROJ_DIRECT
        (include/pogs_amd.h: PogsAmdGetFactor).  A handle that runs CGLS raises RuntimeError."""
        return _lib.get_factor(self._h, min(self._m_global or self.m, self.n), self.dtype)

    def project(self, x0, y0, tol=1e-8):
        x0 = np.ascontiguousarray(x0, self.dtype)
        y0 = np.ascontiguousarray(y0, self.dtype)
        x = np.zeros(self.n, self.dtype)
        y = np.zeros(self.m, self.dtype)
        st = lib.PogsAmdProject(self._h, _ptr(x0), _ptr(y0), tol, _ptr(x), _ptr(y))
        if st != 0:
            raise RuntimeError("pogs_amd: " + _lib.last_error())
        return x, y

    def mul(self, trans, alpha, x, beta, y):
        x = np.ascontiguousarray(x, self.dtype)
        y = np.array(y, dtype=self.dtype, copy=True)
        st = lib.PogsAmdMul(self._h, trans.encode()[0:1], alpha, _ptr(x), beta, _ptr(y))
        if st != 0:
            raise RuntimeError("pogs_amd: " + _lib.last_error())
        return y

    def close(self):
        if self._h:
            lib.PogsAmdDestroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ManySolver:
    """`solve_many`'s k problems kept on the GPU: every matrix is equilibrated and factored once, then re-solved
    with new functions (include/pogs_amd.h: PogsAmdManyCreate / PogsAmdManySolveFn).

    ``A`` as `solve_many` takes it; the handle owns its copy (a device tensor is read during construction only).
    All k problems stay resident: a set that does not fit is refused, `solve_many` solves such a set in chunks."""

    _STARTS = {"cold": _lib.MANY_COLD, "warm": _lib.MANY_WARM_GIVEN, "last": _lib.MANY_WARM_LAST}
    shapes = None        # a ragged handle (from_ragged): the k pairs (m_j, n_j)
    _h = None            # until a create entry has been called

    def __init__(self, A, dtype=None, device=-1):
        mats = _many_matrices(A, dtype)
        self.m, self.n = mats[1], mats[2]
        self._create(lib.PogsAmdManyCreate, mats, self.m, self.n, device)

    @classmethod
    def from_ragged(cls, As, dtype=None, device=-1, shapes=None, order="C"):
        """A handle over problems of unequal shapes (include/pogs_amd.h: PogsAmdManyCreateRagged).  ``As``,
        ``shapes`` and ``order`` as `solve_many_ragged` takes them.  `solve`, `info` and `close` work as on any
        ManySolver; ``x0`` / ``l0`` are lists of k per-problem arrays, and so are the results' 'x', 'y', 'l', 'mu'.
        ``m`` and ``n`` are the largest m_j and n_j, ``shapes`` the k pairs."""
        mats = _ragged_matrices(As, dtype, shapes, order, "ManySolver.from_ragged")
        k, ms, ns = mats[:3]
        self = cls.__new__(cls)
        self.m, self.n, self.shapes = max(ms), max(ns), list(zip(ms, ns))
        self._create(lib.PogsAmdManyCreateRagged, mats, (ctypes.c_size_t * k)(*ms), (ctypes.c_size_t * k)(*ns), device)
        return self

    def _create(self, entry, mats, m, n, device):
        """What both constructors end with: the call of the create entry on the matrices as `_many_matrices` /
        `_ragged_matrices` return them, ``m`` and ``n`` as that entry takes them."""
        k, _, _, aptr, mem, order, dt, tdev, keep_a = mats
        self._h = ctypes.c_void_p()
        self.k, self.dtype = k, np.dtype(dt)
        opt = _direct_options(tdev, device)
        st = entry(ctypes.byref(self._h), _code(self.dtype), int(order), k, m, n, aptr, mem, ctypes.byref(opt))
        if st != 0:
            self._h = ctypes.c_void_p()
            raise RuntimeError("pogs_amd: many-problem handle creation failed: " + _lib.last_error())
        _LIVE_SOLVERS.add(self)

    def get_shapes(self):
        """The k shapes (m_j, n_j) as the handle reports them (PogsAmdManyGetShapes); either kind of handle."""
        if not self._h:
            raise ValueError("ManySolver: the handle is closed")
        marr = (ctypes.c_size_t * self.k)()
        narr = (ctypes.c_size_t * self.k)()
        if lib.PogsAmdManyGetShapes(self._h, marr, narr) != 0:
            raise RuntimeError("pogs_amd: " + _lib.last_error())
        return list(zip(list(marr), list(narr)))

    def _starts(self, x0, l0):
        """The x0 / l0 of start="warm" as the entry reads them: k x n and k x m, or packed problem after problem."""
        k, dt = self.k, self.dtype
        if x0 is None or l0 is None:
            raise ValueError("ManySolver: start='warm' needs both x0 (k x n) and l0 (k x m)" if self.shapes is None else
                             "ManySolver: start='warm' needs both x0 and l0 (lists of k per-problem arrays)")
        if self.shapes is None:
            x0 = np.ascontiguousarray(x0, dtype=dt)
            l0 = np.ascontiguousarray(l0, dtype=dt)
            if x0.shape != (k, self.n) or l0.shape != (k, self.m):
                raise ValueError("ManySolver: x0 must be %d x %d and l0 %d x %d, got %s and %s"
                                 % (k, self.n, k, self.m, x0.shape, l0.shape))
            return x0, l0

        def packed(v, lens, name):
            v = list(v)
            if len(v) != k:
                raise ValueError("ManySolver: %s must be a list of %d per-problem arrays, got %d" % (name, k, len(v)))
            parts = [np.asarray(a, dtype=dt) for a in v]
            for j, a in enumerate(parts):
                if a.shape != (lens[j],):
                    raise ValueError("ManySolver: %s[%d] must have length %d, got shape %s"
                                     % (name, j, lens[j], a.shape))
            return np.ascontiguousarray(np.concatenate(parts))

        return packed(x0, [s[1] for s in self.shapes], "x0"), packed(l0, [s[0] for s in self.shapes], "l0")

    def solve(self, fs, gs, rho=None, start="cold", x0=None, l0=None, abs_tol=1e-4, rel_tol=1e-4, max_iter=2500,
              verbose=0, adaptive_rho=True, gap_stop=True):
        """Solve the k problems with (fs[j], gs[j]).  ``start``: "cold" (z = 0), "warm" (from ``x0``: k x n and
        ``l0``: k x m, the reference's SetInitX + SetInitLambda per problem) or "last" (from each problem's own last
        solution, kept on the device).  ``rho``: None, one value or k values; None means 1.0, and with "last" each
        problem's final rho of the last solve.  Returns `solve_many`'s dictionary plus 'rho', the final rho per
        problem.  On a ragged handle (`from_ragged`) x0 / l0 and the results' 'x', 'y', 'l', 'mu' are lists of k
        per-problem arrays."""
        k, dt, ragged = self.k, self.dtype, self.shapes is not None
        if not self._h:
            raise ValueError("ManySolver: the handle is closed")
        if start not in self._STARTS:
            raise ValueError("ManySolver: start must be 'cold', 'warm' or 'last', got %r" % (start,))
        if not ragged:
            fs, gs = _counted("ManySolver", k, fs, gs)      # (a uniform handle counts first, a ragged one after rho)
        if start == "warm":
            x0, l0 = self._starts(x0, l0)
        elif x0 is not None or l0 is not None:
            raise ValueError("ManySolver: x0 / l0 are read with start='warm' only")
        rhos = None if rho is None else _rho_vector("ManySolver", rho, k)
        ms, ns = ([s[0] for s in self.shapes], [s[1] for s in self.shapes]) if ragged else (self.m, self.n)
        fa, ga, keep = _fn_arrays("ManySolver", fs, gs, self.shapes if ragged else [(ms, ns)] * k, dt, each=ragged)
        out = _Outputs(dt, k, ms, ns, rho=True)
        st = lib.PogsAmdManySolveFn(self._h, fa, ga, None if rhos is None else _ptr(rhos), self._STARTS[start],
                                    None if x0 is None else _ptr(x0), None if l0 is None else _ptr(l0),
                                    *_tail(abs_tol, rel_tol, max_iter, verbose, adaptive_rho, gap_stop),
                                    *out.pointers())
        del keep
        if st != 0:
            raise RuntimeError("pogs_amd: many-problem solve failed: " + _lib.last_error())
        return out.arrays()

    def info(self):
        """k, m, n, dtype code, resident bytes, create's setup seconds and the last solve's loop seconds, launches
        and problem-iterations (include/pogs_amd.h: PogsAmdManyInfo)."""
        out = _lib.PogsAmdManyInfo()
        if lib.PogsAmdManyGetInfo(self._h, ctypes.byref(out)) != 0:
            raise RuntimeError("pogs_amd: " + _lib.last_error())
        return out.as_dict()

    def close(self):
        if self._h:
            lib.PogsAmdManyDestroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def prox_eval(f, rho, v, dtype=None):
    """Element-wise ProxEval on the GPU (reference: src/include/prox_lib.h:207-230)."""
    dt = _resolve_dtype(dtype)
    fa = _as_vector(f).arrays(dt)
    v = np.ascontiguousarray(v, dt)
    out = np.zeros_like(v)
    st = lib.PogsAmdProxEval(_lib.F64 if dt == np.float64 else _lib.F32, len(v), _ptr(fa["h"]), _ptr(fa["a"]),
                             _ptr(fa["b"]), _ptr(fa["c"]), _ptr(fa["d"]), _ptr(fa["e"]), rho, _ptr(v), _ptr(out))
    if st != 0:
        raise RuntimeError("pogs_amd: " + _lib.last_error())
    return out


def func_eval(f, v, dtype=None):
    """sum_i f_i(v_i) on the GPU (reference: src/include/prox_lib.h:326-349,520-529)."""
    dt = _resolve_dtype(dtype)
    fa = _as_vector(f).arrays(dt)
    v = np.ascontiguousarray(v, dt)
    out = ctypes.c_double()
    st = lib.PogsAmdFuncEval(_lib.F64 if dt == np.float64 else _lib.F32, len(v), _ptr(fa["h"]), _ptr(fa["a"]),
                             _ptr(fa["b"]), _ptr(fa["c"]), _ptr(fa["d"]), _ptr(fa["e"]), _ptr(v), ctypes.byref(out))
    if st != 0:
        raise RuntimeError("pogs_amd: " + _lib.last_error())
    return out.value


def proj_subgrad_eval(f, x, v, dtype=None):
    """Element-wise projection of v onto the subdifferential of f_i at x_i, on the GPU
    (reference: ProjSubgradEval, src/include/prox_lib.h:468-493, 538-546)."""
    dt = _resolve_dtype(dtype)
    fa = _as_vector(f).arrays(dt)
    x = np.ascontiguousarray(x, dt)
    v = np.ascontiguousarray(v, dt)
    assert x.shape == v.shape
    out = np.zeros_like(v)
    st = lib.PogsAmdProjSubgradEval(_lib.F64 if dt == np.float64 else _lib.F32, len(v), _ptr(fa["h"]), _ptr(fa["a"]),
                                    _ptr(fa["b"]), _ptr(fa["c"]), _ptr(fa["d"]), _ptr(fa["e"]), _ptr(x), _ptr(v),
                                    _ptr(out))
    if st != 0:
        raise RuntimeError("pogs_amd: " + _lib.last_error())
    return out


def rand_uniform(n, dtype=None):
    """The Norm2Est start vector (reference: src/cpu/include/gsl/gsl_rand.h:8-16)."""
    dt = _resolve_dtype(dtype)
    out = np.zeros(n, dt)
    lib.PogsAmdRandUniform(_lib.F64 if dt == np.float64 else _lib.F32, n, _ptr(out))
    return out


def dist_unique_id():
    buf = ctypes.create_string_buffer(_lib.UNIQUE_ID_BYTES)
    st = lib.PogsAmdDistUniqueId(buf)
    if st != 0:
        raise RuntimeError("pogs_amd: " + _lib.last_error())
    return buf.raw
