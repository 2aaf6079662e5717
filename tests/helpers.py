"""Shared helpers for the parity tests."""
import numpy as np

import pogs_amd
from pogs_amd import graph as G


def soa(fv):
    """FunctionVector -> dict of arrays as oracle_binding expects."""
    return {k: getattr(fv, k) for k in "habcde"}


def fn_arrays(fs, gs, dtype):
    """(fa, ga, keep) for a raw call of the library: the function vectors `fs` and `gs`, each at its own length, as two
    PogsAmdFn arrays (of one unused element where a list is empty), and the list that keeps their coefficient arrays
    alive."""
    from pogs_amd import _lib

    keep = []
    fa = (_lib.PogsAmdFn * max(len(fs), 1))()
    ga = (_lib.PogsAmdFn * max(len(gs), 1))()
    for arr, vectors in ((fa, fs), (ga, gs)):
        for j, v in enumerate(vectors):
            arr[j] = G._fn_struct(v, len(v), dtype, keep)
    return fa, ga, keep


def relerr(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


PROBLEMS = {
    "lasso": lambda b, n: G.lasso_functions(b, 0.1, n),
    "ridge": lambda b, n: G.ridge_functions(b, 0.5, n),
    "elastic_net": lambda b, n: G.elastic_net_functions(b, 0.1, 0.2, n),
    "logistic": lambda b, n: G.logistic_functions(np.sign(b) + (b == 0), 0.01, n),
    "logistic0": lambda b, n: G.logistic_functions(np.sign(b) + (b == 0), 0.0, n),
    "huber": lambda b, n: G.huber_functions(b, 1.0, 0.05, n),
    "svm": lambda b, n: G.svm_functions(np.sign(b) + (b == 0), 1.0, n),
    "nonneg_ls": lambda b, n: G.nonneg_ls_functions(b, n),
}


def objective(A, f, g, x):
    """sum f(Ax) + sum g(x) evaluated in float64 with numpy (independent of every engine)."""
    y = np.asarray(A @ x, np.float64).ravel()
    return _fsum(f, y) + _fsum(g, np.asarray(x, np.float64))


def _fsum(fv, v):
    h = fv.h
    a, b, c, d, e = fv.a, fv.b, fv.c, fv.d, fv.e
    t = a * v - b
    out = np.zeros_like(v)
    F = G.Function
    for code in np.unique(h):
        msk = h == code
        z = t[msk]
        if code == F.kAbs:
            r = np.abs(z)
        elif code == F.kSquare:
            r = 0.5 * z * z
        elif code == F.kLogistic:
            r = np.logaddexp(0, z)
        elif code == F.kHuber:
            r = np.where(np.abs(z) < 1, 0.5 * z * z, np.abs(z) - 0.5)
        elif code == F.kMaxPos0:
            r = np.maximum(z, 0)
        elif code == F.kMaxNeg0:
            r = np.maximum(-z, 0)
        elif code == F.kIdentity:
            r = z
        elif code in (F.kZero, F.kIndGe0, F.kIndLe0, F.kIndEq0, F.kIndBox01):
            r = np.zeros_like(z)
        else:
            raise NotImplementedError(code)
        out[msk] = r
    return float(np.sum(c * out + d * v + 0.5 * e * v * v))


def run_row_sharded(pogs, A, f, g, world, dtype, solver_kw=None, count_collectives=False, transport="1", bounds=None,
                    **solve_kw):
    """Solves with `world` ranks inside this process: one thread + one Solver per rank, rows split
    evenly, joined by the engine's in-process test communicator ("POGSLOCAL:" unique id, see
    pogs_amd/csrc/dist.h).  Verifies the engine's own row-sharded decomposition on ONE GPU.
    Returns the per-rank result dicts (x replicated, y / l row slices)."""
    import os
    import threading

    import numpy as np

    # the in-process communicator is refused without it; "1": stream-ordered (device slots + events, no
    # stream is ever waited for), "host": staged through the host (pogs_amd/csrc/dist.h)
    os.environ["POGS_AMD_TEST_TRANSPORT"] = transport
    m = A.shape[0]
    uid = (b"POGSLOCAL:" + os.urandom(8).hex().encode()).ljust(128, b"\0")
    # rows split evenly unless the caller names the shard boundaries (unequal shards)
    bounds = np.linspace(0, m, world + 1).astype(int) if bounds is None else np.asarray(bounds, int)
    assert len(bounds) == world + 1 and bounds[0] == 0 and bounds[-1] == m
    results, errors = [None] * world, []

    def work(r):
        try:
            lo, hi = int(bounds[r]), int(bounds[r + 1])
            with pogs.Solver(A[lo:hi], dtype=dtype, dist=(r, world, m, uid), **(solver_kw or {})) as s:
                results[r] = s.solve(f.slice(lo, hi), g, **solve_kw)
                if count_collectives:
                    # a second solve on the same handle (factorisation cached): its all-reduce calls
                    # are the iteration loop's alone
                    st0 = s.stats()
                    again = s.solve(f.slice(lo, hi), g, **solve_kw)
                    st1 = s.stats()
                    results[r]["loop_collectives"] = dict(
                        calls=st1["collectives"] - st0["collectives"], iterations=int(again["iterations"]) + 1,
                        misses=int(st1["spec_misses"] - st0["spec_misses"]), hits=int(st1["spec_hits"] - st0["spec_hits"]))
        except Exception as e:  # pragma: no cover - surfaced below
            errors.append((r, e))

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(600)
    assert not errors, errors
    assert all(r is not None for r in results)
    return results, bounds


def run_sharded_oracle(A, f, g, world, dtype, bounds=None, **solve_kw):
    """The ORACLE's row-sharded entry (oracle/pogs_oracle.cpp: OraclePogsShard* / OraclePogsSparseShard*)
    with `world` ranks as threads of this process and an in-test sum in rank order as the collective.
    Returns (per-rank result dicts, bounds) with the same row split as run_row_sharded."""
    import threading

    import oracle_binding as ob

    m = A.shape[0]
    bounds = np.linspace(0, m, world + 1).astype(int) if bounds is None else np.asarray(bounds, int)
    bar = threading.Barrier(world)
    slots = [None] * world
    results, errors = [None] * world, []

    def make_allreduce(r):
        def allreduce(arr):
            slots[r] = arr.copy()
            bar.wait(600)
            total = slots[0].copy()
            for q in range(1, world):
                total += slots[q]
            bar.wait(600)   # nobody overwrites a slot that is still being read
            arr[:] = total
        return allreduce

    def work(r):
        try:
            lo, hi = int(bounds[r]), int(bounds[r + 1])
            results[r] = ob.oracle_solve_shard(A[lo:hi], m, soa(f.slice(lo, hi)), soa(g), make_allreduce(r), dtype=dtype,
                                               **solve_kw)
        except Exception as e:  # pragma: no cover - surfaced below
            errors.append((r, e))
            bar.abort()

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(900)
    assert not errors, errors
    assert all(r is not None for r in results)
    return results, bounds


# ---- kernels against high-precision references (test_gpu_batch_kernels.py, test_gpu_factor_kernels.py) -----------

def gamma(n, dt, u=None):
    """gamma_n = n u / (1 - n u); u: the unit roundoff of dt (eps / 2) unless given (eps for an accumulate that truncates)"""
    u = np.finfo(dt).eps / 2 if u is None else u
    return n * u / (1 - n * u)


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def ints(rng, shape, dt):
    return rng.integers(-4, 5, shape).astype(dt)


def scaled_normal(rng, shape):
    """standard_normal with rows and columns scaled by 2^-10 .. 2^10"""
    r, c = shape
    return rng.standard_normal(shape) * np.exp2(rng.uniform(-10, 10, (r, 1))) * np.exp2(rng.uniform(-10, 10, (1, c)))


def hi(a):
    """the precision of a reference: fp64 for fp32 data, long double for fp64 data"""
    return np.asarray(a, np.longdouble if a.dtype == np.float64 else np.float64)


def within_gamma(got, ref, absref, n, dt):
    err = np.abs(hi(got) - ref)
    bar = gamma(n, dt) * absref
    assert np.all(np.isfinite(got))
    assert np.all(err <= bar), float(np.max(err - bar))


def _w_bars(m, n, dt, gram=True):
    """Bars of W = L^-1 (L L^T = H = I + G, G = A_eq^T A_eq or A_eq A_eq^T, K = min(m, n), R = max(m, n)).

    ||A_eq||_F^2 = K (the equilibration's normalisation), so 1 <= lambda(H) <= 1 + K: cond(H) <= 1 + K,
    ||W||_2 <= 1 and ||W||_F^2 = trace(H^-1) <= K, ||L||_F^2 = trace(H) = 2K.
      Gram (R-term dot products in T):   ||dG||_2 <= ||dG||_F <= gamma_R || |A|^T |A| ||_F <= gamma_R K
      Cholesky (backward):               L^ L^T = H + dG + dC, ||dC||_2 <= gamma_(K+1) ||L^||_F^2 = gamma_(K+1) 2K
      inversion (W^ L^ = I + E):         ||E||_2 <= gamma_K ||W^||_F ||L^||_F <= gamma_K sqrt(2) K
    so the residual R = W^ H W^T - I = (I + E)(I + E)^T - I - W^ (dG + dC) W^T has
      ||R||_2 <= r := 2 e + e^2 + gamma_R K + 2 gamma_(K+1) K,  e = sqrt(2) gamma_K K,
    plus its evaluation in fp64 (two products of K-term sums: 2 gamma64_(2K) ||W^||_2^2 ||H||_2 <= 2 gamma64_(2K) (1 + K)).
    W^ L = T is lower triangular with T T^T = I + R: T is the Cholesky factor of I + R, so T = I + F with
    ||F||_F <= ||R||_F / (sqrt(2) (1 - ||R||_2)) <= sqrt(K) r / (1 - r), and W^ - W = F W: |W^ - W|_max <= ||F||_F
    ||W||_2 <= sqrt(K) r / (1 - r), plus the fp64 reference's own error (the same bound with u of fp64).
    gram=False: H itself is the input (no Gram product in T): the gamma_R K term is left out."""
    K, R = min(m, n), max(m, n)

    def r_of(d):
        e = np.sqrt(2) * gamma(K, d) * K
        return 2 * e + e * e + (gamma(R, d) * K if gram else 0.0) + 2 * gamma(K + 1, d) * K

    r = r_of(dt)
    r64 = r_of(np.float64)
    res_bar = r + 2 * gamma(2 * K, np.float64) * (1 + K)
    w_bar = np.sqrt(K) * (r / (1 - r) + r64 / (1 - r64))
    return res_bar, w_bar


def xmatmul(A, B, slices=4):
    """A @ B for float64 matrices as a long double array, every entry within about n 2^-76 of (largest |entry| of
    A's row) x (largest of B's column): error-free slicing (Ozaki's scheme).  Each operand is cut into `slices` pieces
    of beta bits below its row / column maximum, beta so small that a product of two pieces is a sum of n integers
    below 2^53 in a common unit -- exact in a float64 BLAS whatever its order of summation; the piece products are
    then added in long double, smallest first.  (numpy multiplies long double matrices without a BLAS, about a
    thousand times slower.)"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    n = A.shape[1]
    beta = (53 - int(np.ceil(np.log2(max(n, 2)))) - 1) // 2

    def cut(M, axis):
        mx = np.max(np.abs(M), axis=axis, keepdims=True)
        q = np.ceil(np.log2(np.where(mx > 0, mx, 1.0))).astype(np.int64)        # |M| <= 2^q along the axis
        rem, parts = M.copy(), []
        for s in range(slices):
            c = np.ldexp(1.5, q - beta * (s + 1) + 52)       # ulp(c) = 2^(q - beta (s + 1)): adding c rounds to it
            piece = (rem + c) - c
            rem = rem - piece                                 # exact
            parts.append(piece)
        return parts

    pa, pb = cut(A, 1), cut(B, 0)
    out = np.zeros((A.shape[0], B.shape[1]), np.longdouble)
    for tot in range(slices - 1, -1, -1):
        for i in range(tot + 1):
            out += pa[i] @ pb[tot - i]
    return out
