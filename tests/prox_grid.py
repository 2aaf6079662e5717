"""The grid on which the prox library is compared with the definition of a prox (test_prox_definition_host.py) and the
device with the oracle (test_gpu_prox_grid.py): v in [-60, 60] and [90, 1200], rho in {1e-3, 0.1, 1, 7.5, 1e3}.  It reaches
the branches the N(0, 3) data of test_prox_library_matches_oracle never takes: the asymptotic Lambert seed (argument
> 100), ProxLogistic brackets wider than 10 (rho = 1e-3: 1000), the cubic's three-real-root form, NegLog's cancellation.

Every v is a multiple of 1/4 below 2^11, so the grid is the same in fp32 and fp64; rho is rounded to the working dtype
before anything is derived from it."""
import numpy as np

RHOS = (1e-3, 0.1, 1.0, 7.5, 1e3)
V = np.concatenate([np.arange(-240, 241) * 0.25, 90.0 + 5.0 * np.arange(223)])      # 704 values: 2.75 blocks of 256
assert V.size % 256 != 0 and np.array_equal(V, V.astype(np.float32))

K_EXP, K_LOGISTIC, K_NEGENTR, K_NEGLOG, K_RECIPR = 1, 8, 11, 12, 13
ROOT_FNS = (K_EXP, K_LOGISTIC, K_NEGENTR, K_NEGLOG, K_RECIPR)      # differentiable, behind a root finder or a cancellation


def coefficients(h, n, dt, rng=None):
    """unit coefficients, or random ones as FunctionObj admits them (c, e >= 0), rounded to dt.  b >= 0 so that the
    result (t + b) / a does not cancel for the functions with the domain t > 0: a relative error is then a statement
    about the root t and not about how close b / a lies to it."""
    one = np.ones(n, dt)
    if rng is None:
        return dict(h=np.full(n, h, np.int32), a=one, b=0 * one, c=one.copy(), d=0 * one, e=0 * one)
    return dict(h=np.full(n, h, np.int32), a=(rng.uniform(0.5, 2.0, n) * rng.choice([-1, 1], n)).astype(dt),
                b=np.abs(rng.normal(0, 0.5, n)).astype(dt), c=rng.uniform(0.2, 3.0, n).astype(dt),
                d=rng.normal(0, 0.3, n).astype(dt), e=rng.uniform(0.0, 1.0, n).astype(dt))


def transformed(f, v, rho):
    """(v', rho') of ProxEval's change of variable t = a x - b, in the dtype of the inputs"""
    a, b, c, d, e = (f[k] for k in "abcde")
    return a * (v * rho - d) / (e + rho) - b, (e + rho) / (c * a * a)
