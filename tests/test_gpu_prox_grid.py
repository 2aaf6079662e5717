"""GPU tests of the prox library (csrc/prox.h through PogsAmdProxEval, PogsAmdFuncEval, PogsAmdProjSubgradEval) against the
oracle on the grid of prox_grid.py -- v in [-60, 60] and [90, 1200], rho in {1e-3, 0.1, 1, 7.5, 1e3} -- which reaches the
branches the N(0, 3) data of test_prox_library_matches_oracle never takes (the asymptotic Lambert seed, ProxLogistic
brackets up to 1000 wide, NegLog's cancellation, kRecipr left of 0), at sizes that are no multiple of the 256-thread block.

Tolerances: fp64 those of test_prox_library_matches_oracle; fp32 its rtol per function and its atol scaled by max(1, |v|)
(an fp32 input carries eps |v|, and a prox is non-expansive).  The three regions where the reference's algorithm departs
from the true prox (test_prox_definition_host.py) are the oracle's and the device's alike, so they need no allowance here.
Non-finite results must be non-finite on both sides, at the same places."""
import numpy as np
import pytest

import oracle_binding as ob
import pogs_amd
from prox_grid import RHOS, V, coefficients

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
SIZES = [1, 255, 256, 257, 1000]
WORST = {}      # (what, dtype) -> (largest error / tolerance, function, rho)


def fvec(f):
    return pogs_amd.FunctionVector(len(f["h"]), *(f[k] for k in "habcde"))


def prox_tol(dt, h, want, v):
    if dt == np.float64:
        return 1e-9 + 1e-9 * np.abs(want)
    rtol = 5e-4 if h in (1, 8, 11, 13) else 5e-5
    atol = 5e-5 if h == 8 else 1e-5
    return atol * np.maximum(1.0, np.abs(v)) + rtol * np.abs(want)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("coef", ["unit", "random"])
def test_prox_on_the_grid_matches_oracle(dt, coef):
    rng = np.random.default_rng(7) if coef == "random" else None
    v = V.astype(dt)
    for h in range(16):
        f = coefficients(h, v.size, dt, rng)
        for rho in RHOS:
            rho = float(dt(rho))
            got = pogs_amd.prox_eval(fvec(f), rho, v, dtype=dt)
            want = ob.oracle_prox(f, rho, v, dtype=dt)
            assert got.dtype == dt and got.shape == want.shape
            ok = np.isfinite(want)
            assert np.array_equal(np.isfinite(got), ok), (h, rho)
            err = np.abs(got[ok].astype(np.float64) - want[ok])
            tol = prox_tol(dt, h, want[ok].astype(np.float64), v[ok].astype(np.float64))
            r = float(np.max(err / tol)) if err.size else 0.0
            key = ("prox " + coef, np.dtype(dt).name)
            if r > WORST.get(key, (0.0,))[0]:
                WORST[key] = (r, h, rho)
            print("PROXGRID %s %s h=%2d rho=%-8g worst error / tolerance %.3e" % (coef, np.dtype(dt).name, h, rho, r))
            assert r <= 1.0, (h, rho, r, v[ok][np.argmax(err / tol)])
            # the sizes around one block: the last n points of the grid (the large v), bit for bit what the full launch gave
            for n in (1, 255, 257):
                part = pogs_amd.prox_eval(fvec({k: f[k][-n:] for k in f}), rho, v[-n:], dtype=dt)
                assert part.shape == (n,) and np.array_equal(part.view(np.uint8), got[-n:].view(np.uint8)), (h, rho, n)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_func_eval_block_partials_and_domain_edges(dt, n):
    """the per-block partials and their host sum: every element is counted once, at every size; NegLog and Recipr give
    +inf at a v - b <= 0 and NegEntr gives 0, on both sides of the edge"""
    rng = np.random.default_rng(n)
    rel = 1e-10 if dt == np.float64 else 2e-4
    spots = sorted({i for i in (0, 254, 255, 256, n - 1) if i < n})
    for h in range(16):
        f = coefficients(h, n, dt, rng)
        f["a"] = np.abs(f["a"])          # (as test_func_eval_matches_oracle: the terms of the sum do not cancel)
        v = rng.uniform(0.1, 3.0, n).astype(dt)
        inner = f["a"].astype(np.float64) * v - f["b"]
        v = np.where(inner <= 0.05, ((f["b"] + dt(0.5)) / f["a"]).astype(dt), v)       # inside every domain
        got, want = pogs_amd.func_eval(fvec(f), v, dtype=dt), ob.oracle_func(f, v, dtype=np.float64)
        assert np.isfinite(want) and got == pytest.approx(want, rel=rel), (h, n)
    # one non-zero element at a time: 0.5 v^2 of a single v = 3 is 4.5 wherever it sits
    sq = coefficients(14, n, dt)
    for at in spots:
        v = np.zeros(n, dt)
        v[at] = 3
        assert pogs_amd.func_eval(fvec(sq), v, dtype=dt) == 4.5, at
    # the domain edge a v - b = 0 with a = 1, b = 0.5 (v = 0.5 exactly), one step below it and one above
    for h, at_edge in ((12, np.inf), (13, np.inf), (11, 0.0)):
        f = coefficients(h, n, dt)
        f["b"][:] = 0.5
        base = np.full(n, 2.5, dt)
        inside = pogs_amd.func_eval(fvec(f), base, dtype=dt)
        assert inside == pytest.approx(ob.oracle_func(f, base, dtype=np.float64), rel=rel)
        for at in spots:
            for edge in (dt(0.5), np.nextafter(dt(0.5), dt(0)), dt(-3)):
                v = base.copy()
                v[at] = edge
                got, want = pogs_amd.func_eval(fvec(f), v, dtype=dt), ob.oracle_func(f, v, dtype=dt)
                if np.isinf(at_edge):
                    assert got == np.inf and want == np.inf, (h, at, edge)
                else:
                    assert np.isfinite(got) and got == pytest.approx(want, rel=rel, abs=1e-12), (h, at, edge)
            above = base.copy()
            above[at] = np.nextafter(dt(0.5), dt(1))
            got, want = pogs_amd.func_eval(fvec(f), above, dtype=dt), ob.oracle_func(f, above, dtype=dt)
            assert np.isfinite(want) and got == pytest.approx(want, rel=rel), (h, at)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_proj_subgrad_at_sizes_around_a_block(dt, n):
    rng = np.random.default_rng(n + 5)
    rtol, atol = (1e-11, 1e-11) if dt == np.float64 else (5e-5, 1e-5)
    for h in range(16):
        f = coefficients(h, n, dt, rng)
        x = rng.normal(0, 1.5, n).astype(dt)
        x[::7] = (f["b"][::7] / f["a"][::7]).astype(dt)          # on the kink a x - b = 0, as far as the dtype holds it
        v = rng.normal(0, 2.0, n).astype(dt)
        got = pogs_amd.graph.proj_subgrad_eval(fvec(f), x, v, dtype=dt)
        want = ob.oracle_proj_subgrad(f, x, v, dtype=dt)
        fin = np.isfinite(want)
        assert got.shape == (n,) and np.array_equal(np.isfinite(got), fin), h
        np.testing.assert_allclose(got[fin], want[fin], rtol=rtol, atol=atol, err_msg="h=%d n=%d" % (h, n))


def test_zz_report():
    for (what, dt), (r, h, rho) in sorted(WORST.items()):
        print("PROXGRID worst %-12s %-8s %.3e of the tolerance (h=%d, rho=%g)" % (what, dt, r, h, rho))
