"""CPU test: the oracle's ProxEval against the DEFINITION of a prox, on the grid of prox_grid.py.

x = prox(v) is the root of  c a h'(a x - b) + d + e x + rho (x - v) = 0.  The root is found by bisection on t = a x - b
(a times the left-hand side increases in t) on the inputs as the working dtype holds them; the condition is evaluated in
long double so that the root's own error lies below the fp64 rounding that is measured.  Functions: the five
differentiable ones behind a root finder or a cancellation (kExp, kLogistic, kNegEntr, kNegLog, kRecipr), with unit and with
random coefficients.

The reference's algorithm is right to rounding except in three regions, which the oracle, the compiled reference and the
device share.  They are pinned here as what the algorithm does, not as what a prox is:
  * kExp / kNegEntr with a Lambert argument > 100 (v' - log rho', resp. rho' v' - 1 + log rho'): the asymptotic seed is
    returned as is;
  * kRecipr at v' < 0: the prox of v' = 0 is returned;
  * kNegLog at v' < 0: (v' + sqrt(v'^2 + 4 / rho')) / 2 cancels.
(v', rho': ProxEval's change of variable.)  Outside them the distances measured when the test was written (unit
coefficients: fp64 rel 2e-13, kLogistic abs 4.5e-11; fp32 rel 2e-6 for kNegEntr / kRecipr / kNegLog at v' >= 0, kExp abs
7e-6, kLogistic abs 6e-6) are asserted with a margin of 4.  A relative distance is asserted where the true prox is a normal
number with a full mantissa to lose (|x| >= tiny / eps of the working dtype).  test_zz_report prints the table
profiles/prox_definition_accuracy.txt holds."""
import numpy as np
import pytest

import oracle_binding as ob
from prox_grid import K_EXP, K_LOGISTIC, K_NEGENTR, K_NEGLOG, K_RECIPR, RHOS, ROOT_FNS, V, coefficients, transformed

L = np.longdouble
NAMES = {K_EXP: "kExp", K_LOGISTIC: "kLogistic", K_NEGENTR: "kNegEntr", K_NEGLOG: "kNegLog", K_RECIPR: "kRecipr"}
TABLE = {}      # (dtype, function, coefficients, where) -> [max abs, max rel, points]


def h_prime(h, t):
    with np.errstate(all="ignore"):
        if h == K_EXP:
            return np.exp(t)
        if h == K_LOGISTIC:
            return 1 / (1 + np.exp(-t))
        if h == K_NEGENTR:
            return np.log(t) + 1
        if h == K_NEGLOG:
            return -1 / t
        return -1 / (t * t)


def true_prox(h, f, v, rho):
    """the root in long double, from the inputs as given (fp64 values)"""
    a, b, c, d, e = (f[k].astype(L) for k in "abcde")
    v, rho = v.astype(L), L(rho)

    def g(t):       # a * (c a h'(t) + d + e x + rho (x - v)),  x = (t + b) / a
        x = (t + b) / a
        with np.errstate(all="ignore"):
            return a * (c * a * h_prime(h, t) + d + e * x + rho * (x - v))

    vp, rp = transformed({k: f[k].astype(L) for k in "abcde"}, v, rho)
    if h in (K_EXP, K_LOGISTIC):        # h' in (0, 1] left of 0, h' > 0: the root lies in [min(v', 0) - 1 / rho' - 1, v' + 1]
        lo, hi = np.minimum(vp, 0) - 1 / rp - 1, vp + 1
    else:                               # t > 0, g(0+) = -inf
        lo, hi = np.full_like(vp, L("1e-4900")), np.maximum(np.abs(vp), 1) + 1
        for _ in range(64):
            low = g(hi) < 0
            if not np.any(low):
                break
            hi = np.where(low, 2 * hi, hi)
    assert np.all(g(hi) >= 0) and (h not in (K_EXP, K_LOGISTIC) or np.all(g(lo) <= 0))      # (t > 0: a root below lo is lo)
    for _ in range(240):
        # (a positive bracket that spans binades is halved in the exponent: a root of 1e-196 is found as fast as one of 1)
        wide = (lo > 0) & (hi > 4 * lo)
        mid = np.where(wide, np.sqrt(np.where(wide, lo, 1)) * np.sqrt(np.where(wide, hi, 1)), (lo + hi) / 2)
        up = g(mid) < 0
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    return (((lo + hi) / 2 + b) / a).astype(np.float64)


def lambert_arg(h, vp, rp):
    with np.errstate(all="ignore"):
        return vp - np.log(rp) if h == K_EXP else (rp * vp - 1) + np.log(rp)


def lambert_seed(x):
    lx = np.log(x)
    return -0.36962844 + x - 0.97284858 * lx + 1.3437973 / lx


def record(dt, h, coef, where, got, want):
    err = np.abs(got.astype(np.float64) - want)
    fin = np.finfo(dt)
    big = np.abs(want) >= fin.tiny / fin.eps
    rel = np.where(big, err / np.where(big, np.abs(want), 1), 0.0)
    key = (np.dtype(dt).name, NAMES[h], coef, where)
    row = TABLE.setdefault(key, [0.0, 0.0, 0])
    if err.size:
        row[0], row[1], row[2] = max(row[0], float(err.max())), max(row[1], float(rel.max())), row[2] + err.size
    return err, rel


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("coef", ["unit", "random"])
@pytest.mark.parametrize("h", ROOT_FNS)
def test_prox_against_its_definition(dt, coef, h):
    eps = np.finfo(dt).eps
    rng = np.random.default_rng(100 + h) if coef == "random" else None
    for rho in RHOS:
        rho = dt(rho)
        v = V.astype(dt)
        f = coefficients(h, v.size, dt, rng)
        got = ob.oracle_prox(f, float(rho), v, dtype=dt)
        assert got.dtype == dt and np.all(np.isfinite(got))
        f64 = {k: (f[k] if k == "h" else f[k].astype(np.float64)) for k in f}
        want = true_prox(h, f64, v.astype(np.float64), float(rho))
        vp, rp = transformed(f, v, rho)                    # in the working dtype, as ProxEval forms them
        vp64, rp64 = transformed(f64, v.astype(np.float64), float(rho))
        a, b = f["a"], f["b"]
        if h in (K_EXP, K_NEGENTR):
            arg = lambert_arg(h, vp, rp).astype(np.float64)                # the argument the library sees
            mag = np.abs(vp64) + np.abs(np.log(rp64)) if h == K_EXP else np.abs(rp64 * vp64) + 1 + np.abs(np.log(rp64))
            edge = np.abs(lambert_arg(h, vp64, rp64) - 100) <= 8 * eps * mag       # either branch, by rounding
            inside = (arg > 100) & ~edge
            outside = (arg <= 100) & ~edge
            # inside: the seed formula, evaluated in double on the working-dtype argument
            w = lambert_seed(np.where(arg > 100, arg, 101.0)).astype(dt)
            model = ((vp - w) + b) / a if h == K_EXP else (w / rp + b) / a
            slack = 8 * eps * (np.abs(vp) + np.abs(w) + np.abs(b)) / np.abs(a) if h == K_EXP else 8 * eps * (np.abs(w / rp) + np.abs(b)) / np.abs(a)
            assert np.all(np.abs(got.astype(np.float64) - model)[inside] <= slack[inside])
            at_edge = np.abs(got.astype(np.float64) - model) <= slack
            record(dt, h, coef, "Lambert argument > 100", got[inside], want[inside])
        elif h == K_RECIPR:
            inside, edge = vp < 0, np.zeros(v.size, bool)
            if coef == "unit":           # the prox of v = 0, bit for bit
                at0 = ob.oracle_prox({k: f[k][:1] for k in f}, float(rho), np.zeros(1, dt), dtype=dt)[0]
                assert np.all(got[inside] == at0)
            with np.errstate(all="ignore"):
                t0 = np.power(1 / rp, dt(1) / dt(3))       # CubicSolve(0, 0, -1 / rho'): the cube root of 1 / rho'
            model = (t0 + b) / a
            assert np.all(np.abs(got - model)[inside] <= (8 * eps * (np.abs(t0) + np.abs(b)) / np.abs(a))[inside])
            outside = ~inside
            record(dt, h, coef, "v' < 0", got[inside], want[inside])
        elif h == K_NEGLOG:
            inside, edge = vp < 0, np.zeros(v.size, bool)
            model = ((vp + np.sqrt(vp * vp + dt(4) / rp)) / dt(2) + b) / a      # the cancelling form in the working dtype
            assert model.dtype == dt and np.array_equal(got[inside], model[inside])
            outside = ~inside
            record(dt, h, coef, "v' < 0", got[inside], want[inside])
        else:
            inside, edge, outside = np.zeros(v.size, bool), np.zeros(v.size, bool), np.ones(v.size, bool)
        err, _ = record(dt, h, coef, "elsewhere", got[outside], want[outside])
        bar = bound(dt, h, coef, f64, want, vp64, rp64)
        ok = err <= bar[outside]
        assert np.all(ok), (NAMES[h], float(rho), float(err[~ok].max()), float((err / bar[outside])[~ok].max()), v[outside][~ok][:5])
        if np.any(edge):                 # next to argument 100 either branch may be taken: one of the two statements holds
            e2, _ = record(dt, h, coef, "elsewhere", got[edge], want[edge])
            assert np.all(at_edge[edge] | (e2 <= bar[edge]))


def bound(dt, h, coef, f64, want, vp64, rp64):
    """the distance asserted outside the three regions: 4 x the figures measured with unit coefficients when the test was
    written, an absolute one for kLogistic and fp32 kExp, a relative one otherwise.
      * relative means relative to |x|, from tiny / eps up; for kExp, whose prox v' - W crosses zero, to max(|x|, |v' / a|):
        the library computes W, and x inherits W's rounding where the two cancel;
      * fp32 kNegEntr left of v' = 0 (the figure is for v' >= 0): the result is W(e^arg) / rho' with d log W / d arg <= 1, and
        the fp32 argument rho' v' - 1 + log rho' carries the rounding of its terms;
      * random coefficients add what the unit-coefficient figures cannot contain, the working-dtype rounding of the change
        of variable and of the result: 4 eps (|v'| + |b|) / |a|;
      * fp32 kLogistic: the figure (6e-6) is not reproduced at rho = 1e-3, where the residual is formed from x - v of
        magnitude up to 1 / rho' = 1000 rounded to fp32 (measured 1.3e-4): 4 eps (|v'| + 1 / rho') / |a| is added there too."""
    f32 = dt == np.float32
    fin = np.finfo(dt)
    a, b = np.abs(f64["a"]), np.abs(f64["b"])
    scale = np.maximum(np.abs(want), fin.tiny / fin.eps)
    if h == K_LOGISTIC:
        bar = np.full(want.shape, 4 * (6e-6 if f32 else 4.5e-11))
    elif h == K_EXP and f32:
        bar = np.full(want.shape, 4 * 7e-6)
    elif h == K_EXP:
        bar = 4 * 2e-13 * np.maximum(scale, np.abs(vp64) / a)
    else:
        bar = 4 * (2e-6 if f32 else 2e-13) * scale
    if h == K_NEGENTR and f32:
        bar = bar + np.where(vp64 < 0, 4 * fin.eps * (np.abs(rp64 * vp64) + 1 + np.abs(np.log(rp64))), 0.0) * scale
    if coef == "random" or (h == K_LOGISTIC and f32):
        bar = bar + 4 * fin.eps * (np.abs(vp64) + b + (1 / rp64 if h == K_LOGISTIC else 0)) / a
    return bar


def test_zz_report():
    """prints the distance to the true prox per dtype, function, coefficient set and region"""
    for key, (err, rel, cnt) in sorted(TABLE.items()):
        print("PROXDEF %-8s %-10s %-7s %-24s abs %.3e rel %.3e (%d points)" % (key + (err, rel, cnt)))
