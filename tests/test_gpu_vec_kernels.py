"""GPU tests of the kernels that do not read the matrix (csrc/vec_kernels.hip), one launch at a time through
PogsAmdVecCheck (include/pogs_amd.h, Part 3), which calls the launch functions and block-count helpers the solvers call.
No iteration is modelled: every output is a function of the call's own inputs.

Layout and poison (tests/test_gpu_dense_passes.py): every vector is three elements longer than it need be, inputs NaN
there (function ids 9999), outputs a sentinel that must come back; the device's partial-sum buffer starts as NaN (the
entry does that) and comes back whole, so a record no workgroup wrote poisons the total that reads it and a record too many
shows in the NaN tail.

Three kinds of check:
  * exact integers: entries in [-4, 4]; rho, zt_scale powers of two, alpha 1 or 1.5, a = c = 1, b = d = e = 0 and the
    functions of EXACT_FNS, so that every intermediate is a multiple of 1/8 the mantissa holds: every output, every raw
    partial and every sum equals the fp64 model whatever the order of summation -- a wrong slot, a wrong block offset, a
    skipped or a double-counted element fails here;
  * real, badly scaled data (scaled_normal) with random coefficients: the unit is built with -ffp-contract=off and nothing
    in these kernels but the prox of the four expensive functions calls a math-library function beyond sqrt, so every
    element-wise output is reproduced in numpy in the working dtype, bit for bit; partial records and sums are fp64
    fused accumulations of exact products, within gamma_32 (a record: at most 4 accumulations per thread, 6 tree levels,
    4 waves) or gamma_(nparts+32) (a total) of the long double sum of the device's own z12 and the reproduced w;
  * uniform coefficients: an array the mask declares uniform holds NaN (9999 for h) and the launch must give the bytes
    of the per-element launch."""
import numpy as np
import pytest

import pogs_amd
from helpers import gamma, hi, ints, same_bytes, scaled_normal
from pogs_amd import _lib as P
from test_gpu_dense_passes import CHEAP_FNS, EXACT_FNS, fn_arrays, prox_exact

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SENT = -7.375e-3
PRE_SIZES = [(1, 1), (255, 1025), (1024, 1023), (1025, 257), (2049, 4097), (3000, 5)]
VEC_SIZES = [1, 255, 256, 257, 1000]
SUM_NPARTS = [1, 255, 256, 257, 768, 769, 1023, 1024, 1025, 1793, 2049]
PRE_CHUNK = 1024      # elements per workgroup of admm_pre_kernel (kVecTpb * kPreU)
VEC_CHUNK = 256
RATIOS = {}           # (what, dtype name) -> largest observed error / bound (printed by test_zz_report)


def note(what, dt, err, bar):
    err, bar = np.asarray(err, np.float64), np.asarray(bar, np.float64)
    ok = bar > 0
    r = float(np.max(np.where(ok, err / np.where(ok, bar, 1), np.where(err > 0, np.inf, 0)))) if err.size else 0.0
    key = (what, np.dtype(dt).name)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    return r


def bounded(what, dt, got, ref, bar):
    """|got - ref| <= bar elementwise against a long double reference; the largest ratio is recorded"""
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), what
    err = np.abs(got.astype(np.longdouble) - ref)
    r = note(what, dt, err, bar)
    assert np.all(err <= bar), (what, r)


def inp(dt, n, vals):
    x = np.full(n + 3, np.nan, dt)
    x[:n] = vals
    return x


def outp(dt, n):
    return np.full(n + 3, SENT, dt)


def kept(arr, n):
    """the three elements beyond n hold the sentinel"""
    return np.all(arr[n:] == np.asarray(SENT, arr.dtype)) and arr.size == n + 3


def scaled(rng, n, dt):
    """badly scaled data, kept away from subnormals and overflow: magnitudes of about 2^-20 .. 2^20"""
    return scaled_normal(rng, (n, 1))[:, 0].astype(dt)


def fns(dt, n, h, rng=None):
    f = fn_arrays(dt, n, n + 3, h, rng)
    f["h"][n:] = 9999
    return f


def cheap_prox(f, n, v, rho):
    """dev::ProxEvalCheap / dev::ProxEval on the twelve cheap functions, operation by operation in the working dtype"""
    T = v.dtype.type
    h, a, b, c, d, e = (f[k][:n] for k in "habcde")
    one, zero = T(1), T(0)
    with np.errstate(all="ignore"):
        v = a * (v * rho - d) / (e + rho) - b
        rho = (e + rho) / (c * a * a)
        ir = one / rho
        table = {
            0: np.maximum(zero, v - ir) - np.maximum(zero, -(v + ir)),
            2: np.where(np.abs(v) < one + ir, v * rho / (one + rho), v - np.where(v >= 0, ir, -ir)),
            3: v - ir,
            4: np.where(v <= 0, zero, np.where(v >= 1, one, v)),
            5: np.zeros_like(v),
            6: np.where(v <= 0, zero, v),
            7: np.where(v >= 0, zero, v),
            9: np.where(v + ir <= 0, v + ir, np.where(v >= 0, v, zero)),
            10: np.where(v >= ir, v - ir, np.where(v <= 0, v, zero)),
            12: (v + np.sqrt(v * v + T(4) / rho)) / T(2),
            14: rho * v / (one + rho),
            15: v,
        }
        r = np.empty_like(v)
        for code, val in table.items():
            r[h == code] = val[h == code]
        return ((r + b) / a).astype(T)


def pre_tail(is_x, prev, zt, z12, zs, alpha):
    """admm_pre_kernel around the prox, operation by operation in the working dtype: v, w, ztemp, aux"""
    T = prev.dtype.type
    zsv = T(zs) * zt
    v = prev - zsv
    w = v - z12
    ztn = (zsv + T(alpha) * z12) + (T(1) - T(alpha)) * prev
    aux = prev - ztn if is_x else ztn - prev
    return v, w, ztn, aux


def records(terms, chunk):
    """per-workgroup sums of `terms` (long double, [n][k]) and of their magnitudes: [blocks][k]"""
    n = terms.shape[0]
    blocks = (n + chunk - 1) // chunk
    s = np.zeros((blocks, terms.shape[1]), np.longdouble)
    m = np.zeros_like(s)
    for b in range(blocks):
        s[b] = terms[b * chunk:(b + 1) * chunk].sum(axis=0)
        m[b] = np.abs(terms[b * chunk:(b + 1) * chunk]).sum(axis=0)
    return s, m


def pre_terms(w, h):
    w, h = np.asarray(w, np.longdouble), np.asarray(h, np.longdouble)
    return np.stack([w * h, w * w, h * h], axis=1)


def pre_case(rng, dt, nx, ny, data, hs_x=None, hs_y=None):
    if data == "int":
        mk = lambda n: ints(rng, n, dt)
        g = fns(dt, nx, rng.choice(EXACT_FNS, nx) if hs_x is None else hs_x)
        f = fns(dt, ny, rng.choice(EXACT_FNS, ny) if hs_y is None else hs_y)
    else:
        mk = lambda n: scaled(rng, n, dt)
        g = fns(dt, nx, rng.choice(CHEAP_FNS, nx) if hs_x is None else hs_x, rng)
        f = fns(dt, ny, rng.choice(CHEAP_FNS, ny) if hs_y is None else hs_y, rng)
    vec = dict(x_cur=mk(nx), xt=mk(nx), y_cur=mk(ny), yt=mk(ny))
    return g, f, vec


def run_pre(dt, nx, ny, g, f, vec, rho, alpha, zs, cheap, aux=True, cg=None, **kw):
    bx, by = (nx + PRE_CHUNK - 1) // PRE_CHUNK, (ny + PRE_CHUNK - 1) // PRE_CHUNK
    out = P.vec_check(P.VEC_ADMM_PRE, dt, n_x=nx, n_y=ny, g=g, f=f,
                      x_in=[inp(dt, nx, vec["x_cur"]), inp(dt, nx, vec["xt"])],
                      y_in=[inp(dt, ny, vec["y_cur"]), inp(dt, ny, vec["yt"])],
                      x_out=[outp(dt, nx), outp(dt, nx), outp(dt, nx) if aux else None],
                      y_out=[outp(dt, ny), outp(dt, ny), outp(dt, ny) if aux else None],
                      rho=rho, alpha=alpha, zs=zs, cheap=cheap, partials=np.zeros((bx + by) * 3 + 3),
                      scalars=np.full(P.VEC_SCALARS, SENT), cg=cg, **kw)
    assert out["info"][:2] == [bx, by]
    for side, n in (("x_out", nx), ("y_out", ny)):
        for k, arr in enumerate(out[side]):
            assert arr is None or kept(arr, n), (side, k)
    assert np.all(np.isnan(out["partials"][(bx + by) * 3:]))          # no record beyond the grid
    S = out["scalars"]
    untouched = np.ones(P.VEC_SCALARS, bool)
    untouched[P.SLOT_GAP_X:P.SLOT_GAP_X + 3] = untouched[P.SLOT_GAP_Y:P.SLOT_GAP_Y + 3] = False
    assert np.all(S[untouched] == SENT)
    res = dict(x12=out["x_out"][0][:nx], xtemp=out["x_out"][1][:nx], y12=out["y_out"][0][:ny], ytemp=out["y_out"][1][:ny],
               part_x=out["partials"][:bx * 3].reshape(bx, 3), part_y=out["partials"][bx * 3:(bx + by) * 3].reshape(by, 3),
               sum_x=S[P.SLOT_GAP_X:P.SLOT_GAP_X + 3], sum_y=S[P.SLOT_GAP_Y:P.SLOT_GAP_Y + 3], cg=out["cg"], info=out["info"])
    if aux:
        res.update(x_aux=out["x_out"][2][:nx], y_aux=out["y_out"][2][:ny])
    return res


PRE_OUTPUTS = ("x12", "xtemp", "y12", "ytemp", "part_x", "part_y", "sum_x", "sum_y", "x_aux", "y_aux")


def same_result(a, b):
    return all(same_bytes(a[k], b[k]) for k in PRE_OUTPUTS if k in a or k in b)


# --------------------------------------------------------------------------------------------- admm_pre
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nx,ny", PRE_SIZES)
def test_admm_pre_exact_integers(dt, nx, ny):
    rng = np.random.default_rng(nx * 7 + ny)
    g, f, vec = pre_case(rng, dt, nx, ny, "int")
    for k, (rho, zs, alpha) in enumerate([(2.0, 0.5, 1.5), (0.5, 2.0, 1.0), (1.0, 1.0, 1.5)]):
        aux = k != 1
        cg = np.array([3.0, 4.0]) if k == 0 else None
        res = [run_pre(dt, nx, ny, g, f, vec, rho, alpha, zs, cheap, aux=aux, cg=cg) for cheap in (1, 0)]
        assert same_result(res[0], res[1])
        r = res[0]
        if cg is not None:
            assert np.array_equal(r["cg"], [0.0, 0.0])
        for is_x, n, fn, pv, zt, s in ((True, nx, g, "x_cur", "xt", "x"), (False, ny, f, "y_cur", "yt", "y")):
            prev, ztv = vec[pv].astype(np.float64), vec[zt].astype(np.float64)
            v = prev - zs * ztv
            h = prox_exact(fn["h"][:n], v, rho)
            _, w, ztn, auxv = pre_tail(is_x, prev, ztv, h, zs, alpha)
            assert np.array_equal(r[s + "12"], h.astype(dt)), s
            assert np.array_equal(r[s + "temp"], ztn.astype(dt)), s
            if aux:
                assert np.array_equal(r[s + "_aux"], auxv.astype(dt)), s
            rec, mag = records(pre_terms(w, h), PRE_CHUNK)
            assert float(mag.sum()) * 64 < 2.0 ** 53           # multiples of 1/64: every partial sum is exact in fp64
            assert np.array_equal(r["part_" + s], rec.astype(np.float64)), s
            assert np.array_equal(r["sum_" + s], rec.sum(axis=0).astype(np.float64)), s


def check_pre_sums(dt, r, vec, zs, alpha, nx, ny, z12_ref=None, what="pre"):
    """element-wise outputs from the device's own z12, bit for bit; records and totals within their gamma bounds"""
    for is_x, n, pv, zt, s in ((True, nx, "x_cur", "xt", "x"), (False, ny, "y_cur", "yt", "y")):
        z12 = r[s + "12"]
        assert np.all(np.isfinite(z12)), s
        if z12_ref is not None:
            assert same_bytes(z12, z12_ref[s]), (what, s, "z12")
        _, w, ztn, auxv = pre_tail(is_x, vec[pv], vec[zt], z12, zs, alpha)
        assert same_bytes(r[s + "temp"], ztn), (what, s, "ztemp")
        if s + "_aux" in r:
            assert same_bytes(r[s + "_aux"], auxv), (what, s, "aux")
        terms = pre_terms(w, z12)
        rec, mag = records(terms, PRE_CHUNK)
        bounded(what + " record", dt, r["part_" + s], rec, gamma(32, np.float64) * mag)
        nparts = rec.shape[0]
        bounded(what + " total", dt, r["sum_" + s], terms.sum(axis=0), gamma(nparts + 32, np.float64) * np.abs(terms).sum(axis=0))
        # the total is the sum of the device's own records too (the job's slots and offsets)
        bounded(what + " total of records", dt, r["sum_" + s], r["part_" + s].astype(np.longdouble).sum(axis=0),
                gamma(nparts + 32, np.float64) * np.abs(r["part_" + s]).sum(axis=0))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nx,ny", PRE_SIZES)
def test_admm_pre_real_data_cheap_functions(dt, nx, ny):
    rng = np.random.default_rng(nx * 11 + ny)
    g, f, vec = pre_case(rng, dt, nx, ny, "real")
    rho, zs, alpha = dt(rng.uniform(0.3, 3.0)), dt(rng.uniform(0.3, 2.0)), dt(1.0 + rng.uniform(0.2, 0.8))
    res = [run_pre(dt, nx, ny, g, f, vec, rho, alpha, zs, cheap) for cheap in (1, 0)]
    assert same_result(res[0], res[1])
    ref = {}
    for n, fn, pv, zt, s in ((nx, g, "x_cur", "xt", "x"), (ny, f, "y_cur", "yt", "y")):
        v = vec[pv] - zs * vec[zt]
        assert v.dtype == dt
        ref[s] = cheap_prox(fn, n, v, rho)
    check_pre_sums(dt, res[0], vec, zs, alpha, nx, ny, ref, "pre cheap")


@pytest.mark.parametrize("dt", DTYPES)
def test_admm_pre_with_the_expensive_functions(dt):
    """cheap = 0 with all 16 functions: z12 is PogsAmdProxEval at the reproduced v, bit for bit"""
    nx, ny = 1025, 257
    rng = np.random.default_rng(5)
    g, f, _ = pre_case(rng, dt, nx, ny, "real", rng.integers(0, 16, nx), rng.integers(0, 16, ny))
    mk = lambda n: (rng.normal(0, 3.0, n) * np.exp2(rng.uniform(-3, 3, n))).astype(dt)
    vec = dict(x_cur=mk(nx), xt=mk(nx), y_cur=mk(ny), yt=mk(ny))
    rho, zs, alpha = dt(1.7), dt(0.8), dt(1.5)
    r = run_pre(dt, nx, ny, g, f, vec, rho, alpha, zs, 0)
    ref = {}
    for n, fn, pv, zt, s in ((nx, g, "x_cur", "xt", "x"), (ny, f, "y_cur", "yt", "y")):
        v = vec[pv] - zs * vec[zt]
        fv = pogs_amd.FunctionVector(n, *(fn[k][:n] for k in "habcde"))
        ref[s] = pogs_amd.prox_eval(fv, float(rho), v, dtype=dt)
        cheap = np.isin(fn["h"][:n], CHEAP_FNS)
        assert same_bytes(ref[s][cheap], cheap_prox(fn, n, v, rho)[cheap])      # the full library on the cheap functions
    check_pre_sums(dt, r, vec, zs, alpha, nx, ny, ref, "pre mixed")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cheap", [1, 0])
def test_admm_pre_uniform_coefficients(dt, cheap):
    """all 16 masks: an array declared uniform holds NaN (9999 for h) and is not read"""
    nx, ny = 1025, 257
    rng = np.random.default_rng(17)
    uni = dict(h=2, c=dt(1.75), d=dt(-0.375), e=dt(0.625))     # kHuber: a reader of the poisoned h takes the default branch
    rho, zs, alpha = dt(1.3), dt(0.7), dt(1.5)
    g, f, vec = pre_case(rng, dt, nx, ny, "real")
    for mask in range(16):
        mg, mf = mask, (mask * 7 + 5) % 16
        full, poisoned = [], []
        for fn, n, m in ((g, nx, mg), (f, ny, mf)):
            a, b = {k: v.copy() for k, v in fn.items()}, {k: v.copy() for k, v in fn.items()}
            for bit, k in enumerate("hcde"):
                if m >> bit & 1:
                    a[k][:n] = uni[k]
                    b[k][:] = 9999 if k == "h" else np.nan
            full.append(a)
            poisoned.append(b)
        u = lambda m: (m, uni["h"], uni["c"], uni["d"], uni["e"])
        want = run_pre(dt, nx, ny, full[0], full[1], vec, rho, alpha, zs, cheap)
        got = run_pre(dt, nx, ny, poisoned[0], poisoned[1], vec, rho, alpha, zs, cheap, ug=u(mg), uf=u(mf))
        assert got["info"][2:] == [mg, mf]
        assert np.all(np.isfinite(want["x12"])) and np.all(np.isfinite(want["y12"]))
        assert same_result(got, want), mask
        # the probe finds the same masks on the full arrays (at least: a random array may be uniform by accident at n = 1)
        probed = run_pre(dt, nx, ny, full[0], full[1], vec, rho, alpha, zs, cheap, probe=1)
        assert probed["info"][2:] == [mg, mf]
        assert same_result(probed, want), mask


# --------------------------------------------------------------------------------------------- probe_uniform
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 256, 257, 524288 + 300])
def test_probe_uniform(dt, n):
    base = dict(h=np.full(n + 3, 9999, np.int32), a=np.full(n + 3, np.nan, dt), b=np.full(n + 3, np.nan, dt),
                c=np.full(n + 3, np.nan, dt), d=np.full(n + 3, np.nan, dt), e=np.full(n + 3, np.nan, dt))
    base["h"][:n], base["c"][:n], base["d"][:n], base["e"][:n] = 12, 1.5, -0.25, 0.75

    def probe(g):
        out = P.vec_check(P.VEC_PROBE_UNIFORM, dt, n_x=n, g=g)
        return out["info"][0], out["info"][1], out["scalars"][:3]

    mask, h, cde = probe(base)
    assert (mask, h) == (15, 12) and np.array_equal(cde, [1.5, -0.25, 0.75])     # the NaN tail is not read
    other = dict(h=3, c=1.25, d=0.5, e=0.0)
    for idx in sorted({i for i in (1, n - 1, 524288) if 0 < i < n}):
        for which in ("h", "c", "d", "e", "hcde"):
            g = {k: v.copy() for k, v in base.items()}
            for k in which:
                g[k][idx] = other[k]
            mask, h, cde = probe(g)
            assert mask == 15 - sum(1 << "hcde".index(k) for k in which), (idx, which)
            assert h == 12 and np.array_equal(cde, [1.5, -0.25, 0.75])          # the values are element 0's
    if n > 1:
        g = {k: v.copy() for k, v in base.items()}
        g["c"][n - 1] = np.nan
        assert probe(g)[0] == 15 - 2
        g["c"][:n] = np.nan                       # the same NaN everywhere still differs from itself
        assert probe(g)[0] == 15 - 2
        # d = {0.0, -0.0} is reported uniform with the value of element 0: -0.0 == 0.0.  The prox can then differ only in the
        # sign of a zero: d enters it as v * rho - d alone, where the two zeros give the same sum unless v * rho is a zero
        for first, rest in ((0.0, -0.0), (-0.0, 0.0)):
            g = {k: v.copy() for k, v in base.items()}
            g["d"][:n] = rest
            g["d"][0] = first
            mask, h, cde = probe(g)
            assert mask == 15 and cde[1] == 0 and np.signbit(cde[1]) == np.signbit(first)


# --------------------------------------------------------------------------------------------- the 256-per-block kernels
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", VEC_SIZES)
def test_scale_objective(dt, n):
    rng = np.random.default_rng(n)
    for divide in (1, 0):
        g = fns(dt, n, rng.integers(0, 16, n), rng)
        g["c"][:n:3] *= -1                      # negative c and e are clamped to 0
        g["e"][:n] -= dt(0.3)
        if n > 4:
            g["c"][4], g["e"][3], g["a"][2], g["d"][1] = np.nan, np.nan, np.nan, np.nan      # NaN passes through
        s = scaled(rng, n, dt)
        out = P.vec_check(P.VEC_SCALE_OBJECTIVE, dt, n_x=n, g=g, x_in=[inp(dt, n, s)], x_out=[outp(dt, n)] * 4, mode=divide)
        a, c, d, e = out["x_out"]
        assert all(kept(v, n) for v in (a, c, d, e))
        ga, gc, gd, ge = (g[k][:n] for k in "acde")
        with np.errstate(invalid="ignore"):
            wc, we = np.where(gc < 0, dt(0), gc), np.where(ge < 0, dt(0), ge)
        ss = s * s                               # e is scaled by s * s, the product rounded first
        wa, wd, we = (ga / s, gd / s, we / ss) if divide else (ga * s, gd * s, we * ss)
        for got, want, k in ((a, wa, "a"), (c, wc, "c"), (d, wd, "d"), (e, we, "e")):
            assert want.dtype == dt and same_bytes(np.isnan(got[:n]), np.isnan(want)), k
            ok = ~np.isnan(want)
            assert same_bytes(got[:n][ok], want[ok]), k
        if n > 4:
            assert np.isnan(c[4]) and np.isnan(e[3]) and np.isnan(a[2]) and np.isnan(d[1])
            assert np.all(c[:n][np.arange(n) != 4] >= 0) and np.all(e[:n][np.arange(n) != 3] >= 0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", VEC_SIZES)
def test_unscale(dt, n):
    """x = x12 e, y = y12 / d, mu = -rho (zs xt - xprev + x12) / e, l = -rho (zs yt - yprev + y12) d (pogs.cpp:510-518)"""
    rng = np.random.default_rng(n + 1)
    ny = {1: 257, 255: 1, 256: 256, 257: 1000, 1000: 255}[n]        # the y blocks start at a non-zero block
    rho, zs = dt(1.9), dt(0.6)
    for data in ("int", "real"):
        mk = (lambda k: ints(rng, k, dt)) if data == "int" else (lambda k: scaled(rng, k, dt))
        x12, xt, xprev, y12, yt, yprev = mk(n), mk(n), mk(n), mk(ny), mk(ny), mk(ny)
        e, d = np.exp2(rng.integers(-3, 4, n)).astype(dt), np.exp2(rng.integers(-3, 4, ny)).astype(dt)
        if data == "real":
            e, d = e * rng.uniform(1, 2, n).astype(dt), d * rng.uniform(1, 2, ny).astype(dt)
        for with_mu in (True, False):
            out = P.vec_check(P.VEC_UNSCALE, dt, n_x=n, n_y=ny, rho=rho, zs=zs,
                              x_in=[inp(dt, n, v) for v in (x12, xt, xprev, e)], y_in=[inp(dt, ny, v) for v in (y12, yt, yprev, d)],
                              x_out=[outp(dt, n), outp(dt, n) if with_mu else None], y_out=[outp(dt, ny), outp(dt, ny)])
            xo, mu = out["x_out"]
            yo, lo = out["y_out"]
            assert kept(xo, n) and kept(yo, ny) and kept(lo, ny)
            assert same_bytes(xo[:n], x12 * e) and same_bytes(yo[:ny], y12 / d)
            assert same_bytes(lo[:ny], (-rho) * ((zs * yt - yprev) + y12) * d)
            if with_mu:
                assert kept(mu, n) and same_bytes(mu[:n], (-rho) * ((zs * xt - xprev) + x12) / e)
            else:
                assert mu is None                 # (nothing to write through: the launch got a null pointer and did not fault)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", VEC_SIZES)
def test_admm_tail(dt, n):
    rng = np.random.default_rng(n + 2)
    blocks = (n + VEC_CHUNK - 1) // VEC_CHUNK
    for data in ("int", "real"):
        mk = (lambda: ints(rng, n, dt)) if data == "int" else (lambda: scaled(rng, n, dt))
        znew, zprev, z12, ztemp = mk(), mk(), mk(), mk()
        zt_in = outp(dt, n)
        zt_in[:n] = ztemp
        out = P.vec_check(P.VEC_ADMM_TAIL, dt, n_x=n, x_in=[inp(dt, n, v) for v in (znew, zprev, z12)], x_out=[zt_in],
                          partials=np.zeros(blocks * 2 + 3), scalars=np.full(P.VEC_SCALARS, SENT))
        assert out["info"][0] == blocks and kept(out["x_out"][0], n)
        assert same_bytes(out["x_out"][0][:n], ztemp - znew)
        part = out["partials"]
        assert np.all(np.isnan(part[blocks * 2:]))
        S = out["scalars"]
        assert np.all(np.delete(S, [P.SLOT_DXPREV2, P.SLOT_DXPREV2 + 1]) == SENT)
        p, q = np.asarray(zprev - znew, np.longdouble), np.asarray(z12 - znew, np.longdouble)
        terms = np.stack([p * p, q * q], axis=1)
        rec, mag = records(terms, VEC_CHUNK)
        got_rec, got_sum = part[:blocks * 2].reshape(blocks, 2), S[P.SLOT_DXPREV2:P.SLOT_DXPREV2 + 2]
        if data == "int":
            assert np.array_equal(got_rec, rec.astype(np.float64)) and np.array_equal(got_sum, rec.sum(axis=0).astype(np.float64))
        else:
            bounded("tail record", dt, got_rec, rec, gamma(32, np.float64) * mag)
            bounded("tail total", dt, got_sum, terms.sum(axis=0), gamma(blocks + 32, np.float64) * mag.sum(axis=0))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", VEC_SIZES)
def test_blas1_helpers(dt, n):
    """exact_u, scale_by (both directions), axpby (b == 0 and b != 0), scal, sqrt, fill"""
    rng = np.random.default_rng(n + 3)
    one = lambda op, **kw: P.vec_check(op, dt, n_x=n, **kw)["x_out"][0]
    for data in ("int", "real"):
        mk = (lambda: ints(rng, n, dt)) if data == "int" else (lambda: scaled(rng, n, dt))
        x, y, z = mk(), mk(), mk()
        c, a, b = (dt(0.5), dt(2.0), dt(-4.0)) if data == "int" else (dt(0.37), dt(-1.3), dt(2.9))
        nz = np.where(y == 0, dt(1), y)
        ytail = outp(dt, n)
        ytail[:n] = y
        checks = [
            ("exact_u", one(P.VEC_EXACT_U, x_in=[inp(dt, n, v) for v in (x, y, z)], s0=c, x_out=[outp(dt, n)]), (x + c * y) - z),
            ("scale_by /", one(P.VEC_SCALE_BY, x_in=[inp(dt, n, x), inp(dt, n, nz)], s0=a, mode=1, x_out=[outp(dt, n)]), a * x / nz),
            ("scale_by *", one(P.VEC_SCALE_BY, x_in=[inp(dt, n, x), inp(dt, n, y)], s0=a, mode=0, x_out=[outp(dt, n)]), a * x * y),
            ("axpby", one(P.VEC_AXPBY, x_in=[inp(dt, n, x)], s0=a, s1=b, x_out=[ytail]), a * x + b * y),
            # b == 0: y is not read (NaN there would otherwise come through 0 * NaN)
            ("axpby b=0", one(P.VEC_AXPBY, x_in=[inp(dt, n, x)], s0=a, s1=0.0, x_out=[np.where(np.arange(n + 3) < n, np.nan, SENT).astype(dt)]), a * x),
            ("scal", one(P.VEC_SCAL, s0=a, x_out=[ytail]), y * a),
            ("sqrt", one(P.VEC_SQRT, x_out=[np.abs(ytail)]), np.sqrt(np.abs(y))),
            ("fill", one(P.VEC_FILL, s0=c, x_out=[outp(dt, n)]), np.full(n, c, dt)),
        ]
        for what, got, want in checks:
            assert want.dtype == dt, what
            if what == "sqrt":
                assert got.size == n + 3 and np.all(got[n:] == np.abs(np.asarray(SENT, dt))), what
            else:
                assert kept(got, n), what
            assert same_bytes(got[:n], want), (what, data)


# --------------------------------------------------------------------------------------------- the scalar sums
def sum_jobs_case(rng, nparts, combos, data):
    """jobs with their own records and slots in one partials array that is NaN wherever no job reads"""
    jobs, first, slot, want, absw = [], 1, 1, {}, {}
    chunks = []
    for ns, stride, offset in combos:
        st = stride if stride > 0 else ns
        length = offset + (nparts - 1) * st + ns
        p = np.full(length, np.nan)
        idx = offset + np.arange(nparts)[:, None] * st + np.arange(ns)[None, :]
        vals = rng.integers(-2 ** 20, 2 ** 20, (nparts, ns)).astype(np.float64) if data == "int" else \
            scaled_normal(rng, (nparts, ns))
        p[idx] = vals
        chunks.append((first, p))
        jobs.append([first, nparts, ns, stride, offset, slot])
        want[slot] = np.asarray(p[idx], np.longdouble).sum(axis=0)
        absw[slot] = np.abs(p[idx]).sum(axis=0)
        first += length + 1
        slot += ns + 1
    assert slot <= P.VEC_SCALARS
    partials = np.full(first + 2, np.nan)
    for at, p in chunks:
        partials[at:at + p.size] = p
    return jobs, partials, want, absw


@pytest.mark.parametrize("nparts", SUM_NPARTS)
def test_sum_jobs(nparts):
    rng = np.random.default_rng(nparts)
    combos = [(ns, stride, offset) for ns in (1, 2, 3, 6) for stride in (0, ns, ns + 3) for offset in (0, 2)]
    groups = [combos[0:8], combos[8:16], combos[16:24], combos[5:6], combos[22:24], combos[11:12], combos[2:4]]
    assert sorted(len(g) for g in groups) == [1, 1, 2, 2, 8, 8, 8]
    for data in ("int", "real"):
        for group in groups:
            jobs, partials, want, absw = sum_jobs_case(rng, nparts, group, data)
            S = P.vec_check(P.VEC_SUM_JOBS, np.float64, partials=partials, jobs=jobs, scalars=np.full(P.VEC_SCALARS, SENT))["scalars"]
            written = np.zeros(P.VEC_SCALARS, bool)
            for job in jobs:
                ns, slot = job[2], job[5]
                written[slot:slot + ns] = True
                if data == "int":
                    assert float(np.max(absw[slot])) < 2.0 ** 53           # every partial total is exact in fp64
                    assert np.array_equal(S[slot:slot + ns], want[slot].astype(np.float64)), job
                else:
                    bounded("sum_jobs total", np.float64, S[slot:slot + ns], want[slot], gamma(nparts + 32, np.float64) * absw[slot])
            assert np.all(S[~written] == SENT)


@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 1000])
def test_max_partials(n):
    rng = np.random.default_rng(n)
    for at in sorted({0, n // 2, n - 1}):
        p = rng.uniform(0.0, 1.0, n)
        p[at] = 2.5
        S = P.vec_check(P.VEC_MAX_PARTIALS, np.float64, partials=p, scalars=np.full(P.VEC_SCALARS, SENT))["scalars"]
        assert S[0] == 2.5 and np.all(S[1:] == SENT)
    S = P.vec_check(P.VEC_MAX_PARTIALS, np.float64, partials=np.full(n, -1.0), scalars=np.full(P.VEC_SCALARS, SENT))["scalars"]
    assert S[0] == 0.0            # the maximum starts from 0: the partials are magnitudes


def test_sum_cg():
    """the three CGLS scalars formed in the launch that sums their last partials; all exact in fp64"""
    rng = np.random.default_rng(3)
    nparts = 300
    parts = rng.integers(-8, 9, nparts).astype(np.float64)
    total = float(parts.sum())
    eps = 2.0 ** -40

    def run(mode, slot, S, cg, shift=0.0, adjust=0.0):
        p = parts.copy()
        p[7] += adjust
        out = P.vec_check(P.VEC_SUM_CG, np.float64, partials=np.concatenate([[np.nan], p, [np.nan]]), mode=mode,
                          jobs=[[1, nparts, 1, 0, 0, slot]], scalars=S, cg=cg, s0=shift, s1=eps)
        changed = np.flatnonzero(~((out["scalars"] == S) | (np.isnan(S) & np.isnan(out["scalars"]))))
        assert set(changed) <= {slot}
        return out["scalars"], out["cg"]

    S0 = np.full(P.VEC_SCALARS, SENT)
    S0[P.SLOT_CG_P2] = 3.0
    cg0 = np.array([6.0, SENT, SENT, SENT, SENT])
    # mode 1: delta = q2 + shift p2 > 0: alpha = gamma / delta, the flag is left alone
    S, cg = run(1, P.SLOT_CG_Q2, S0, cg0, shift=0.5, adjust=40.0 - total)
    assert S[P.SLOT_CG_Q2] == 40.0 and np.array_equal(cg, [6.0, 6.0 / 41.5, SENT, 41.5, SENT])
    # delta < 0 raises the indefinite flag and is kept
    S, cg = run(1, P.SLOT_CG_Q2, S0, cg0, shift=0.5, adjust=-40.0 - total)
    assert S[P.SLOT_CG_Q2] == -40.0 and np.array_equal(cg, [6.0, 6.0 / -38.5, SENT, -38.5, 1.0])
    # delta == 0 raises it too and becomes eps
    S, cg = run(1, P.SLOT_CG_Q2, S0, cg0, shift=0.5, adjust=-1.5 - total)
    assert S[P.SLOT_CG_Q2] == -1.5 and np.array_equal(cg, [6.0, 6.0 / eps, SENT, eps, 1.0])
    # mode 2: beta = s2 / the old gamma, gamma = s2
    S, cg = run(2, P.SLOT_CG_S2, S0, cg0, adjust=21.0 - total)
    assert S[P.SLOT_CG_S2] == 21.0 and np.array_equal(cg, [21.0, SENT, 21.0 / 6.0, SENT, SENT])
    # mode 3: gamma = s2, the flag is cleared
    S, cg = run(3, P.SLOT_CG_S2, S0, np.array([6.0, SENT, SENT, SENT, 1.0]), adjust=21.0 - total)
    assert S[P.SLOT_CG_S2] == 21.0 and np.array_equal(cg, [21.0, SENT, SENT, SENT, 0.0])


# --------------------------------------------------------------------------------------------- the publish path
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("overlay", [((3, 30), (2, 3)), ((20, 0), (4, 0)), None])
@pytest.mark.parametrize("counts", [(3, 2), (0, 2), (3, 0), (8, 1)])
def test_publish_path(mode, overlay, counts):
    """queue_sum + set_overlay + fetch_scalars, twice: pending jobs go through sum_publish_kernel, none through
    publish_scalars_kernel; mode 1 is the copying path (launch_apply_overlay, then a copy).  A counter that
    sum_publish_kernel left non-zero would keep the second launch from publishing: wait_publish then copies and clears
    poll_fetch, so poll_fetch == 1 after both fetches is the assertion that finds it."""
    rng = np.random.default_rng(counts[0] * 16 + counts[1])
    slots = [12, 0, 15, 40, 44, 36, 9, 48]                # disjoint from the overlay ranges; ns <= 3
    S0 = 1000.0 + np.arange(P.VEC_SCALARS)
    partials = np.full(4000, np.nan)
    at = [1]

    def make(count, base):
        jobs, want = [], {}
        for k in range(count):
            ns, nparts = 1 + (k + base) % 3, 5 + 260 * ((k + base) % 2)
            vals = rng.integers(-1000, 1000, (nparts, ns)).astype(np.float64)
            partials[at[0]:at[0] + vals.size] = vals.ravel()
            jobs.append([at[0], nparts, ns, 0, 0, slots[(k + base) % 8]])
            want[slots[(k + base) % 8]] = vals.sum(axis=0)
            at[0] += vals.size + 1
        return jobs, want

    jobs1, want1 = make(counts[0], 0)
    jobs2, want2 = make(counts[1], 3)
    ov = None
    src = np.zeros(0)
    if overlay is not None:
        src = -1.0 - np.arange(sum(overlay[1]), dtype=np.float64)
        ov = (src, overlay[0], overlay[1])
    out = P.vec_check(P.VEC_PUBLISH, np.float64, partials=partials, jobs=jobs1 or None, jobs2=jobs2 or None, scalars=S0,
                      overlay=ov, mode=mode)
    exp1 = S0[:P.NUM_SLOTS].copy()
    for slot, v in want1.items():
        exp1[slot:slot + v.size] = v
    if overlay is not None:
        base = 0
        for q in range(2):                                 # src is read in the order of the ranges
            exp1[overlay[0][q]:overlay[0][q] + overlay[1][q]] = src[base:base + overlay[1][q]]
            base += overlay[1][q]
    exp2 = exp1.copy()                                     # overlaid slots were stored into the device block too
    for slot, v in want2.items():
        exp2[slot:slot + v.size] = v
    host1, dev1, host2, dev2 = out["pub"]
    for got, want, what in ((host1, exp1, "host 1"), (dev1, exp1, "device 1"), (host2, exp2, "host 2"), (dev2, exp2, "device 2")):
        assert np.array_equal(got[:P.NUM_SLOTS], want), what
        assert np.all(np.isnan(got[P.NUM_SLOTS:])), what
    assert out["info"][:2] == [0, 0]                       # the counter word after each fetch
    assert out["info"][2:] == ([1, 1] if mode == 0 else [0, 0])


def test_zz_report():
    """prints the largest error-to-bound ratio per check and dtype (profiles/vec_kernel_accuracy.txt is this table)"""
    for (what, dt), r in sorted(RATIOS.items()):
        print("RATIO %-34s %-8s %.3e" % (what, dt, r))
    assert all(r <= 1.0 for r in RATIOS.values())
