"""GPU tests of the dense streaming passes kernel by kernel (csrc/stream.h: stream_rows_kernel, stream_tri_kernel,
stream_rows2_kernel, stream_rows2_pf_kernel, xl_apply_rows_kernel, reduce_cols_kernel; csrc/fused_cols.h:
pre_cols_kernel, pack_cols_kernel) through PogsAmdDensePassCheck (include/pogs_amd.h, Part 3), which launches the
instantiations a dense solve launches.  ONE pass and its second stage on given arrays; no iteration is modelled.

Layout and poison: M has ldm = n_pad + 2 VEC with NaN in [n_pad, ldm); columns [n, n_pad) of M and of the dot vectors are
zero (the contract); every vector is three elements longer than it need be, inputs NaN there, outputs a sentinel that
must come back; the device's partial-sum buffers start as NaN (the entry does that), so a slot no workgroup wrote
poisons the total that reads it.  W_SWEEP: the entries right of the diagonal inside the diagonal's own 16-byte vector are
zero (that vector is loaded whole), every vector wholly right of the diagonal is NaN.

Three kinds of check (tests/test_gpu_batch_kernels.py):
  * exact integers: entries in [-4, 4]; rho, zs powers of two, alpha 1 or 1.5, a = c = 1, b = d = e = 0 and the functions
    kZero, kAbs, kIdentity, kIndBox01, kIndEq0, kIndGe0, kIndLe0, kMaxNeg0, kMaxPos0, so that every intermediate of
    FusedIterOp::row is a multiple of 1/8 the mantissa holds: every output equals the model for any summation order.
    Where a case's numbers could leave the mantissa (wide fp32 totals) the test asserts the precondition it relies on;
  * bounds on real, badly scaled data (scaled_normal): row dots within gamma_n (|M| |x|) of the hi() reference; what follows
    the dot in the functor has no free rounding (the unit is built with -ffp-contract=off) and is reproduced in numpy in
    the working dtype from the device's own ynew and y12s, bit for bit; y12s against the oracle's prox at that v with the
    tolerances of test_prox_library_matches_oracle; column totals within gamma_(rows+32) (|M|^T |u|) of M^T u with u built
    from the device's outputs; scalars within gamma_(rows+32) in fp64 of the long double sum of the device's vectors;
  * isolation: a row's outputs do not depend on the grid."""
import os

import numpy as np
import pytest

import oracle_binding as ob
from helpers import gamma, hi, ints, same_bytes, scaled_normal
from pogs_amd import _lib as P

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SENT = -7.375e-3
PLANS = [(64, 1), (64, 2), (64, 4), (256, 2), (256, 3), (256, 4), (256, 5), (256, 6), (256, 8), (256, 10),
         (512, 6), (512, 8), (512, 10), (1024, 6), (1024, 8)]
CAPS = sorted(t * v for t, v in PLANS)
EXACT_FNS = (15, 0, 3, 4, 5, 6, 7, 9, 10)         # kZero kAbs kIdentity kIndBox01 kIndEq0 kIndGe0 kIndLe0 kMaxNeg0 kMaxPos0
CHEAP_FNS = (0, 2, 3, 4, 5, 6, 7, 9, 10, 12, 14, 15)
LOGISTIC = 8
RATIOS = {}     # (what, dtype name) -> largest observed error / bound (printed by test_zz_report)


def vecw(dt):
    return 16 // np.dtype(dt).itemsize


def rup(v, a):
    return (v + a - 1) // a * a


def widths(dt, tpb, nv):
    """first natural width of the shape, a ragged one just below the last, the last"""
    V, cap = vecw(dt), tpb * nv
    prev = max([c for c in CAPS if c < cap], default=0)
    return [prev * V + 1, cap * V - 1, cap * V]


def note(what, dt, err, bar):
    ok = bar > 0
    r = float(np.max(np.where(ok, err / np.where(ok, bar, 1), np.where(err > 0, np.inf, 0)))) if np.size(err) else 0.0
    key = (what, np.dtype(dt).name)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    return r


def bounded(what, dt, got, ref, bar):
    """|got - ref| <= bar elementwise; the largest ratio is recorded"""
    assert np.all(np.isfinite(np.asarray(got, np.float64))), what
    err = np.abs(hi(np.asarray(got)) - ref) if np.asarray(got).dtype != np.longdouble else np.abs(got - ref)
    r = note(what, dt, np.asarray(err, np.float64), np.asarray(bar, np.float64))
    assert np.all(err <= bar), (what, r)


def make_M(rng, dt, rows, n, data):
    V = vecw(dt)
    n_pad = rup(n, V)
    M = np.full((rows, n_pad + 2 * V), np.nan, dt)
    M[:, :n] = ints(rng, (rows, n), dt) if data == "int" else scaled_normal(rng, (rows, n)).astype(dt)
    M[:, n:n_pad] = 0
    return M


def colv(dt, n, vals=None):
    """a column-side vector: values, zero padding to n_pad, NaN beyond (inputs) / sentinel everywhere (vals None)"""
    n_pad = rup(n, vecw(dt))
    if vals is None:
        return np.full(n_pad + 3, SENT, dt)
    x = np.full(n_pad + 3, np.nan, dt)
    x[:n], x[n:n_pad] = vals, 0
    return x


def rowv(dt, rows, vals=None):
    if vals is None:
        return np.full(rows + 3, SENT, dt)
    y = np.full(rows + 3, np.nan, dt)
    y[:rows] = vals
    return y


def fn_arrays(dt, count, length, h, rng=None):
    """function objects: the exact configuration (a = c = 1, b = d = e = 0), or random coefficients (rng)"""
    f = dict(h=np.full(length, 15, np.int32), a=np.full(length, np.nan, dt), b=np.full(length, np.nan, dt),
             c=np.full(length, np.nan, dt), d=np.full(length, np.nan, dt), e=np.full(length, np.nan, dt))
    f["h"][:count] = h
    if rng is None:
        f["a"][:count], f["b"][:count], f["c"][:count], f["d"][:count], f["e"][:count] = 1, 0, 1, 0, 0
    else:
        f["a"][:count] = rng.uniform(0.5, 2.0, count) * rng.choice([-1, 1], count)
        f["b"][:count] = rng.normal(0, 0.5, count)
        f["c"][:count] = rng.uniform(0.2, 3.0, count)
        f["d"][:count] = rng.normal(0, 0.3, count)
        f["e"][:count] = rng.uniform(0.0, 1.0, count)
    return f


def prox_exact(h, v, rho):
    """ProxEvalCheap in the exact configuration: v and 1 / rho are multiples of 1/8, every branch is exact"""
    ir = 1.0 / rho
    z = np.zeros_like(v)
    table = {
        15: v, 0: np.maximum(z, v - ir) - np.maximum(z, -(v + ir)), 3: v - ir,
        4: np.where(v <= 0, z, np.where(v >= 1, z + 1, v)), 5: z, 6: np.where(v <= 0, z, v), 7: np.where(v >= 0, z, v),
        9: np.where(v + ir <= 0, v + ir, np.where(v >= 0, v, z)), 10: np.where(v >= ir, v - ir, np.where(v <= 0, v, z)),
    }
    out = np.empty_like(v)
    for code, val in table.items():
        out[h == code] = val[h == code]
    return out


def prox_tols(dt, h):
    """the tolerances of test_prox_library_matches_oracle, per function code"""
    if dt == np.float64:
        return np.full(h.shape, 1e-9), np.full(h.shape, 1e-9)
    return np.where(np.isin(h, (1, 8, 11, 13)), 5e-4, 5e-5), np.where(h == 8, 5e-5, 1e-5)


def check_prox(what, dt, got, f, count, rho, v):
    objs = {k: f[k][:count] for k in "habcde"}
    want = ob.oracle_prox(objs, rho, v, dtype=dt)
    rtol, atol = prox_tols(dt, objs["h"])
    ok = np.isfinite(want)
    assert np.all(np.isfinite(got) == ok), what
    bounded(what, dt, got[ok], hi(want[ok]), (atol + rtol * np.abs(want))[ok])


def fused_tail(yn, h, ytemp_in, zs, alpha, xside):
    """FusedIterOp::row after the dot, operation by operation in the working dtype"""
    T = yn.dtype.type
    ztn = ytemp_in - yn
    zts = T(zs) * ztn
    v = yn - zts
    yh = (zts + T(alpha) * h) + (T(1) - T(alpha)) * yn
    u1 = h if xside else (h + zts) - yn
    return ztn, zts, v, yh, u1


def sum_check(what, got, terms_a, terms_b, count):
    """an fp64 fma sum of exact products of working-precision values, any grouping: within gamma_(count+32) of the long
    double sum"""
    a, b = np.asarray(terms_a, np.longdouble), np.asarray(terms_b, np.longdouble)
    ref, absref = np.sum(a * b), np.sum(np.abs(a * b))
    bounded(what, np.float64, np.asarray([np.longdouble(got)]), np.asarray([ref]),
            np.asarray([gamma(count + 32, np.float64) * absref]))


def exact_fits(dt, absref, quantum=0.125):
    """every partial sum of terms that are multiples of `quantum` with this sum of magnitudes is held exactly (integers
    up to 2^(mantissa bits + 1) are)"""
    return float(np.max(absref)) / quantum <= 2.0 ** (np.finfo(dt).nmant + 1)


def check_totals(what, dt, M, n, rows, got, u, exact, quantum=0.125):
    """got[:n] = M^T u: bit for bit on integers (asserting that they fit the mantissa in any order of summation),
    gamma-bounded otherwise; padding zero, tail kept"""
    n_pad = rup(n, vecw(dt))
    Mh, uh = hi(M[:rows, :n]), hi(np.asarray(u))
    ref, absref = Mh.T @ uh, np.abs(Mh).T @ np.abs(uh)
    if exact:
        assert exact_fits(dt, absref, quantum), (what, "the integers of this case leave the mantissa")
        assert np.array_equal(got[:n], ref.astype(dt)), what
    else:
        bounded(what, dt, got[:n], ref, gamma(rows + 32, dt) * absref)
    assert np.all(got[n:n_pad] == 0) and np.all(got[n_pad:] == np.asarray(SENT, dt)), what


def iter_case(rng, dt, rows, n, data, functor, hs=None):
    """inputs of one ITER_* / PRE_ACC pass"""
    M = make_M(rng, dt, rows, n, data)
    if data == "int":
        x0, x1 = ints(rng, n, dt), ints(rng, n, dt)
        ycur, y12, yt, ytemp = (ints(rng, rows, dt) for _ in range(4))
        hcodes = rng.choice(EXACT_FNS, rows) if hs is None else hs
        f = fn_arrays(dt, rows, rows + 3, hcodes)
    else:
        x0, x1 = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
        ycur, y12, yt, ytemp = (rng.normal(0, 3.0, rows).astype(dt) for _ in range(4))
        hcodes = rng.choice(CHEAP_FNS, rows) if hs is None else hs
        f = fn_arrays(dt, rows, rows + 3, hcodes, rng)
    vec = dict(x0=colv(dt, n, x0), x1=colv(dt, n, x1), ycur=rowv(dt, rows, ycur), y12=rowv(dt, rows, y12),
               yt=rowv(dt, rows, yt), ytemp=rowv(dt, rows, ytemp), ynew=rowv(dt, rows), y12s=rowv(dt, rows),
               ytemps=rowv(dt, rows), tot0=colv(dt, n), tot1=colv(dt, n))
    return M, vec, f


def check_iter(tag, dt, M, n, rows, vec, f, out, functor, lean, rho, alpha, zs, c_old, exact):
    """every output of an ITER_FULL / ITER_LEAN pass with REDUCE as the second stage"""
    xside, logistic = functor == P.PASS_FN_XSIDE, functor == P.PASS_FN_LOGISTIC
    u = np.finfo(dt).eps / 2
    Mh = hi(M[:rows, :n])
    x0, x1 = vec["x0"][:n], vec["x1"][:n]
    ycur, y12, yt, ytemp_in = (vec[k][:rows] for k in ("ycur", "y12", "yt", "ytemp"))
    yn, h = out["ynew"][:rows], out["y12s"][:rows]
    for k in ("ynew", "y12s", "ytemps"):
        assert np.all(out[k][rows:] == np.asarray(SENT, dt)), (tag, k)
    assert np.all(np.isnan(out["ytemp"][rows:])), tag        # in / out: its tail is the input's
    quantum = 1.0 if (rho, zs, alpha) == (1.0, 1.0, 1.0) else 0.125
    # the first dot
    dot0, abs0 = Mh @ hi(x0), np.abs(Mh) @ np.abs(hi(x0))
    ref = hi(ytemp_in) - dot0 if xside else dot0
    if exact:
        assert np.array_equal(yn, ref.astype(dt)), tag
    else:
        bounded("ynew dot", dt, yn, ref, gamma(n, dt) * abs0 * (1 + u) + (u * np.abs(ref) if xside else 0))
    # what follows the dot: bit for bit from the device's ynew and y12s
    ztn, zts, v, yh, u1 = fused_tail(yn, h, ytemp_in, zs, alpha, xside)
    assert same_bytes(out["ytemp"][:rows], ztn), tag
    assert same_bytes(out["ytemps"][:rows], yh), tag
    if exact and not logistic:
        assert np.array_equal(h, prox_exact(f["h"][:rows], v.astype(np.float64), rho).astype(dt)), tag
    else:
        check_prox("y12s prox" + (" logistic" if logistic else ""), dt, h, f, rows, rho, v)
    # column totals from the device's own u
    ex_tot = exact and not logistic
    check_totals("tot0", dt, M, n, rows, out["tot0"], yh, ex_tot, quantum)
    if not lean:
        check_totals("tot1", dt, M, n, rows, out["tot1"], u1, ex_tot, quantum)
    else:
        assert np.all(out["tot1"] == np.asarray(SENT, dt)), tag
    # scalars: |yprev - y|^2, |y12 - y|^2, |exact residual|^2, sum w h, |w|^2, |h|^2
    S = out["scalars"]
    a, b, w = ycur - yn, y12 - yn, v - h
    for k, (p, q) in {0: (a, a), 1: (b, b), 3: (w, h), 4: (w, w), 5: (h, h)}.items():
        sum_check("row scalar", S[k], p, q, rows)
    if lean:
        assert S[2] == 0.0, tag
    else:
        # the second dot comes back through the exact-residual sum only
        T = np.dtype(dt).type
        dot1, abs1 = Mh @ hi(x1), np.abs(Mh) @ np.abs(hi(x1))
        r_ref = (dot1 + hi(y12) + hi(T(c_old) * yt) - hi(ycur)) if xside else dot1 - hi(y12)
        s_ref = np.sum(np.asarray(r_ref, np.longdouble) ** 2)
        if exact:
            assert S[2] == float(s_ref), tag
        else:
            d = gamma(n, dt) * abs1 + 4 * u * (np.abs(dot1) + np.abs(hi(y12)) + (np.abs(hi(yt * T(c_old))) + np.abs(hi(ycur)) if xside else 0))
            bar = np.sum(2 * np.abs(r_ref) * d + d * d) + gamma(rows + 32, np.float64) * s_ref
            bounded("second dot (residual sum)", dt, np.asarray([np.longdouble(S[2])]), np.asarray([s_ref]),
                    np.asarray([bar], np.longdouble))


def run_iter(rng, dt, rows, n, data, form=P.PASS_ITER_FULL, functor=P.PASS_FN_CHEAP, num_cu=1, force=None, rho=2.0,
             alpha=1.5, zs=0.5, c_old=0.5, hs=None):
    if functor == P.PASS_FN_LOGISTIC:
        hs = np.full(rows, LOGISTIC)
    M, vec, f = iter_case(rng, dt, rows, n, data, functor, hs)
    if data != "int":
        rho, zs, c_old = 0.7, 1.3, 0.9
    lean = form == P.PASS_ITER_LEAN
    out = P.dense_pass_check(form, M, n, vec, functor=functor, f=f, rho=rho, alpha=alpha, zs=zs, c_old=c_old, num_cu=num_cu,
                             force=force)
    check_iter((np.dtype(dt).name, rows, n, form, functor, num_cu), dt, M, n, rows, vec, f, out, functor, lean, rho, alpha,
               zs, c_old, data == "int")
    return out


def probe(dt, form, n, num_cu, functor=P.PASS_FN_CHEAP, force=None):
    """info of the form at this width with enough rows to fill the grid of a small num_cu"""
    rows = 200
    rng = np.random.default_rng(0)
    if form in (P.PASS_ITER_FULL, P.PASS_ITER_LEAN, P.PASS_PRE_ACC):
        hs = np.full(rows, LOGISTIC) if functor == P.PASS_FN_LOGISTIC else None
        M, vec, f = iter_case(rng, dt, rows, n, "int", functor, hs)
        return P.dense_pass_check(form, M, n, vec, functor=functor, f=f, num_cu=num_cu, force=force)["info"]
    M, vec = exact_case(rng, dt, rows, n, "int")
    return P.dense_pass_check(form, M, n, vec, num_cu=num_cu, force=force)["info"]


def row_counts(R, grid):
    return sorted({r for r in (1, R - 1, R + 1, grid * R - 1, grid * R + 1, 2 * grid * R + R + 1) if r >= 1})


# ---- EXACT: the dot + column-sum pass of stream_rows_kernel (the form that runs windowed) ------------------------------

def exact_case(rng, dt, rows, n, data):
    M = make_M(rng, dt, rows, n, data)
    if data == "int":
        x0, y12, yt, ycur = ints(rng, n, dt), ints(rng, rows, dt), ints(rng, rows, dt), ints(rng, rows, dt)
        x12, xt, x_cur = ints(rng, n, dt), ints(rng, n, dt), ints(rng, n, dt)
    else:
        x0 = rng.standard_normal(n).astype(dt)
        y12, yt, ycur = (rng.normal(0, 3.0, rows).astype(dt) for _ in range(3))
        x12, xt, x_cur = (rng.normal(0, 3.0, n).astype(dt) for _ in range(3))
    vec = dict(x0=colv(dt, n, x0), y12=rowv(dt, rows, y12), yt=rowv(dt, rows, yt), ycur=rowv(dt, rows, ycur),
               x12=colv(dt, n, x12), xt=colv(dt, n, xt), x_cur=colv(dt, n, x_cur), tot0=colv(dt, n),
               dots=np.full(2 * (rows + 3), SENT, dt))
    return M, vec


def run_exact(rng, dt, rows, n, data, num_cu=1, force=None):
    M, vec = exact_case(rng, dt, rows, n, data)
    zs = 0.5 if data == "int" else 1.3
    out = P.dense_pass_check(P.PASS_EXACT, M, n, vec, zs=zs, num_cu=num_cu, force=force)
    T, u = np.dtype(dt).type, np.finfo(dt).eps / 2
    Mh = hi(M[:rows, :n])
    x0, y12, yt, ycur = vec["x0"][:n], vec["y12"][:rows], vec["yt"][:rows], vec["ycur"][:rows]
    dot, absdot = Mh @ hi(x0), np.abs(Mh) @ np.abs(hi(x0))
    tag = (np.dtype(dt).name, rows, n, num_cu, force)
    # the plain row dots (stream_rows_kernel, dot only)
    dots = out["dots"]
    if data == "int":
        assert np.array_equal(dots[:rows], dot.astype(dt)), tag
    else:
        bounded("plain dot", dt, dots[:rows], dot, gamma(n, dt) * absdot)
    assert np.all(dots[rows:] == np.asarray(SENT, dt)), tag
    # row scalar |M x0 - y12|^2: the dot comes back through it
    r_ref = dot - hi(y12)
    s_ref = np.sum(np.asarray(r_ref, np.longdouble) ** 2)
    if data == "int":
        assert out["scalars"][0] == float(s_ref), tag
    else:
        d = gamma(n, dt) * absdot + 2 * u * (np.abs(dot) + np.abs(hi(y12)))
        bounded("exact row residual sum", dt, np.asarray([np.longdouble(out["scalars"][0])]), np.asarray([s_ref]),
                np.asarray([np.sum(2 * np.abs(r_ref) * d + d * d) + gamma(rows + 32, np.float64) * s_ref], np.longdouble))
    # column totals of u = y12 + zs yt - ycur (working dtype, as ExactRowOp forms it)
    uvec = (y12 + T(zs) * yt) - ycur
    check_totals("exact tot0", dt, M, n, rows, out["tot0"], uvec, data == "int")
    # column scalar from the device's totals: sum_j (tot + x12 + zs xt - xcur)^2
    tot = out["tot0"][:n]
    sd = ((tot + vec["x12"][:n]) + T(zs) * vec["xt"][:n]) - vec["x_cur"][:n]
    sum_check("exact col scalar", out["col_scalars"][0], sd, sd, n)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("plan", PLANS)
def test_exact_integers_every_shape_at_its_natural_widths(dtype, plan):
    """Bit for bit on integers at the first, a ragged and the last width of every shape of POGS_STREAM_PLANS, with
    num_cu in {1, 3} so that a few dozen rows wrap round the grid, exercise both slots and end on a ragged tile (3: a
    grid that is no multiple of 8 takes logical_block_id's remainder branch).  ITER_FULL with the cheap functor at every
    row count; the lean form (fp64), XSIDE, PRE_ACC and EXACT at two of them; the 1024-thread shapes run EXACT alone (the
    one-pass kernels are not built for them).  Chosen: rho = 2, zs = 0.5, alpha = 1.5, c_old = 0.5."""
    tpb, nv = plan
    rng = np.random.default_rng(100 + tpb + nv)
    for n in widths(dtype, tpb, nv):
        for num_cu in (1, 3):
            if tpb == 1024:
                info = probe(dtype, P.PASS_EXACT, n, num_cu)
                assert (info["tpb"], info["nv"], info["xl"], info["kernel"]) == (tpb, nv, 0, P.PASS_KERNEL_PLAIN)
                for rows in row_counts(info["rows_per_step"], info["grid"]):
                    run_exact(rng, dtype, rows, n, "int", num_cu)
                continue
            info = probe(dtype, P.PASS_ITER_FULL, n, num_cu)
            assert (info["tpb"], info["nv"], info["xl"], info["kernel"]) == (tpb, nv, 0, P.PASS_KERNEL_PLAIN)
            R, grid = info["rows_per_step"], info["grid"]
            counts = row_counts(R, grid)
            for rows in counts:
                out = run_iter(rng, dtype, rows, n, "int", num_cu=num_cu)
                assert out["info"]["nparts"] == min(grid, -(-rows // R))
            for rows in (counts[-1], R + 1):
                run_iter(rng, dtype, rows, n, "int", functor=P.PASS_FN_XSIDE, num_cu=num_cu)
                run_exact(rng, dtype, rows, n, "int", num_cu)
                run_pre_acc(rng, dtype, rows, n, "int", P.PASS_FN_CHEAP, num_cu)
            if dtype == np.float64:
                li = probe(dtype, P.PASS_ITER_LEAN, n, num_cu)
                for rows in row_counts(li["rows_per_step"], li["grid"])[-3:]:
                    run_iter(rng, dtype, rows, n, "int", form=P.PASS_ITER_LEAN, num_cu=num_cu)
                    run_iter(rng, dtype, rows, n, "int", form=P.PASS_ITER_LEAN, functor=P.PASS_FN_LOGISTIC, num_cu=num_cu)


def run_pre_acc(rng, dt, rows, n, data, functor, num_cu=1, cols=P.PASS_COLS_REDUCE):
    M, vec, _ = iter_case(rng, dt, rows, n, data, functor)
    zs = 0.5 if data == "int" else 1.3
    vec = {k: vec[k] for k in ("ycur", "y12", "yt", "ytemp", "tot0", "tot1")}
    out = P.dense_pass_check(P.PASS_PRE_ACC, M, n, vec, functor=functor, zs=zs, num_cu=num_cu)
    T = np.dtype(dt).type
    ycur, y12, yt, ytemp = (vec[k][:rows] for k in ("ycur", "y12", "yt", "ytemp"))
    u1 = y12 if functor == P.PASS_FN_XSIDE else (y12 + T(zs) * yt) - ycur
    check_totals("pre_acc tot0", dt, M, n, rows, out["tot0"], ytemp, data == "int")
    check_totals("pre_acc tot1", dt, M, n, rows, out["tot1"], u1, data == "int")
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_real_data_bounds_per_form(dtype):
    """The gamma bounds on badly scaled data: every form at a narrow, a middle and a wide shape, every cheap function, the
    logistic functor in the plain kernel, PRE_ACC with both functors, EXACT."""
    rng = np.random.default_rng(7)
    V = vecw(dtype)
    for n, num_cu in ((61, 1), (256 * 3 * V - 1, 3), (512 * 8 * V - V - 1, 1)):
        info = probe(dtype, P.PASS_ITER_FULL, n, num_cu)
        rows = 2 * info["grid"] * info["rows_per_step"] + info["rows_per_step"] + 1
        hs = np.resize(np.asarray(CHEAP_FNS), rows)
        run_iter(rng, dtype, rows, n, "real", num_cu=num_cu, hs=hs)
        run_iter(rng, dtype, rows, n, "real", functor=P.PASS_FN_XSIDE, num_cu=num_cu, alpha=1.7)
        out = run_iter(rng, dtype, rows, n, "real", functor=P.PASS_FN_LOGISTIC, num_cu=num_cu, alpha=1.0)
        assert out["info"]["kernel"] == P.PASS_KERNEL_PLAIN
        if dtype == np.float64:
            run_iter(rng, dtype, rows, n, "real", form=P.PASS_ITER_LEAN, num_cu=num_cu, hs=hs)
        run_pre_acc(rng, dtype, rows, n, "real", P.PASS_FN_CHEAP, num_cu)
        run_pre_acc(rng, dtype, rows, n, "real", P.PASS_FN_XSIDE, num_cu)
        run_exact(rng, dtype, rows, n, "real", num_cu)


def device_num_cu():
    """the CU count a num_cu = 0 call uses: a 64-thread PRE_ACC pass over enough rows fills 8 workgroups per CU"""
    rng = np.random.default_rng(0)
    rows = 8 * 8 * 1024 + 1
    M, vec, _ = iter_case(rng, np.float32, rows, 4, "int", P.PASS_FN_XSIDE)
    vec = {k: vec[k] for k in ("y12", "ytemp", "tot0", "tot1")}
    info = P.dense_pass_check(P.PASS_PRE_ACC, M, 4, vec, functor=P.PASS_FN_XSIDE)["info"]
    assert info["grid"] % 8 == 0 and info["grid"] < -(-rows // info["rows_per_step"])
    return info["grid"] // 8


def test_the_prefetching_kernel_fp32_256x5_logistic():
    """stream_rows2_pf_kernel (fp32, 256 x 5, logistic): its unconditional, clamped loads at rows < R, at a ragged last
    tile and at a width whose last vector is the only one of its thread; with num_cu in {1, 3} and, once, on the device's
    own grid with rows = 2 grid R + 1 (n = 4100, about 2000 rows, 35 MB).  On integers ynew, ytemp and the three residual
    sums are exact; the logistic prox is compared with the oracle and the totals with M^T u of the device's own u."""
    dt = np.float32
    rng = np.random.default_rng(11)
    for n in (4097, 4100, 5119, 5120):
        for num_cu in (1, 3):
            info = probe(dt, P.PASS_ITER_FULL, n, num_cu, functor=P.PASS_FN_LOGISTIC)
            assert (info["tpb"], info["nv"], info["kernel"]) == (256, 5, P.PASS_KERNEL_PF)
            assert info["grid"] == 2 * num_cu and info["rows_per_step"] == 2
            for rows in row_counts(2, info["grid"]):
                out = run_iter(rng, dt, rows, n, "int", functor=P.PASS_FN_LOGISTIC, num_cu=num_cu, alpha=1.0)
                assert out["info"]["nparts"] == min(info["grid"], -(-rows // 2))
            run_iter(rng, dt, 2 * info["grid"] * 2 + 3, n, "real", functor=P.PASS_FN_LOGISTIC, num_cu=num_cu)
    # the shape forced onto rows of exactly one vector, and a few more: all lanes but one load a clamped column
    for n in (1, 4, 5, 9):
        for rows in (1, 3, 9):
            out = run_iter(rng, dt, rows, n, "int", functor=P.PASS_FN_LOGISTIC, num_cu=1, force=(256, 5), alpha=1.0)
            assert out["info"]["kernel"] == P.PASS_KERNEL_PF
    # the cheap functor at this shape runs the plain kernel at two workgroups per CU (bpc_override)
    info = probe(dt, P.PASS_ITER_FULL, 4100, 3)
    assert (info["kernel"], info["grid"]) == (P.PASS_KERNEL_PLAIN, 6)
    ncu = device_num_cu()
    rows = 2 * (2 * ncu) * 2 + 1
    out = run_iter(rng, dt, rows, 4100, "int", functor=P.PASS_FN_LOGISTIC, num_cu=0, alpha=1.0, rho=1.0, zs=1.0)
    assert out["info"]["kernel"] == P.PASS_KERNEL_PF and rows == 2 * out["info"]["grid"] * out["info"]["rows_per_step"] + 1
    out = run_iter(rng, dt, rows, 4100, "int", num_cu=0, alpha=1.0, rho=1.0, zs=1.0)
    assert out["info"]["kernel"] == P.PASS_KERNEL_PLAIN and out["info"]["grid"] == 2 * ncu


def test_the_shipped_grid_wraps_fp64_256x10():
    """fp64 at 256 x 10 on the device's own CU count, rows = 2 grid R + 1: full and lean form"""
    dt = np.float64
    rng = np.random.default_rng(12)
    ncu = device_num_cu()
    n = 256 * 10 * 2 - 3
    for form, per_cu, R in ((P.PASS_ITER_FULL, 2, 1), (P.PASS_ITER_LEAN, 2, 2)):
        rows = 2 * per_cu * ncu * R + 1
        out = run_iter(rng, dt, rows, n, "int", form=form, num_cu=0)
        info = out["info"]
        assert (info["tpb"], info["nv"], info["rows_per_step"]) == (256, 10, R)
        assert rows == 2 * info["grid"] * R + 1, info


# ---- windowed plans --------------------------------------------------------------------------------------------------

def test_natural_windowed_exact_pass_fp32_40001():
    rng = np.random.default_rng(13)
    for rows in (1, 33):
        out = run_exact(rng, np.float32, rows, 40001, "int", num_cu=3)
        assert out["info"]["xl"] == 1 and out["info"]["windows"] == 5 and (out["info"]["tpb"], out["info"]["nv"]) == (256, 8)
    run_exact(rng, np.float32, 33, 40001, "real", num_cu=3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_window_passes(dtype, monkeypatch):
    """POGS_AMD_XL_LIMIT (vectors): rows wider than that take 64 x 2 windows, so small matrices span several"""
    monkeypatch.setenv("POGS_AMD_XL_LIMIT", "16")
    rng = np.random.default_rng(14)
    V = vecw(dtype)
    for n in (17 * V - 1, 128 * V, 128 * V + 1, 3 * 128 * V - V - 1):
        for rows in (1, 5, 97, 200):
            out = run_exact(rng, dtype, rows, n, "int", num_cu=1)
            assert out["info"]["xl"] == 1 and out["info"]["windows"] == -(-rup(n, V) // (128 * V))
        run_exact(rng, dtype, 97, n, "real", num_cu=3)
    out = run_sweep(rng, dtype, 3 * 128 * V - 5)
    assert out["info"]["xl"] == 1 and out["info"]["windows"] == 3 and out["info"]["kernel"] == P.PASS_KERNEL_PLAIN


# ---- the W sweep: stream_tri_kernel ------------------------------------------------------------------------------------

def make_W(rng, dt, n):
    """square lower-triangular integers; right of the diagonal: zero inside the diagonal's vector, NaN beyond"""
    V = vecw(dt)
    n_pad = rup(n, V)
    W = np.zeros((n, n_pad + 2 * V), dt)
    W[:, :n] = np.tril(rng.integers(-4, 5, (n, n), dtype=np.int8))
    first_nan = (np.arange(n) // V + 1) * V              # first column of the first vector wholly right of the diagonal
    W[np.arange(W.shape[1])[None, :] >= first_nan[:, None]] = np.nan
    return W


def run_sweep(rng, dt, n, num_cu=None, force=None, add=True):
    W = make_W(rng, dt, n)
    num_cu = (3 if n < 1100 else 0) if num_cu is None else num_cu      # (a 200 MB triangle on the device's own grid)
    r, a = ints(rng, n, dt), ints(rng, n, dt)
    vec = dict(x0=colv(dt, n, r), tot0=colv(dt, n), dots=np.full(2 * (n + 3), SENT, dt))
    if add:
        vec["x1"] = colv(dt, n, a)
    out = P.dense_pass_check(P.PASS_W_SWEEP, W, n, vec, num_cu=num_cu, force=force)
    L = np.tril(W[:, :n].astype(np.float64))             # exact: integers
    rr = (r + a if add else r).astype(np.float64)
    t = L @ rr
    x, absx = L.T @ t, np.abs(L).T @ (np.abs(L) @ np.abs(rr))
    tag = (np.dtype(dt).name, n, num_cu, force)
    assert np.array_equal(out["dots"][:n], t.astype(dt)), tag        # t = W (r + add) by the dot-only lower launch
    assert np.all(out["dots"][n:] == np.asarray(SENT, dt)), tag
    got = out["tot0"]
    g = gamma(n, dt)
    # t is not returned by the solver's form: the composite against W^T (W r), two stages of n-term sums
    bounded("w sweep composite", dt, got[:n], x, g * absx * (2 + g))
    assert exact_fits(dt, np.abs(L).T @ np.abs(t), quantum=1.0), (tag, "the integers of this case leave the mantissa")
    assert np.array_equal(got[:n], x.astype(dt)), tag
    n_pad = rup(n, vecw(dt))
    assert np.all(got[n:n_pad] == 0) and np.all(got[n_pad:] == np.asarray(SENT, dt)), tag
    return out


SWEEPS = [   # (dtype, tpb, nv, n): natural widths that cross q TPB VEC and h TPB VEC, n no multiple of 4 R
    (np.float32, 64, 1, 250), (np.float32, 64, 2, 301), (np.float32, 64, 4, 603),
    (np.float64, 256, 3, 1031), (np.float64, 256, 5, 2051), (np.float64, 256, 6, 2563), (np.float64, 256, 8, 3075),
    (np.float64, 256, 10, 4099), (np.float64, 512, 6, 5123),
]


@pytest.mark.parametrize("case", SWEEPS, ids=lambda c: "%s-%dx%d-%d" % (np.dtype(c[0]).name, c[1], c[2], c[3]))
def test_w_sweep_phases_at_natural_widths(case):
    """x = W^T (W (r + add)) over the lower triangle by stream_tri_kernel, all six TriPhases structures (NV 1, 2-3, 4-5, 6,
    8, 10): rows below and above both phase boundaries, the last step of every phase ragged."""
    dt, tpb, nv, n = case
    rng = np.random.default_rng(n)
    out = run_sweep(rng, dt, n)
    info = out["info"]
    assert (info["tpb"], info["nv"], info["kernel"], info["xl"]) == (tpb, nv, P.PASS_KERNEL_TRI, 0)
    V, q = vecw(dt), nv // 4
    h = nv // 2 if nv // 2 > q else 0
    assert n > max(q, h) * tpb * V and n % (4 * info["rows_per_step"]) != 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_w_sweep_small_sizes_and_the_1024_thread_shapes(dtype):
    """sizes inside the first phase and around its boundary at 64 x 4 / 64 x 2 (fp32: 256 rows, fp64: 128), one row, no
    addend; the 1024-thread shapes at a forced plan: (1024, 6) runs the triangular kernel, (1024, 8) the plain one"""
    rng = np.random.default_rng(15)
    V = vecw(dtype)
    for n in (1, 2, V + 1, 63, 64 * V - 1, 64 * V + 1, 64 * V + 9, 128 * V + 3):
        for num_cu in (1, 3):
            run_sweep(rng, dtype, n, num_cu=num_cu, add=(n % 2 == 1))
    for nv, kernel in ((6, P.PASS_KERNEL_TRI), (8, P.PASS_KERNEL_PLAIN)):
        for n in (301, 1024 * V + 7):
            out = run_sweep(rng, dtype, n, num_cu=3, force=(1024, nv))
            assert (out["info"]["tpb"], out["info"]["nv"], out["info"]["kernel"]) == (1024, nv, kernel)


# ---- the column side: pre_cols_kernel, pack_cols_kernel ----------------------------------------------------------------

NPARTS = (1, 15, 16, 17, 31, 32, 33, 64, 65)


def parts_case(rng, dt, nparts, n, data):
    """a PRE_ACC pass at 64 x nv whose grid is exactly nparts: 8 rows per step, num_cu = 16 (at most 128 workgroups)"""
    rows = nparts * 8 - 3
    M, vec, _ = iter_case(rng, dt, rows, n, data, P.PASS_FN_XSIDE)
    return M, {k: vec[k] for k in ("y12", "ytemp")}, rows


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("data", ["int", "real"])
def test_pre_cols_second_stage(dtype, data):
    """pre_cols_kernel<T, false> behind a PRE_ACC pass, nparts straddling its loop strides (16, 32), with both partial
    sets and with the second absent: x12 against the oracle (exact configuration: the model), xtemp bit for bit from the
    device's x12, rhs = M^T u0 exact on integers and gamma-bounded on real data, the four scalars from the device's
    vectors; scalar 3 is exactly 0 without the second set."""
    rng = np.random.default_rng(21)
    V = vecw(dtype)
    T = np.dtype(dtype).type
    rho, alpha, zs = (2.0, 1.5, 0.5) if data == "int" else (0.7, 1.7, 1.3)
    for nparts in NPARTS:
        for n in (61, 16 * V + 1):        # one workgroup of columns, and a second with a single column
            M, vec, rows = parts_case(rng, dtype, nparts, n, data)
            if data == "int":
                x_cur, xt = ints(rng, n, dtype), ints(rng, n, dtype)
                g = fn_arrays(dtype, n, rup(n, V) + 3, rng.choice(EXACT_FNS, n))
            else:
                x_cur, xt = rng.normal(0, 3.0, n).astype(dtype), rng.normal(0, 0.3, n).astype(dtype)
                g = fn_arrays(dtype, n, rup(n, V) + 3, rng.integers(0, 16, n), rng)
            vec.update(x_cur=colv(dtype, n, x_cur), xt=colv(dtype, n, xt), x12=colv(dtype, n), xtemp=colv(dtype, n),
                       rhs=colv(dtype, n))
            for cols in (P.PASS_COLS_PRE, P.PASS_COLS_PRE_ONE):
                out = P.dense_pass_check(P.PASS_PRE_ACC, M, n, vec, functor=P.PASS_FN_XSIDE, cols=cols, g=g, rho=rho,
                                         alpha=alpha, zs=zs, num_cu=16)
                tag = (np.dtype(dtype).name, data, nparts, n, cols)
                assert out["info"]["nparts"] == nparts and (out["info"]["tpb"], out["info"]["rows_per_step"]) == (64, 8)
                ztv = T(zs) * xt
                v = x_cur - ztv
                h = out["x12"][:n]
                if data == "int":
                    assert np.array_equal(h, prox_exact(g["h"][:n], v.astype(np.float64), rho).astype(dtype)), tag
                else:
                    check_prox("x12 prox", dtype, h, g, n, rho, v)
                xtemp = (ztv + T(alpha) * h) + (T(1) - T(alpha)) * x_cur
                assert same_bytes(out["xtemp"][:n], xtemp), tag
                for k in ("x12", "xtemp"):
                    assert np.all(out[k][n:] == np.asarray(SENT, dtype)), tag
                check_totals("pre_cols rhs", dtype, M, n, rows, out["rhs"], vec["ytemp"][:rows], data == "int")
                w = v - h
                S = out["col_scalars"]
                sum_check("pre_cols scalar", S[0], w, h, n)
                sum_check("pre_cols scalar", S[1], w, w, n)
                sum_check("pre_cols scalar", S[2], h, h, n)
                if cols == P.PASS_COLS_PRE_ONE:
                    assert S[3] == 0.0, tag
                    continue
                # exact dual residual sd = ((t1 + h) + zs xt) - prev with t1 = (M^T y12)_j
                Mh = hi(M[:rows, :n])
                t1, abst1 = Mh.T @ hi(vec["y12"][:rows]), np.abs(Mh).T @ np.abs(hi(vec["y12"][:rows]))
                sd_ref = t1 + hi(h) + hi(T(zs) * xt) - hi(x_cur)
                s_ref = np.sum(np.asarray(sd_ref, np.longdouble) ** 2)
                if data == "int":
                    assert exact_fits(dtype, abst1) and S[3] == float(s_ref), tag
                else:
                    u = np.finfo(dtype).eps / 2
                    d = gamma(rows + 32, dtype) * abst1 + 4 * u * (np.abs(t1) + np.abs(hi(h)) + np.abs(hi(T(zs) * xt)) + np.abs(hi(x_cur)))
                    bounded("pre_cols exact-dual sum", dtype, np.asarray([np.longdouble(S[3])]), np.asarray([s_ref]),
                            np.asarray([np.sum(2 * np.abs(sd_ref) * d + d * d) + gamma(n + 32, np.float64) * s_ref], np.longdouble))


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_cols_equals_reduce_cols_bit_for_bit(dtype):
    """pack_cols_kernel's totals, cast back, are reduce_cols_kernel's (the claim of colsum_group), on badly scaled data,
    nparts straddling the strides of both loops (b + 56 < nparts: 57, 63, 64, 65, 120)"""
    rng = np.random.default_rng(22)
    V = vecw(dtype)
    for nparts in NPARTS + (57, 63, 120):
        n = 32 * V + 5
        M, vec, rows = parts_case(rng, dtype, nparts, n, "real")
        n_pad = rup(n, V)
        red = P.dense_pass_check(P.PASS_PRE_ACC, M, n, dict(vec, tot0=colv(dtype, n), tot1=colv(dtype, n)),
                                 functor=P.PASS_FN_XSIDE, num_cu=16)
        pk = P.dense_pass_check(P.PASS_PRE_ACC, M, n, dict(vec, pack=np.full(2 * n_pad + 6, SENT)),
                                functor=P.PASS_FN_XSIDE, cols=P.PASS_COLS_PACK, num_cu=16)
        assert red["info"]["nparts"] == pk["info"]["nparts"] == nparts
        pack = pk["pack"]
        assert same_bytes(pack[:n].astype(dtype), red["tot0"][:n]) and same_bytes(pack[n_pad:n_pad + n].astype(dtype), red["tot1"][:n])
        assert np.all(pack[n:n_pad] == 0) and np.all(pack[n_pad + n:2 * n_pad] == 0)
        assert np.all(pack[2 * n_pad:] == SENT)                       # no scalar jobs behind a PRE_ACC pass
        check_totals("pack source tot0", dtype, M, n, rows, red["tot0"], vec["ytemp"][:rows], False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_cols_scalar_jobs_behind_the_iteration_pass(dtype):
    """the extra workgroup of pack_cols_kernel sums the pass's six scalars with the strides 6 / 0 and 6 / 3: on integers
    they equal launch_sum_jobs's sums, and the totals equal reduce_cols's"""
    rng = np.random.default_rng(23)
    n, rows, V = 300, 8 * 24 * 2 + 5, vecw(dtype)
    n_pad = rup(n, V)
    M, vec, f = iter_case(rng, dtype, rows, n, "int", P.PASS_FN_CHEAP)
    kw = dict(f=f, rho=2.0, alpha=1.5, zs=0.5, num_cu=3)
    red = P.dense_pass_check(P.PASS_ITER_FULL, M, n, vec, **kw)
    pk = P.dense_pass_check(P.PASS_ITER_FULL, M, n, dict({k: v for k, v in vec.items() if k not in ("tot0", "tot1")},
                                                         pack=np.full(2 * n_pad + 6, SENT)), cols=P.PASS_COLS_PACK, **kw)
    check_iter("pack source", dtype, M, n, rows, vec, f, red, P.PASS_FN_CHEAP, False, 2.0, 1.5, 0.5, 0.5, True)
    assert np.array_equal(pk["pack"][2 * n_pad:], red["scalars"]) and np.array_equal(pk["scalars"], red["scalars"])
    assert np.array_equal(pk["pack"][:n], red["tot0"][:n]) and np.array_equal(pk["pack"][n_pad:n_pad + n], red["tot1"][:n])


# ---- isolation -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_a_rows_outputs_do_not_depend_on_the_grid(dtype):
    rng = np.random.default_rng(31)
    rows, n = 3001, 1100
    M, vec, f = iter_case(rng, dtype, rows, n, "real", P.PASS_FN_CHEAP)
    kw = dict(f=f, rho=0.7, alpha=1.7, zs=1.3)
    one = P.dense_pass_check(P.PASS_ITER_FULL, M, n, vec, num_cu=1, **kw)
    dev = P.dense_pass_check(P.PASS_ITER_FULL, M, n, vec, num_cu=0, **kw)
    assert one["info"]["grid"] < dev["info"]["grid"]
    for k in ("ynew", "ytemp", "y12s", "ytemps"):
        assert same_bytes(one[k], dev[k]), k
    for out in (one, dev):
        check_iter("isolation", dtype, M, n, rows, vec, f, out, P.PASS_FN_CHEAP, False, 0.7, 1.7, 1.3, 0.0, False)


def test_zz_report():
    """prints the largest error-to-bound ratio per check and dtype (profiles/dense_pass_accuracy.txt is this table)"""
    for (what, dt), r in sorted(RATIOS.items()):
        print("RATIO %-34s %-8s %.3e" % (what, dt, r))
    assert all(r <= 1.0 for r in RATIOS.values())
