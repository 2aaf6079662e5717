"""stream_rows_mixed_kernel (csrc/stream_mixed.h): the single-vector streaming pass over a float32 matrix with fp64
arithmetic, in its three forms -- ACC (GemvTOp), DOT + ACC (DcgQRowOp, guarded) and DOT (ProjTailOp) -- through
PogsAmdStreamMixedCheck, i.e. through the launch functions and functors the fused CGLS loop of a mixed-storage handle
uses, with the second stage (reduce_cols, the scalar records summed).

  * exact integers: small-integer M, x and u make every product and every partial sum an integer far below 2^53, so q,
    the column totals and |q|^2 must EQUAL numpy's integer results whatever the order of the sums: n around the vector
    widths (n_pad % 4 == 2 at 2, 6, 130, 1030: the upper pair of the row's last float vector has no x entry and no
    partial slot), rows around the rows-per-step R of the form (1, R - 1, R, R + 1, 3 R + 1, 1037), one CU and the
    device's (other grids);
  * every shape of the mixed plan forced, at its first and at its full width (and at full width - 2, n_pad % 4 == 2,
    which includes 256 x 10 x 4 - 2), the 256 x 6 .. 10 ones running as 512 threads;
  * real, badly scaled data against np.longdouble: rows within gamma_(n+8) sum_j |a_ij x_j|, column totals -- with the
    device's own q as coefficients -- within gamma_(rows+grid+8) sum_i |a_ij q_i|, gamma_k = k u / (1 - k u), u = 2^-53
    (a row dot is n products fused onto a running sum plus the wavefront tree and the NW partials; a column total adds
    at most `rows` fused products per workgroup and then `grid` partials; 8 covers the trees);
  * padding: ldm > round_up(n, 4) with NaN beyond never reaches a result;
  * the guard: with the done flag set a DOT + ACC launch leaves q, the partials and the totals as given;
  * two calls return the same bytes.
Every ratio error / bar is printed (pytest -s); profiles/stream_mixed_accuracy.txt is that table."""
import numpy as np
import pytest

from helpers import gamma, same_bytes
from pogs_amd import _lib

pytestmark = pytest.mark.gpu
ACC, DOT_ACC, DOT = _lib.STREAM_MIXED_ACC, _lib.STREAM_MIXED_DOT_ACC, _lib.STREAM_MIXED_DOT
FORMS = {"acc": ACC, "dot_acc": DOT_ACC, "dot": DOT}
SHAPES = [(64, 1), (64, 2), (64, 4), (256, 2), (256, 3), (256, 4), (256, 5), (256, 6), (256, 8), (256, 10)]


def report(line):
    print("stream_mixed: " + line)


def padded(M, n, ldm=None, fill=0.0):
    """rows of round_up(n, 4) floats (zero past n) at stride ldm, `fill` beyond"""
    rows, n32 = M.shape[0], -(-n // 4) * 4
    out = np.full((rows, ldm or n32), fill, np.float32)
    out[:, :n32] = 0
    out[:, :n] = M
    return out


def vec_pad(v, n):
    out = np.zeros(n + n % 2)
    out[:n] = v
    return out


def run(form, M, n, x=None, u=None, **kw):
    return _lib.stream_mixed_check(form, M, n, x=None if x is None else vec_pad(x, n), u=u, **kw)


def check_exact(form, M, n, x, u, **kw):
    """integers: the outputs equal numpy's; what the form does not write is still NaN"""
    Mi, rows = M.astype(np.int64), M.shape[0]
    out = run(form, padded(M, n), n, x=x, u=u, **kw)
    q = Mi @ x.astype(np.int64)
    if form == ACC:
        assert np.array_equal(out["tot"][:n], Mi.T @ u.astype(np.int64)), (n, rows, kw)
        assert np.all(np.isnan(out["q"])) and np.all(np.isnan(out["scalars"]))
    else:
        assert np.array_equal(out["q"], q), (n, rows, kw)
        assert out["scalars"][0] == float(np.sum(q * q)), (n, rows, kw)
    if form == DOT_ACC:
        assert np.array_equal(out["tot"][:n], Mi.T @ q), (n, rows, kw)
        assert np.isnan(out["scalars"][1])
    if form == DOT:
        assert out["scalars"][1] == out["scalars"][0] and np.all(np.isnan(out["tot"]))
    if form != DOT:
        assert not out["tot"][n:].any()   # the padding column of the totals is written as zero
    return out


def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7, 8, 130, 1030])
def test_exact_on_integers_around_the_vector_widths_and_the_rows_per_step(n):
    rng = np.random.default_rng(n)
    M_all = rng.integers(-4, 5, (1037, n)).astype(np.float32)
    x = rng.integers(-4, 5, n).astype(np.float64)
    u_all = rng.integers(-4, 5, 1037).astype(np.float64)
    for name, form in FORMS.items():
        for num_cu in (1, 0):
            R = run(form, padded(M_all[:1], n), n, x=x, u=u_all[:1], num_cu=num_cu)["info"]["rows_per_step"]
            grids = []
            for rows in sorted({1, R - 1, R, R + 1, 3 * R + 1, 1037} - {0}):
                out = check_exact(form, M_all[:rows], n, x, u_all[:rows], num_cu=num_cu)
                info = out["info"]
                assert info["rows_per_step"] == R and info["grid"] == min(-(-rows // R), (num_cu or device_cus()) * info["blocks_per_cu"])
                grids.append(info["grid"])
            report("exact n %4d %-7s num_cu %s: shape %dx%d R %d grids %s" % (n, name, num_cu or "device", info["tpb"], info["nv"], R, grids))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_shape_of_the_mixed_plan_at_its_first_and_full_width(shape):
    tpb, nv = shape
    k = SHAPES.index(shape)
    first = 1 if k == 0 else SHAPES[k - 1][0] * SHAPES[k - 1][1] * 4 + 1
    full = tpb * nv * 4
    rng = np.random.default_rng(tpb * nv)
    for n in (first, full - 2, full):
        x = rng.integers(-4, 5, n).astype(np.float64)
        for name, form in FORMS.items():
            R = run(form, padded(np.zeros((1, n), np.float32), n), n, x=x, u=np.zeros(1), num_cu=1, force=shape)["info"]["rows_per_step"]
            rows = 3 * R + 1
            M = rng.integers(-4, 5, (rows, n)).astype(np.float32)
            u = rng.integers(-4, 5, rows).astype(np.float64)
            info = check_exact(form, M, n, x, u, num_cu=1, force=shape)["info"]
            assert (info["tpb"], info["nv"]) == shape
            assert (info["exec_tpb"], info["exec_nv"]) == ((512, nv // 2) if tpb == 256 and nv >= 6 else shape)
            # unforced, the plan of n is this shape
            assert (lambda i: (i["tpb"], i["nv"]))(run(form, padded(M, n), n, x=x, u=u, num_cu=1)["info"]) == shape
    report("shape %dx%d: widths %d, %d, %d exact in all three forms" % (tpb, nv, first, full - 2, full))


REAL = [(1037, 130), (257, 1030), (100, 5122), (60, 10238)]


@pytest.mark.parametrize("rows,n", REAL, ids=lambda v: str(v))
def test_real_badly_scaled_data_within_the_gamma_bounds(rows, n):
    rng = np.random.default_rng(rows + n)
    M = (rng.standard_normal((rows, n)) * np.exp2(rng.uniform(-10, 10, (rows, 1))) * np.exp2(rng.uniform(-10, 10, (1, n)))).astype(np.float32)
    x = rng.standard_normal(n) * np.exp2(rng.uniform(-10, 10, n))
    u = rng.standard_normal(rows) * np.exp2(rng.uniform(-10, 10, rows))
    Ml, absM = M.astype(np.longdouble), np.abs(M).astype(np.longdouble)
    q_ref, q_abs = Ml @ x.astype(np.longdouble), absM @ np.abs(x).astype(np.longdouble)
    for name, form in FORMS.items():
        out = run(form, padded(M, n), n, x=x, u=u)
        grid, line = out["info"]["grid"], []
        if form != ACC:
            assert np.all(np.isfinite(out["q"]))
            ratio = float(np.max(np.abs(out["q"].astype(np.longdouble) - q_ref) / (gamma(n + 8, np.float64) * q_abs)))
            line.append("rows %.3f" % ratio)
            assert ratio <= 1.0, (name, ratio)
            # |q|^2 from the device's own q: `rows` fused products, then the records
            s_ref = np.sum(out["q"].astype(np.longdouble) ** 2)
            for k in range(out["info"]["ns"]):
                ratio = float(abs(np.longdouble(out["scalars"][k]) - s_ref) / (gamma(rows + grid + 8, np.float64) * s_ref))
                line.append("|q|^2[%d] %.3f" % (k, ratio))
                assert ratio <= 1.0, (name, k, ratio)
        if form != DOT:
            coef = (u if form == ACC else out["q"]).astype(np.longdouble)
            t_ref, t_abs = Ml.T @ coef, absM.T @ np.abs(coef)
            assert np.all(np.isfinite(out["tot"]))
            ratio = float(np.max(np.abs(out["tot"][:n].astype(np.longdouble) - t_ref) / (gamma(rows + grid + 8, np.float64) * t_abs)))
            line.append("columns %.3f" % ratio)
            assert ratio <= 1.0, (name, ratio)
        report("real %5d x %5d %-7s grid %4d: error / bar  %s" % (rows, n, name, grid, "  ".join(line)))


@pytest.mark.parametrize("n", [6, 130, 1027])
def test_padding_beyond_the_row_never_reaches_a_result(n):
    rng = np.random.default_rng(7 * n)
    rows = 41
    M = rng.standard_normal((rows, n)).astype(np.float32)
    x, u = rng.standard_normal(n), rng.standard_normal(rows)
    n32 = -(-n // 4) * 4
    for form in FORMS.values():
        tight = run(form, padded(M, n), n, x=x, u=u)
        loose = run(form, padded(M, n, ldm=n32 + 8, fill=np.nan), n, x=x, u=u)
        for k in ("q", "tot", "scalars"):
            assert same_bytes(tight[k], loose[k]), (form, k)
        written = {ACC: ("tot",), DOT_ACC: ("q", "tot"), DOT: ("q", "scalars")}[form]
        assert all(np.all(np.isfinite(loose[k])) for k in written)


def test_the_guard_leaves_everything_as_given():
    rng = np.random.default_rng(3)
    rows, n = 77, 130
    M = padded(rng.integers(-4, 5, (rows, n)).astype(np.float32), n)
    x = vec_pad(rng.integers(-4, 5, n).astype(np.float64), n)
    q0, tot0, s0 = np.arange(rows, dtype=np.float64), -np.arange(n, dtype=np.float64), np.array([5.0, 6.0])
    grid = _lib.stream_mixed_check(DOT_ACC, M, n, x=x, num_cu=2)["info"]["grid"]
    ended = _lib.stream_mixed_check(DOT_ACC, M, n, x=x, q=q0, tot=tot0, scalars=s0, done=1.0, num_cu=2, partials=grid * n)
    assert same_bytes(ended["q"], q0) and same_bytes(ended["tot"], tot0) and same_bytes(ended["scalars"], s0)
    assert np.all(np.isnan(ended["partials"]))   # as the entry left them before the launch
    ran = _lib.stream_mixed_check(DOT_ACC, M, n, x=x, q=q0, tot=tot0, scalars=s0, done=0.0, num_cu=2, partials=grid * n)
    assert np.array_equal(ran["q"], M[:, :n].astype(np.float64) @ x[:n]) and np.all(np.isfinite(ran["partials"]))
    assert np.array_equal(ran["partials"].reshape(grid, n).sum(axis=0), ran["tot"])


def test_two_calls_return_the_same_bytes():
    rng = np.random.default_rng(11)
    rows, n = 1037, 1030
    M = padded(rng.standard_normal((rows, n)).astype(np.float32), n)
    x, u = rng.standard_normal(n), rng.standard_normal(rows)
    for form in FORMS.values():
        a, b = (_lib.stream_mixed_check(form, M, n, x=x, u=u) for _ in range(2))
        for k in ("q", "tot", "scalars"):
            assert same_bytes(a[k], b[k]), (form, k)
