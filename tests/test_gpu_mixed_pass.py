"""GPU tests of the mixed-storage pass (csrc/stream_mixed.h: stream_rows2_mixed_kernel -- the fp64 one-pass iteration's
pass over a FLOAT matrix) through PogsAmdDensePassMixedCheck, against PogsAmdDensePassCheck in fp64 on M.astype(float64):
the existing entry is the yardstick and is unchanged.  The helpers, the poison layout and the model (check_iter) are those
of tests/test_gpu_dense_passes.py, imported, not copied.

Layout and poison: the float matrix has ldm = round_up(n, 4) + 8 with NaN in [round_up(n, 4), ldm) and zeros in
[n, round_up(n, 4)); the vectors are those of the fp64 case: n_pad = round_up(n, 2) entries, NaN (inputs) or a sentinel
(outputs) in the three elements beyond -- when n_pad % 4 == 2 the last float vector of a row reaches two columns past
n_pad, exactly where that poison sits: a kernel that loaded x there, or stored a partial there, shows it.

Two kinds of check:
  * exact integers (entries in [-4, 4], the exact configuration of test_gpu_dense_passes.py): every output of the mixed
    entry equals the fp64 entry's BIT FOR BIT -- row outputs, both column totals, the six scalars and the second-stage
    outputs (REDUCE, PRE, PRE_ONE, PACK) -- and the model of check_iter.  With the LOGISTIC functor the prox is not an
    exact number: the row outputs and the three residual sums (functions of the exact dots alone) are still compared bit
    for bit, the column totals and the three prox sums -- sums of inexact terms, added in this kernel's own grouping --
    through check_iter's bounds;
  * badly scaled real data whose entries are representable in float: check_iter's gamma bounds.  Their addend counts
    hold for this kernel's partition: a dot has n products whatever the split into threads and wavefronts (gamma_n), a
    column total rows products plus the second stage's adds (gamma_(rows + 32): the bound of ANY summation order of
    that many terms), a scalar likewise.  The largest error / bound ratios are printed by test_zz_report
    (profiles/mixed_pass_accuracy.txt is that table)."""
import numpy as np
import pytest

import test_gpu_dense_passes as dp
from helpers import same_bytes
from pogs_amd import _lib as P

pytestmark = pytest.mark.gpu

F64 = np.float64
MIXED_PLANS = [(64, 1), (64, 2), (64, 4), (256, 2), (256, 3), (256, 4), (256, 5), (256, 6), (256, 8), (256, 10)]
MIXED_CAPS = sorted(t * v for t, v in MIXED_PLANS)
RATIOS = {}     # this file's table: check_iter's notes are redirected here (see the fixture)
ROW_OUT = ("ynew", "ytemp", "y12s", "ytemps")


@pytest.fixture(autouse=True)
def _own_ratio_table(monkeypatch):
    monkeypatch.setattr(dp, "RATIOS", RATIOS)


def to_f32_matrix(M64, n):
    """the float matrix of the mixed entry from the fp64 case's: same values (they must be representable), zero
    padding to round_up(n, 4), NaN beyond"""
    n32 = dp.rup(n, 4)
    M = np.full((M64.shape[0], n32 + 8), np.nan, np.float32)
    M[:, :n] = M64[:, :n].astype(np.float32)
    M[:, n:n32] = 0
    assert np.array_equal(M[:, :n].astype(F64), M64[:, :n])
    return M


def case(rng, rows, n, data, functor, hs=None):
    if functor == P.PASS_FN_LOGISTIC:
        hs = np.full(rows, dp.LOGISTIC)
    M64, vec, f = dp.iter_case(rng, F64, rows, n, data, functor, hs)
    if data != "int":
        M64[:, :n] = M64[:, :n].astype(np.float32).astype(F64)      # entries already representable in float
    return M64, to_f32_matrix(M64, n), vec, f


def params(data):
    return dict(rho=2.0, alpha=1.5, zs=0.5) if data == "int" else dict(rho=0.7, alpha=1.5, zs=1.3)


def run_pair(rng, rows, n, data, form=P.PASS_ITER_FULL, functor=P.PASS_FN_CHEAP, num_cu=1, force=None, alpha=None):
    """one case through both entries; the mixed output is held to the model, and on integers to the fp64 entry's bytes"""
    M64, M32, vec, f = case(rng, rows, n, data, functor)
    kw = params(data)
    if alpha is not None:
        kw["alpha"] = alpha
    lean, logistic, exact = form == P.PASS_ITER_LEAN, functor == P.PASS_FN_LOGISTIC, data == "int"
    ref = P.dense_pass_check(form, M64, n, vec, functor=functor, f=f, num_cu=num_cu, **kw)
    out = P.dense_pass_mixed_check(form, M32, n, vec, functor=functor, f=f, num_cu=num_cu, force=force, **kw)
    tag = ("mixed", rows, n, data, form, functor, num_cu, force)
    info = out["info"]
    assert info["kernel"] == P.PASS_KERNEL_MIXED and info["xl"] == 0 and info["windows"] == 1, tag
    # (the launch functions never start more workgroups than there are row blocks: stream_mixed.h, mixed_grid)
    assert info["grid"] == info["nparts"] <= -(-rows // info["rows_per_step"]), tag
    dp.check_iter(tag, F64, M64, n, rows, vec, f, out, functor, lean, kw["rho"], kw["alpha"], kw["zs"], 0.0, exact)
    if exact:
        for k in ROW_OUT:
            assert same_bytes(out[k], ref[k]), (tag, k)
        assert same_bytes(out["scalars"][:3], ref["scalars"][:3]), tag
        if not logistic:
            assert same_bytes(out["scalars"], ref["scalars"]), tag
            assert same_bytes(out["tot0"], ref["tot0"]) and same_bytes(out["tot1"], ref["tot1"]), tag
    return out, ref


def row_counts(R):
    return sorted({r for r in (1, R - 1, R, R + 1, 3 * R + 1) if r >= 1})


def rows_per_step(n, form, functor, num_cu=1, force=None):
    rng = np.random.default_rng(0)
    return run_pair(rng, 40, n, "int", form, functor, num_cu, force)[0]["info"]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7, 8, 130, 1030])
def test_exact_integers_bit_for_bit_with_the_fp64_entry(n):
    """n with n_pad % 4 == 2 (1, 2, 5, 6, 130, 1030) and without; rows in {1, R - 1, R, R + 1, 3 R + 1} for the shape's R
    of each form; both forms, both functors; num_cu = 1, so 3 R + 1 rows wrap round the grid wherever the form runs fewer
    than four workgroups per CU, and 3 (a grid that is no multiple of 8) once per form"""
    rng = np.random.default_rng(1000 + n)
    for form in (P.PASS_ITER_FULL, P.PASS_ITER_LEAN):
        for functor in (P.PASS_FN_CHEAP, P.PASS_FN_LOGISTIC):
            info = rows_per_step(n, form, functor)
            want = (64, 1) if n <= 256 else (256, 2)
            assert (info["tpb"], info["nv"]) == want
            for rows in row_counts(info["rows_per_step"]):
                run_pair(rng, rows, n, "int", form, functor, alpha=1.0 if functor == P.PASS_FN_LOGISTIC else None)
        run_pair(rng, 7 * info["rows_per_step"] + 1, n, "int", form, P.PASS_FN_CHEAP, num_cu=3)


@pytest.mark.parametrize("plan", MIXED_PLANS, ids=lambda p: "%dx%d" % p)
def test_every_mixed_shape_forced_at_its_first_and_full_width(plan):
    """every one-pass shape of the mixed plan through force_tpb / force_nv: at the first width that needs it, at its full
    width and two columns short of it (n_pad % 4 == 2 in the LAST thread's last vector); integers, both forms, rows
    3 R + 1 and R - 1; the natural choice at those widths is the shape itself"""
    tpb, nv = plan
    cap = tpb * nv
    prev = max([c for c in MIXED_CAPS if c < cap], default=0)
    rng = np.random.default_rng(2000 + cap)
    for n in (prev * 4 + 1, cap * 4 - 2, cap * 4):
        for form in (P.PASS_ITER_FULL, P.PASS_ITER_LEAN):
            info = rows_per_step(n, form, P.PASS_FN_CHEAP, force=plan)
            assert (info["tpb"], info["nv"]) == plan
            assert rows_per_step(n, form, P.PASS_FN_CHEAP)["tpb"] == tpb       # (the natural plan agrees)
            R = info["rows_per_step"]
            for rows in {3 * R + 1, max(1, R - 1)}:
                run_pair(rng, rows, n, "int", form, P.PASS_FN_CHEAP, force=plan)
            run_pair(rng, 2 * R + 1, n, "int", form, P.PASS_FN_LOGISTIC, force=plan, alpha=1.0)
    # the shape forced onto rows far narrower than it: most lanes hold no column at all
    for n in (1, 6, 9):
        run_pair(rng, 5, n, "int", P.PASS_ITER_FULL, P.PASS_FN_CHEAP, force=plan)
        run_pair(rng, 5, n, "int", P.PASS_ITER_LEAN, P.PASS_FN_LOGISTIC, force=plan, alpha=1.0)


def cols_vectors(rng, n, data):
    V = 2
    if data == "int":
        x_cur, xt = dp.ints(rng, n, F64), dp.ints(rng, n, F64)
        g = dp.fn_arrays(F64, n, dp.rup(n, V) + 3, rng.choice(dp.EXACT_FNS, n))
    else:
        x_cur, xt = rng.normal(0, 3.0, n), rng.normal(0, 0.3, n)
        g = dp.fn_arrays(F64, n, dp.rup(n, V) + 3, rng.integers(0, 16, n), rng)
    extra = dict(x_cur=dp.colv(F64, n, x_cur), xt=dp.colv(F64, n, xt), x12=dp.colv(F64, n), xtemp=dp.colv(F64, n),
                 rhs=dp.colv(F64, n))
    return extra, g


@pytest.mark.parametrize("n", [6, 130, 1030])
def test_second_stages_bit_for_bit_on_integers(n):
    """cols PRE, PRE_ONE and PACK behind the mixed pass (PACK not with ITER_LEAN, PRE not either: a lean pass forms one
    partial set): x12, xtemp, rhs, the four column scalars and the packed buffer equal the fp64 entry's bytes"""
    rng = np.random.default_rng(3000 + n)
    n_pad = dp.rup(n, 2)
    kw = dict(rho=2.0, alpha=1.5, zs=0.5, num_cu=1)
    for form, colss in ((P.PASS_ITER_FULL, (P.PASS_COLS_PRE, P.PASS_COLS_PRE_ONE, P.PASS_COLS_PACK)),
                        (P.PASS_ITER_LEAN, (P.PASS_COLS_PRE_ONE,))):
        for functor in (P.PASS_FN_CHEAP, P.PASS_FN_LOGISTIC):
            R = rows_per_step(n, form, functor)["rows_per_step"]
            rows = 3 * R + 1
            M64, M32, vec, f = case(rng, rows, n, "int", functor)
            extra, g = cols_vectors(rng, n, "int")
            for cols in colss:
                v = {k: w for k, w in vec.items() if k not in ("tot0", "tot1")}
                if cols == P.PASS_COLS_PACK:
                    v["pack"] = np.full(2 * n_pad + 6, dp.SENT)
                else:
                    v.update(extra)
                ref = P.dense_pass_check(form, M64, n, v, functor=functor, cols=cols, f=f, g=g, **kw)
                out = P.dense_pass_mixed_check(form, M32, n, v, functor=functor, cols=cols, f=f, g=g, **kw)
                tag = (n, form, functor, cols)
                for k in ROW_OUT:
                    assert same_bytes(out[k], ref[k]), (tag, k)
                if functor == P.PASS_FN_LOGISTIC:
                    # the totals are sums of inexact terms in another grouping: the exact parts only
                    assert same_bytes(out["scalars"][:3], ref["scalars"][:3]), tag
                    if cols != P.PASS_COLS_PACK:
                        assert same_bytes(out["x12"], ref["x12"]) and same_bytes(out["xtemp"], ref["xtemp"]), tag
                        assert same_bytes(out["col_scalars"][:3], ref["col_scalars"][:3]), tag
                        assert np.allclose(out["rhs"][:n], ref["rhs"][:n], rtol=1e-12, atol=1e-12), tag
                    continue
                assert same_bytes(out["scalars"], ref["scalars"]), tag
                if cols == P.PASS_COLS_PACK:
                    assert same_bytes(out["pack"], ref["pack"]), tag
                    assert np.array_equal(out["pack"][2 * n_pad:], out["scalars"]), tag
                else:
                    for k in ("x12", "xtemp", "rhs"):
                        assert same_bytes(out[k], ref[k]), (tag, k)
                    assert same_bytes(out["col_scalars"], ref["col_scalars"]), tag


@pytest.mark.parametrize("n", [5, 130, 1030, 256 * 10 * 4 - 2])
def test_real_data_within_the_gamma_bounds(n):
    """badly scaled rows and columns (2^-10 .. 2^10 each), entries rounded to float first: the model's bounds, every
    cheap function, the logistic functor, both forms; rows = 2 grid R + R + 1 with num_cu = 3"""
    rng = np.random.default_rng(4000 + n)
    for form in (P.PASS_ITER_FULL, P.PASS_ITER_LEAN):
        info = rows_per_step(n, form, P.PASS_FN_CHEAP, num_cu=3)
        R = info["rows_per_step"]
        rows = min(2 * info["grid"] * R + R + 1, 40) if n > 5000 else 2 * 3 * 8 * R + R + 1
        M64, M32, vec, f = case(rng, rows, n, "real", P.PASS_FN_CHEAP, hs=np.resize(np.asarray(dp.CHEAP_FNS), rows))
        kw = params("real")
        out = P.dense_pass_mixed_check(form, M32, n, vec, f=f, num_cu=3, **kw)
        dp.check_iter(("mixed real", n, form), F64, M64, n, rows, vec, f, out, P.PASS_FN_CHEAP, form == P.PASS_ITER_LEAN,
                      kw["rho"], kw["alpha"], kw["zs"], 0.0, False)
        run_pair(rng, rows, n, "real", form, P.PASS_FN_LOGISTIC, num_cu=3, alpha=1.0)


def test_two_runs_of_one_call_return_identical_bytes():
    rng = np.random.default_rng(5)
    rows, n = 301, 1030
    for form in (P.PASS_ITER_FULL, P.PASS_ITER_LEAN):
        M64, M32, vec, f = case(rng, rows, n, "real", P.PASS_FN_CHEAP)
        runs = [P.dense_pass_mixed_check(form, M32, n, vec, f=f, num_cu=0, **params("real")) for _ in range(2)]
        for k in ROW_OUT + ("tot0", "tot1", "scalars"):
            assert same_bytes(runs[0][k], runs[1][k]), (form, k)
        assert runs[0]["info"] == runs[1]["info"]


def test_zz_report():
    """prints the largest error-to-bound ratio per check (profiles/mixed_pass_accuracy.txt is this table)"""
    for (what, dt), r in sorted(RATIOS.items()):
        print("RATIO %-34s %-8s %.3e" % (what, dt, r))
    assert RATIOS and all(r <= 1.0 for r in RATIOS.values())
