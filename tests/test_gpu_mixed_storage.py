"""GPU tests of mixed-storage handles (pogs_amd.Solver(A, dtype=np.float64, storage=np.float32); include/pogs_amd.h:
POGS_AMD_STORE_F32): an fp64 handle whose equilibrated matrix is rounded to float, with the one-pass iteration reading
the float copy.  Matrices are float64 random and NOT representable in float; lasso and logistic are the two families
the one-pass iteration serves, Huber runs the two-pass fallback.

What is held to what:
  * the stored matrix: every entry survives float32 and is within 2^-24 relative of the plain fp64 handle's; d, e are
    the plain handle's, the norm estimate within 1e-6;
  * a fixed trajectory (adaptive_rho off, tolerances 0, 60 iterations -- no decision can flip):
      (a) POGS_AMD_MIXED_PASS=0 against 1 on the same rounded matrix: only summation orders differ, so the distance is
          held to 10 x the distance between the plain fp64 handle and the fp64 oracle (summation orders as well), measured
          in the same test, not below 1e-15;
      (b) the mixed handle against the plain fp64 handle: held to 10 x the distance, on the CPU oracle, between the
          problem of A and the problem of A rounded to float (the factor 10: the handle rounds the equilibrated entries,
          the yardstick the raw ones -- the same 2^-24 relative bound, other individual errors);
    both distances and the yardsticks are printed (profiles/mixed_storage_accuracy.txt is that table);
  * converged solves (default tolerances, adaptive rho): against the fp64 oracle on the ORIGINAL matrix by the bounds
    tests/test_gpu_dense.py applies to an fp32 handle (_check_solution, tight=False): a mixed handle is at least that
    accurate;
  * every path that never touches the float copy -- warm start, solve_batch, mul, project -- bit for bit against the same
    handle created with POGS_AMD_MIXED_PASS=0."""
import numpy as np
import pytest

import oracle_binding as ob
import test_gpu_dense as gd
from helpers import PROBLEMS, relerr, same_bytes, soa

pytestmark = pytest.mark.gpu

SHAPES = [(203, 102), (200, 100), (1500, 1030)]
FUSED = ["lasso", "logistic"]
FIXED = dict(abs_tol=0.0, rel_tol=0.0, max_iter=60, adaptive_rho=False)
LINES = []     # the accuracy table (test_zz_report)


def _pogs():
    import pogs_amd

    return pogs_amd


def problem(shape, family, seed=7, logistic_weight=None):
    m, n = shape
    rng = np.random.default_rng(seed + m + n)
    A = rng.standard_normal((m, n))
    b = A @ (rng.standard_normal(n) * (rng.random(n) < 0.2)) + 0.1 * rng.standard_normal(m)
    if logistic_weight is None:
        f, g = PROBLEMS[family](b, n)
    else:
        f, g = _pogs().graph.logistic_functions(np.sign(b) + (b == 0), logistic_weight, n)
    assert not np.array_equal(A.astype(np.float32).astype(np.float64), A)
    return A, f, g


def mixed_solver(A, monkeypatch, switch=None, **kw):
    """a mixed handle; switch "0" / "1": POGS_AMD_MIXED_PASS as read at create, None: unset (the default, on)"""
    if switch is None:
        monkeypatch.delenv("POGS_AMD_MIXED_PASS", raising=False)
    else:
        monkeypatch.setenv("POGS_AMD_MIXED_PASS", switch)
    return _pogs().Solver(A, dtype=np.float64, storage=np.float32, **kw)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_stored_matrix_is_the_rounded_equilibrated_matrix(shape, monkeypatch):
    A, _, _ = problem(shape, "lasso")
    with mixed_solver(A, monkeypatch) as s:
        assert s.storage == _pogs().STORE_F32
        Am, dm, em, nm = s.equilibrated()
    with _pogs().Solver(A, dtype=np.float64) as s:
        assert s.storage == _pogs().STORE_SAME
        Ap, dp_, ep, npl = s.equilibrated()
    assert np.array_equal(Am.astype(np.float32).astype(np.float64), Am)
    assert not np.array_equal(Ap.astype(np.float32).astype(np.float64), Ap)
    assert np.all(np.abs(Am - Ap) <= 2.0 ** -24 * np.abs(Ap))
    assert np.array_equal(Am, Ap.astype(np.float32).astype(np.float64))       # to nearest: numpy's rounding
    assert same_bytes(dm, dp_) and same_bytes(em, ep)
    assert nm == pytest.approx(npl, rel=1e-6)


@pytest.mark.parametrize("family", FUSED)
@pytest.mark.parametrize("shape", SHAPES)
def test_fixed_trajectory_against_the_switch_and_against_the_plain_handle(shape, family, monkeypatch):
    A, f, g = problem(shape, family)
    # the yardstick of (b), on the CPU: the problem of A against the problem of A rounded to float, same 60 iterations
    A32 = A.astype(np.float32).astype(np.float64)
    o_full = ob.oracle_solve(A, soa(f), soa(g), dtype=np.float64, **FIXED)
    o_round = ob.oracle_solve(A32, soa(f), soa(g), dtype=np.float64, **FIXED)
    assert o_full["status"] == o_round["status"] and o_full["iterations"] == o_round["iterations"]
    yard = relerr(o_round["x"], o_full["x"])
    assert yard > 0
    with _pogs().Solver(A, dtype=np.float64) as s:
        plain = s.solve(f, g, **FIXED)
    with mixed_solver(A, monkeypatch, "0") as s:
        off = s.solve(f, g, **FIXED)
    with mixed_solver(A, monkeypatch, "1") as s:
        on = s.solve(f, g, **FIXED)
    assert plain["iterations"] == off["iterations"] == on["iterations"] == o_full["iterations"]
    d_ref = relerr(plain["x"], o_full["x"])          # summation orders alone: the engine against the oracle
    d_switch = relerr(on["x"], off["x"])
    d_mixed = relerr(on["x"], plain["x"])
    line = "%-9s %5d x %-5d  engine-oracle %.3e  switch on-off %.3e  |  yardstick(A, float(A)) %.3e  mixed-plain %.3e" % (
        family, shape[0], shape[1], d_ref, d_switch, yard, d_mixed)
    print("ACCURACY " + line)
    LINES.append(line)
    assert d_switch <= max(10 * d_ref, 1e-15), line
    assert d_mixed <= 10 * yard, line
    assert relerr(on["y"], plain["y"]) <= 10 * max(yard, relerr(o_round["y"], o_full["y"])), line


def test_converged_solves_follow_the_oracle_on_the_original_matrix(monkeypatch):
    """default tolerances, adaptive rho: the lean -> exact -> full sequence and at least one missed rho prediction occur
    (asserted from stats), status 0, x, y, lambda, optval by the fp32 handle's bounds against the fp64 oracle on A"""
    seen_exact, seen_miss = 0, 0
    for shape in SHAPES:
        for family in FUSED + (["huber"] if shape == (200, 100) else []):
            A, f, g = problem(shape, family)
            if family == "logistic" and shape == (1500, 1030):
                # (PROBLEMS' weight 0.01 leaves the oracle at max_iter on this shape; 0.2 converges in ~490 iterations)
                A, f, g = problem(shape, family, logistic_weight=0.2)
            want = ob.oracle_solve(A, soa(f), soa(g), dtype=np.float64)
            assert want["status"] == 0
            with mixed_solver(A, monkeypatch) as s:
                got = s.solve(f, g)
                st = s.stats()
            with _pogs().Solver(A, dtype=np.float64) as s:
                plain = s.solve(f, g)
            print("ITERATIONS %-9s %5d x %-5d  mixed %d  plain fp64 %d  oracle %d  (exact %d, misses %d)" % (
                family, shape[0], shape[1], got["iterations"], plain["iterations"], want["iterations"], st["exact_iters"],
                st["spec_misses"]))
            assert got["status"] == 0
            gd._check_solution(A, f, g, got, want, np.float32, tight=False)
            if family in FUSED:
                seen_exact += int(st["exact_iters"] > 0)
                seen_miss += int(st["spec_misses"] > 0)
                assert st["spec_hits"] > 0
    assert seen_exact > 0 and seen_miss > 0


@pytest.mark.parametrize("family", FUSED)
def test_two_solves_on_one_handle_return_identical_bytes(family, monkeypatch):
    A, f, g = problem((1500, 1030), family, logistic_weight=0.2 if family == "logistic" else None)
    with mixed_solver(A, monkeypatch) as s:
        a, b = s.solve(f, g), s.solve(f, g)
    assert a["iterations"] == b["iterations"] and a["optval"] == b["optval"]
    for k in ("x", "y", "l"):
        assert same_bytes(a[k], b[k]), k


@pytest.mark.parametrize("shape", [(203, 102), (1500, 1030)])
def test_paths_that_never_read_the_float_copy_are_bit_for_bit_the_switched_off_handle(shape, monkeypatch):
    """mul, project, the factor, solve_batch of 3 (a warm-started batch too), and a warm start: (x0, l0) become (z, z~) by
    products with the fp64 copy; cut at max_iter = 1, everything the solve returns -- the prox point, the duals -- was
    formed before the iteration's one mixed launch, so x, y, l and optval show the warm start and nothing else"""
    m, n = shape
    A, f, g = problem(shape, "lasso")
    rng = np.random.default_rng(5)
    x0, y0, u = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    fs, gs = zip(*(PROBLEMS["lasso"](rng.standard_normal(m), n) for _ in range(3)))
    res = {}
    for switch in ("0", "1"):
        with mixed_solver(A, monkeypatch, switch) as s:
            r = dict(project=s.project(x0, y0), mul_n=s.mul("n", 1.5, x0, -0.5, y0), mul_t=s.mul("t", 0.7, u, 2.0, x0))
            r["batch"] = s.solve_batch(list(fs), list(gs), max_iter=40)
            r["batch"] += s.solve_batch(list(fs), list(gs), max_iter=10, x0=[0.1 * x0] * 3, l0=[0.1 * u] * 3)
            r["factor"] = s.factor()
            r["warm"] = s.solve(f, g, x0=0.1 * x0, l0=0.1 * u, max_iter=1)
            res[switch] = r
    off, on = res["0"], res["1"]
    for k in ("mul_n", "mul_t"):
        assert same_bytes(on[k], off[k]), k
    for a, b in zip(on["project"], off["project"]):
        assert same_bytes(a, b)
    for a, b in zip(on["factor"], off["factor"]):
        assert same_bytes(a, b)
    for a, b in zip(on["batch"], off["batch"]):
        assert a["iterations"] == b["iterations"] and a["status"] == b["status"]
        for k in ("x", "y", "l"):
            assert same_bytes(a[k], b[k]), ("batch", k)
    assert on["warm"]["optval"] == off["warm"]["optval"] and np.any(on["warm"]["x"] != 0)
    for k in ("x", "y", "l"):
        assert same_bytes(on["warm"][k], off["warm"][k]), ("warm", k)


def test_stream_bytes_count_a_mixed_launch_as_four_bytes_per_entry(monkeypatch):
    m, n = 1500, 1030
    A, f, g = problem((m, n), "lasso")
    with mixed_solver(A, monkeypatch, "1", profile=True) as s:
        # a fixed run: the first iteration adds the unspeculated column-sum pass over the fp64 copy, every later
        # launch is the mixed pass
        s.begin_run(f, g, abs_tol=0.0, rel_tol=0.0, max_iter=100000, adaptive_rho=False)
        s.iterate(1)
        st = s.stats()
        assert st["stream_launches"] == 2 and st["stream_bytes"] == m * n * (8 + 4)
        s.reset_stats()
        s.iterate(20)
        st = s.stats()
        assert st["stream_launches"] == 20 and st["stream_bytes"] / st["stream_launches"] == m * n * 4
        assert st["spec_hits"] == 20 and st["spec_misses"] == 0
        # a lasso solve with nothing to decide: one fp64 pass, then mixed passes only
        s.reset_stats()
        r = s.solve(f, g, **FIXED)
        st = s.stats()
        assert st["stream_launches"] == st["iterations"] + 1 and st["iterations"] >= r["iterations"] >= 59
        assert st["stream_bytes"] == m * n * 4 * (st["stream_launches"] - 1) + m * n * 8
        assert st["stream_bytes"] / st["stream_launches"] < m * n * 4 * 1.02
    with mixed_solver(A, monkeypatch, "0", profile=True) as s:
        s.solve(f, g, **FIXED)
        st = s.stats()
        assert st["stream_bytes"] == m * n * 8 * st["stream_launches"]


def test_zz_report():
    """prints the table of profiles/mixed_storage_accuracy.txt"""
    for line in LINES:
        print("ACCURACY " + line)
    assert LINES
