"""GPU tests of mixed-storage SPARSE handles (pogs_amd.Solver(A_sparse, dtype=np.float64, values=np.float32); include/
pogs_amd.h: PogsAmdCreateSparseMixed): an fp64 handle whose equilibrated non-zeros are rounded to float and whose tiled
copies store them as floats.  Matrices come from synth.csr_lasso in float64 and are NOT representable in float:

    tall     3000 x 800, 20 per row
    wide     800 x 3000, 20 per row
    blocks   2000 x 12400, 10 per row: two column blocks for A (fp64 tiles are 12288 columns wide)

What is held to what:
  * the stored matrix: PogsAmdGetEquil returns float32(plain handle's values) exactly; d, e are the plain handle's
    bytes, the norm estimate within 1e-6;
  * the switch: a float converts to double exactly and the tile plan fixes the order of every sum, so the handle must
    return the BYTES of the same handle created with POGS_AMD_MIXED_PASS=0 (rounded values kept as doubles, the
    existing kernel): iterations, optval, x, y, lambda, cg_iters, matvecs of converged solves (default tolerances,
    adaptive rho) and of a warm-started one, lasso and logistic, CGLS and DIRECT, tall and wide, CSR input and the
    device-CSR tuple; solve_batch of 3, mul, project, PogsAmdSparseCgCheck (loop 0); two solves on one handle;
  * against the plain fp64 handle, on a fixed trajectory (DIRECT, adaptive_rho off, tolerances 0, 60 iterations -- no
    decision can flip): relerr(x_mixed, x_plain) <= 10 x the distance, on the CPU oracle with the same settings,
    between the problem of A and the problem of A rounded to float (the factor 10: the handle rounds the equilibrated
    entries, the yardstick the raw ones -- tests/test_gpu_mixed_storage.py); the lines are
    profiles/sparse_mixed_accuracy.txt;
  * converged solves against the fp64 oracle on the ORIGINAL matrix by the bounds tests/test_gpu_sparse.py applies to an
    fp32 handle (x, y within 2e-5, iterations within max(5, 10 %)): a mixed handle is at least that accurate;
  * accounting: stream_bytes per launch by the formula with 4-byte values (8 switched off); the pool holds less with
    the mixed handle alive than with the switched-off one;
  * a copy that is not tiled (POGS_AMD_SPMV=plain) solves and matches the switched-off handle's bytes.

Logistic: weight 0.2 (helpers.PROBLEMS' 0.01 leaves the oracle at max_iter on the tall matrix)."""
import ctypes

import numpy as np
import pytest

import oracle_binding as ob
from helpers import relerr, same_bytes, soa

pytestmark = pytest.mark.gpu

MATS = {"tall": (3000, 800, 20, 41), "wide": (800, 3000, 20, 42), "blocks": (2000, 12400, 10, 43)}
FAMILIES = ["lasso", "logistic"]
FIXED = dict(abs_tol=0.0, rel_tol=0.0, max_iter=60, adaptive_rho=False)
LINES = []      # the accuracy table (test_zz_report)
_CACHE = {}


def _pogs():
    import pogs_amd

    return pogs_amd


def _proj(name):
    from pogs_amd import _lib

    return dict(cgls=_lib.PROJ_CGLS, direct=_lib.PROJ_DIRECT)[name]


def matrix(name):
    """(A, b) of MATS[name], made once; the values are not representable in float"""
    if ("A", name) not in _CACHE:
        from pogs_amd import synth

        m, n, per_row, seed = MATS[name]
        A, b, _ = synth.csr_lasso(m, n, per_row, seed=seed, dtype=np.float64)
        assert not np.array_equal(A.data.astype(np.float32).astype(np.float64), A.data)
        _CACHE["A", name] = (A, b)
    return _CACHE["A", name]


def problem(name, family):
    A, b = matrix(name)
    G = _pogs().graph
    n = A.shape[1]
    f, g = G.lasso_functions(b, 0.1, n) if family == "lasso" else G.logistic_functions(np.sign(b) + (b == 0), 0.2, n)
    return A, f, g


def oracle(name, family, rounded=False, **kw):
    """the CPU oracle's dense (direct) solve of the problem, or of the problem of float32(A); computed once, never changed"""
    key = ("o", name, family, rounded, tuple(sorted(kw.items())))
    if key not in _CACHE:
        A, f, g = problem(name, family)
        D = (A.astype(np.float32).astype(np.float64) if rounded else A).toarray()
        _CACHE[key] = ob.oracle_solve(D, soa(f), soa(g), dtype=np.float64, **kw)
    return _CACHE[key]


def mixed_solver(A, monkeypatch, switch=None, device=False, **kw):
    """a mixed handle; switch "0" / "1": POGS_AMD_MIXED_PASS as read at create, None: unset (the default, on);
    device: the matrix handed over as the device-CSR tuple"""
    if switch is None:
        monkeypatch.delenv("POGS_AMD_MIXED_PASS", raising=False)
    else:
        monkeypatch.setenv("POGS_AMD_MIXED_PASS", switch)
    if not device:
        return _pogs().Solver(A, dtype=np.float64, values=np.float32, **kw)
    import torch

    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev) for a, dt in
         ((A.data, np.float64), (A.indptr, np.int32), (A.indices, np.int32))]
    s = _pogs().Solver((t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), A.nnz), dtype=np.float64, shape=A.shape,
                       device_ptr=True, values=np.float32, **kw)
    torch.cuda.synchronize()
    del t   # (inputs are copied at create)
    return s


def equil(s, nnz):
    from pogs_amd import _lib

    v, d, e, nrm = np.zeros(nnz), np.zeros(s.m), np.zeros(s.n), ctypes.c_double()
    assert _lib.lib.PogsAmdGetEquil(s._h, v.ctypes.data, d.ctypes.data, e.ctypes.data, ctypes.byref(nrm)) == 0
    return v, d, e, nrm.value


def assert_same_solve(a, b, where):
    assert a["status"] == b["status"] and a["iterations"] == b["iterations"], (where, a["iterations"], b["iterations"])
    assert a["optval"] == b["optval"], (where, a["optval"], b["optval"])
    for k in ("x", "y", "l"):
        assert same_bytes(a[k], b[k]), (where, k, relerr(a[k], b[k]))


@pytest.mark.parametrize("name", sorted(MATS))
def test_the_stored_matrix_is_the_rounded_equilibrated_matrix(name, monkeypatch):
    A, _ = matrix(name)
    pogs = _pogs()
    with pogs.Solver(A, dtype=np.float64) as s:
        assert s.storage == pogs.STORE_SAME
        vp, dp_, ep, nrm_p = equil(s, A.nnz)
    assert not np.array_equal(vp.astype(np.float32).astype(np.float64), vp)
    for switch in ("1", "0"):
        with mixed_solver(A, monkeypatch, switch) as s:
            assert s.storage == pogs.STORE_F32 and s.sparse
            vm, dm, em, nrm_m = equil(s, A.nnz)
        assert np.array_equal(vm.astype(np.float32).astype(np.float64), vm)      # survives float32
        assert np.array_equal(vm, vp.astype(np.float32).astype(np.float64))       # to nearest: numpy's rounding
        assert same_bytes(dm, dp_) and same_bytes(em, ep)
        assert nrm_m == pytest.approx(nrm_p, rel=1e-6)


SWITCH_CASES = [(n, f, p) for n in ("tall", "wide") for f in FAMILIES for p in ("cgls", "direct")] + \
               [("blocks", "lasso", "cgls"), ("blocks", "lasso", "direct")]


@pytest.mark.parametrize("name,family,projector", SWITCH_CASES)
def test_the_handle_returns_the_bytes_of_the_switched_off_handle(name, family, projector, monkeypatch):
    """converged solves (default tolerances, adaptive rho), a warm-started one, a repeated one; CSR input and the
    device-CSR tuple.  (The wide two-block matrix does not converge within max_iter at this lambda: its runs are cut
    at 150 iterations and compared all the same -- it is there for the second column block, not for the solve.)"""
    A, f, g = problem(name, family)
    kw = dict(max_iter=150) if name == "blocks" else {}
    res = {}
    for switch, device in (("0", False), ("1", False), ("1", True)):
        with mixed_solver(A, monkeypatch, switch, device=device, projector=_proj(projector)) as s:
            cold = s.solve(f, g, **kw)
            st = s.stats()
            again = s.solve(f, g, **kw)
            warm = s.solve(f, g, x0=0.5 * cold["x"], l0=0.5 * cold["l"], **kw)
            res[switch, device] = (cold, again, warm, st, s.stats())
    off = res["0", False]
    assert (off[0]["status"] == 0 or name == "blocks") and off[0]["iterations"] > 20
    assert (off[3]["cg_iters"] > 0) == (projector == "cgls") and off[3]["matvecs"] > 0
    for key in (("1", False), ("1", True)):
        on = res[key]
        for i, what in enumerate(("cold", "again", "warm")):
            assert_same_solve(on[i], off[i], (name, family, projector, key, what))
        assert_same_solve(on[1], on[0], (name, family, projector, key, "two solves on one handle"))
        for st_on, st_off in ((on[3], off[3]), (on[4], off[4])):
            assert st_on["cg_iters"] == st_off["cg_iters"] and st_on["matvecs"] == st_off["matvecs"]
            assert st_on["iterations"] == st_off["iterations"]


@pytest.mark.parametrize("name,projector", [("tall", "cgls"), ("wide", "cgls"), ("blocks", "cgls"), ("tall", "direct"),
                                            ("wide", "direct")])
def test_batch_mul_project_and_the_cg_check_are_bit_for_bit_the_switched_off_handle(name, projector, monkeypatch):
    from pogs_amd import _lib

    A, f, g = problem(name, "lasso")
    m, n = A.shape
    G = _pogs().graph
    rng = np.random.default_rng(5)
    x0, y0, u = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    fs, gs = zip(*(G.lasso_functions(rng.standard_normal(m), 0.1, n) for _ in range(3)))
    cg_in = [rng.standard_normal(k) for k in (n, m, n, m, n, n, m)]   # x0, y0, x_warm, y_warm, x_prev, x12, y12
    res = {}
    for switch in ("0", "1"):
        with mixed_solver(A, monkeypatch, switch, projector=_proj(projector)) as s:
            r = dict(project=s.project(x0, y0), mul_n=s.mul("n", 1.5, x0, -0.5, y0), mul_t=s.mul("t", 0.7, u, 2.0, x0))
            r["batch"] = s.solve_batch(list(fs), list(gs), max_iter=60)
            if projector == "cgls":
                r["cg"] = _lib.sparse_cg_check(s._h, *cg_in, 1e-9, max_steps=40, ahead=2, loop=_lib.CG_FUSED)
            r["after"] = s.solve(f, g, max_iter=30)
            res[switch] = r
    off, on = res["0"], res["1"]
    for k in ("mul_n", "mul_t"):
        assert same_bytes(on[k], off[k]) and np.any(on[k] != 0), k
    for a, b in zip(on["project"], off["project"]):
        assert same_bytes(a, b) and np.any(a != 0)
    assert len(on["batch"]) == 3
    for a, b in zip(on["batch"], off["batch"]):
        assert_same_solve(a, b, "batch")
    if projector == "cgls":
        a, b = on["cg"], off["cg"]
        assert a["steps"] == b["steps"] > 0 and a["enqueued"] == b["enqueued"] and a["info"] == b["info"]
        assert all(i["tiled"] == 1 for i in a["info"])
        for k in ("x", "y_new", "xtemp", "ytemp", "r", "p", "s", "rec_x"):
            assert same_bytes(a[k], b[k]), ("cg check", k)
        for k in _lib.CG_SLOTS:
            assert same_bytes(np.float64(a[k]), np.float64(b[k])), ("cg check", k)
    assert_same_solve(on["after"], off["after"], "solve after the diagnostics")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", ["tall", "wide"])
def test_fixed_trajectory_against_the_plain_handle(name, family, monkeypatch):
    A, f, g = problem(name, family)
    o_full, o_round = oracle(name, family, **FIXED), oracle(name, family, rounded=True, **FIXED)
    assert o_full["status"] == o_round["status"] and o_full["iterations"] == o_round["iterations"]
    yard = relerr(o_round["x"], o_full["x"])
    assert yard > 0
    direct = _proj("direct")
    with _pogs().Solver(A, dtype=np.float64, projector=direct) as s:
        plain = s.solve(f, g, **FIXED)
    with mixed_solver(A, monkeypatch, projector=direct) as s:
        on = s.solve(f, g, **FIXED)
    assert plain["iterations"] == on["iterations"] == o_full["iterations"]
    d_ref, d_mixed = relerr(plain["x"], o_full["x"]), relerr(on["x"], plain["x"])
    line = "%-9s %-6s %5d x %-5d  engine-oracle %.3e  |  yardstick(A, float(A)) %.3e  mixed-plain %.3e" % (
        family, name, A.shape[0], A.shape[1], d_ref, yard, d_mixed)
    print("ACCURACY " + line)
    LINES.append(line)
    assert d_mixed <= 10 * yard, line
    assert d_mixed > 0, line   # (the handle did round: it is not the plain handle)


@pytest.mark.parametrize("name,family,projector", [("tall", f, p) for f in FAMILIES for p in ("cgls", "direct")] +
                         [("wide", "lasso", "cgls"), ("wide", "lasso", "direct")])
def test_converged_solves_follow_the_oracle_on_the_original_matrix(name, family, projector, monkeypatch):
    """status 0; x, y within 2e-5 and the iterations within max(5, 10 %) of the fp64 oracle on A (its direct solve of
    the dense matrix for a DIRECT handle, its CGLS solve of the sparse one for a CGLS handle)"""
    A, f, g = problem(name, family)
    if projector == "direct":
        want = oracle(name, family)
    else:
        key = ("os", name, family)
        if key not in _CACHE:
            _CACHE[key] = ob.oracle_solve(A, soa(f), soa(g), dtype=np.float64)
        want = _CACHE[key]
    with mixed_solver(A, monkeypatch, projector=_proj(projector)) as s:
        got = s.solve(f, g)
    print("ITERATIONS %-9s %-6s %-6s mixed %d  oracle %d  x %.3e  y %.3e" % (
        family, name, projector, got["iterations"], want["iterations"], relerr(got["x"], want["x"]),
        relerr(got["y"], want["y"])))
    assert got["status"] == want["status"] == 0
    assert abs(got["iterations"] - want["iterations"]) <= max(5, int(0.1 * want["iterations"]))
    assert relerr(got["x"], want["x"]) < 2e-5
    assert relerr(got["y"], want["y"]) < 2e-5
    assert got["optval"] == pytest.approx(want["optval"], rel=2e-5)


def test_stream_bytes_count_a_mixed_product_with_four_byte_values(monkeypatch):
    """algorithmic bytes of one product (csrc/sparse.hip): nnz (s + 4) + 4 ((m + n) / 2 + 1) + 8 (m + n), s = 4 on the
    float tiled copies and 8 switched off"""
    A, f, g = problem("tall", "lasso")
    m, n = A.shape
    for switch, s_bytes in (("1", 4), ("0", 8)):
        with mixed_solver(A, monkeypatch, switch, profile=True) as s:
            s.solve(f, g, **FIXED)
            st = s.stats()
        assert st["stream_launches"] > 60
        assert st["stream_bytes"] / st["stream_launches"] == A.nnz * (s_bytes + 4) + 4.0 * (0.5 * (m + n) + 1) + 8.0 * (m + n)


def test_the_mixed_handle_holds_less_device_memory(monkeypatch):
    """4 bytes less per stored element on each tiled copy (nnz = 4e5, so each value array is past the pool's 2 MB size
    classes: 8 E bytes never round to what 4 E bytes round to)"""
    from pogs_amd import _lib, synth

    A, _, _ = synth.csr_lasso(20000, 4000, 20, seed=44, dtype=np.float64)
    assert A.nnz >= 2e5
    live = {}
    for switch in ("0", "1"):
        base = _lib.pool_stats()["live_bytes"]
        with mixed_solver(A, monkeypatch, switch):
            live[switch] = _lib.pool_stats()["live_bytes"] - base
    print("MEMORY nnz %d: live bytes switched off %d, mixed %d, difference %d (%.2f bytes per non-zero and copy)" % (
        A.nnz, live["0"], live["1"], live["0"] - live["1"], (live["0"] - live["1"]) / (2.0 * A.nnz)))
    assert live["1"] < live["0"]


def test_a_copy_that_is_not_tiled_still_solves_and_matches_the_switched_off_handle(monkeypatch):
    monkeypatch.setenv("POGS_AMD_SPMV", "plain")
    A, f, g = problem("tall", "lasso")
    res = {}
    for switch in ("0", "1"):
        with mixed_solver(A, monkeypatch, switch) as s:
            res[switch] = (s.solve(f, g), equil(s, A.nnz)[0])
    assert res["1"][0]["status"] == 0
    assert_same_solve(res["1"][0], res["0"][0], "plain kernel")
    assert same_bytes(res["1"][1], res["0"][1])
    assert np.array_equal(res["1"][1].astype(np.float32).astype(np.float64), res["1"][1])


def test_zz_report():
    """prints the table of profiles/sparse_mixed_accuracy.txt"""
    for line in LINES:
        print("ACCURACY " + line)
    assert LINES
