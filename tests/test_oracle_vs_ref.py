"""CPU tests: the oracle against the compiled reference (oracle/_ref/libpogs_cpu.so) on a few more random
problems than reference_outputs.npz holds, so the restatement is pinned beyond those fixtures.  The
reference's solutions of exactly these problems are stored in tests/golden/oracle_vs_ref.npz
(tests/golden/make_oracle_vs_ref.py runs the reference on CASES below); the problems are regenerated
from their seeds."""
import functools
import os

import numpy as np
import pytest

import oracle_binding as ob
from helpers import relerr, soa
from pogs_amd import graph as G
from pogs_amd import synth

# name -> (generator, (m, n, seed[, nnz per row]), dtype, keyword arguments of the solve)
CASES = {
    "dense_f64": ("dense", (1500, 400, 21), np.float64, {}),
    "dense_f32": ("dense", (1500, 400, 21), np.float32, {}),
    "no_gap_stop": ("dense", (600, 200, 22), np.float64, {"gap_stop": False}),
    "no_adaptive_rho": ("dense", (600, 200, 22), np.float64, {"adaptive_rho": False, "max_iter": 400}),
    "rho5": ("dense", (600, 200, 22), np.float64, {"rho": 5.0}),
    "rel_tol": ("dense", (600, 200, 22), np.float64, {"rel_tol": 1e-6}),
    "column_major": ("dense", (500, 120, 23), np.float64, {"order": 0}),
    "sparse": ("csr", (5000, 1200, 24, 25), np.float64, {}),
}
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "oracle_vs_ref.npz")


def problem(name):
    """(A, f, g, dtype, solve keyword arguments) of CASES[name]: a lasso with lambda = 0.1."""
    kind, shape, dtype, kw = CASES[name]
    if kind == "csr":
        m, n, seed, nnz = shape
        A, b, _ = synth.csr_lasso(m, n, nnz, seed=seed, dtype=dtype)
    else:
        m, n, seed = shape
        A, b, _ = synth.dense_lasso(m, n, seed=seed, dtype=dtype)
    f, g = G.lasso_functions(b, 0.1, n)
    return A, f, g, dtype, kw


@functools.lru_cache(maxsize=None)
def _fixture():
    return dict(np.load(FIXTURE))


def _ref(name):
    """The compiled reference's solution of CASES[name]."""
    z = _fixture()
    return {"x": z[name + "_x"], "optval": float(z[name + "_optval"]), "iterations": int(z[name + "_iterations"]),
            "status": int(z[name + "_status"])}


def _oracle(name):
    A, f, g, dtype, kw = problem(name)
    return ob.oracle_solve(A, soa(f), soa(g), dtype=dtype, **kw)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-9), (np.float32, 1e-4)])
def test_dense_lasso_live(dtype, tol):
    name = "dense_f64" if dtype == np.float64 else "dense_f32"
    want = _ref(name)
    got = _oracle(name)
    assert got["status"] == want["status"] == 0
    assert abs(got["iterations"] - want["iterations"]) <= (0 if dtype == np.float64 else 5)
    assert relerr(got["x"], want["x"]) < tol
    assert got["optval"] == pytest.approx(want["optval"], rel=max(tol, 1e-9))


def test_dense_no_gap_stop_no_adaptive_rho_live():
    for name in ("no_gap_stop", "no_adaptive_rho", "rho5", "rel_tol"):
        want = _ref(name)
        got = _oracle(name)
        assert got["status"] == want["status"], name
        assert got["iterations"] == want["iterations"], name
        assert relerr(got["x"], want["x"]) < 1e-8, name


def test_column_major_live():
    want = _ref("column_major")
    got = _oracle("column_major")
    assert got["iterations"] == want["iterations"]
    assert relerr(got["x"], want["x"]) < 1e-9


def test_sparse_live():
    want = _ref("sparse")
    got = _oracle("sparse")
    assert got["status"] == want["status"] == 0
    assert abs(got["iterations"] - want["iterations"]) <= 1
    assert relerr(got["x"], want["x"]) < 1e-7
