"""CPU tests of the warm-started batched solves (include/pogs_amd.h: PogsAmdSolveBatchWarmFn) and of the chained path
built on them: the header compiles as C99 with a call of the entry, the library exports it, the chain schedule covers
every problem once with its predecessor solved earlier, `Solver.solve_chain` hands each problem its predecessor's
(x, l, rho), and `Solver.solve_batch` refuses starts that do not fit before any library call."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from pogs_amd import _lib, graph

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

SNIPPET = r"""
#include "pogs_amd.h"
int call_warm(PogsAmdSolver *s, const PogsAmdFn *f, const PogsAmdFn *g, const double *x0, const double *l0, double *x,
              double *l, unsigned int *it, int *st, double *rho_final) {
  double rho[POGS_AMD_BATCH_MAX];
  int warm[POGS_AMD_BATCH_MAX];
  for (int j = 0; j < POGS_AMD_BATCH_MAX; ++j) { rho[j] = 1.0; warm[j] = j & 1; }
  return PogsAmdSolveBatchWarmFn(s, 2, f, g, rho, x0, l0, warm, 1e-4, 1e-4, 2500u, 0u, 1, 1, x, NULL, l, NULL, NULL, it,
                                 st, rho_final);
}
"""


def test_header_compiles_as_c99_with_a_warm_batch_call(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "batch_warm_call.c"
    src.write_text(SNIPPET)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_library_exports_the_warm_batch_entry():
    assert "PogsAmdSolveBatchWarmFn" in _lib.ABI_SYMBOLS
    fn = getattr(_lib.lib, "PogsAmdSolveBatchWarmFn")
    assert fn is not None and len(fn.argtypes) == 22


@pytest.mark.parametrize("slots", [1, 2, 16, None])
@pytest.mark.parametrize("P", [0, 1, 5, 16, 17, 20, 100])
def test_chain_schedule(P, slots):
    rounds = graph._chain_schedule(P, slots)
    cap = min(_lib.BATCH_MAX, slots or _lib.BATCH_MAX)
    L = -(-P // cap) if P else 0
    seen = {}
    for r, rnd in enumerate(rounds):
        assert 1 <= len(rnd) <= cap
        for j, pred in rnd:
            assert j not in seen
            seen[j] = r
            if pred is None:
                assert j % L == 0                       # the first element of its segment
            else:
                assert pred == j - 1
                assert pred // L == j // L              # the same segment
                assert seen[pred] < r                   # solved in an earlier round
    assert sorted(seen) == list(range(P))               # every index exactly once
    assert len(rounds) == L
    for j in range(P):
        assert seen[j] == j % L                         # round r holds element r of every segment
    if P and P <= cap:
        assert len(rounds) == 1 and all(pred is None for _, pred in rounds[0])


def _fake_solver(m, n):
    # a handle-less Solver: enough for the argument checks, which come before any library call
    s = object.__new__(graph.Solver)
    s._h = ctypes.c_void_p()
    s.m, s.n, s.dtype, s.sparse = m, n, np.float64, False
    return s


def _run_fake_chain(monkeypatch, P, slots, status_of, rho=0.7):
    """solve_chain with solve_batch replaced: problem j (recognised by its lambda) returns x = j + 1, l = -(j + 1),
    rho = 10 + j and status_of(j).  Returns (results, calls): a call is a list of (problem, x0, l0, warm, rho)."""
    m, n = 6, 4
    calls = []

    def fake(self, fs, gs, rho=1.0, x0=None, l0=None, warm=None, return_rho=False, **kw):
        assert return_rho
        k = len(fs)
        assert len(gs) == k and len(rho) == k and k <= min(_lib.BATCH_MAX, slots or _lib.BATCH_MAX)
        js = [int(round(float(np.ravel(g.c)[0]))) for g in gs]
        x0 = x0 if x0 is not None else [None] * k
        l0 = l0 if l0 is not None else [None] * k
        warm = warm if warm is not None else [x is not None for x in x0]
        calls.append([(js[q], x0[q], l0[q], bool(warm[q]), rho[q]) for q in range(k)])
        return [{"x": np.full(n, j + 1.0), "y": np.zeros(m), "l": np.full(m, -(j + 1.0)), "mu": np.zeros(n),
                 "optval": 0.0, "iterations": 3, "status": status_of(j), "rho": 10.0 + j} for j in js]

    monkeypatch.setattr(graph.Solver, "solve_batch", fake)
    s = _fake_solver(m, n)
    pairs = [graph.lasso_functions(np.ones(m), float(j), n) for j in range(P)]
    res = s.solve_chain([p[0] for p in pairs], [p[1] for p in pairs], rho=rho, slots=slots)
    return res, calls


@pytest.mark.parametrize("P,slots", [(6, 2), (5, 2), (20, None), (7, 16), (9, 1)])
def test_chain_hands_each_problem_its_predecessor(monkeypatch, P, slots):
    res, calls = _run_fake_chain(monkeypatch, P, slots, lambda j: 0)
    assert [int(r["x"][0]) for r in res] == list(range(1, P + 1))    # problem order
    sched = graph._chain_schedule(P, slots)
    assert len(calls) == len(sched)
    for call, rnd in zip(calls, sched):
        assert [c[0] for c in call] == [j for j, _ in rnd]
        for (j, x0, l0, warm, rho), (_, pred) in zip(call, rnd):
            if pred is None:
                assert not warm and x0 is None and l0 is None and rho == 0.7
            else:
                assert warm and x0 is res[pred]["x"] and l0 is res[pred]["l"] and rho == res[pred]["rho"] == 10.0 + pred


@pytest.mark.parametrize("bad", [1, 2, 4])
def test_chain_starts_cold_after_a_failed_predecessor(monkeypatch, bad):
    res, calls = _run_fake_chain(monkeypatch, 6, 2, lambda j: bad if j in (1, 3) else (3 if j == 4 else 0))
    by_problem = {c[0]: c for call in calls for c in call}
    for j in (2, 4):            # successors of the failed problems 1 and 3
        _, x0, l0, warm, rho = by_problem[j]
        assert not warm and x0 is None and l0 is None and rho == 0.7
    for j in (1, 5):            # successors of a solved problem (0) and of one at max_iter (4)
        _, x0, l0, warm, rho = by_problem[j]
        assert warm and x0 is res[j - 1]["x"] and l0 is res[j - 1]["l"] and rho == 10.0 + (j - 1)


def test_bad_starts_raise_before_the_library(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")

    for name in ("PogsAmdSolveBatchFn", "PogsAmdSolveBatchSparseFn", "PogsAmdSolveBatchWarmFn"):
        monkeypatch.setattr(graph.lib, name, boom)
    m, n = 20, 10
    s = _fake_solver(m, n)
    f, g = graph.lasso_functions(np.ones(m), 0.1, n)
    x, l = np.zeros(n), np.zeros(m)
    with pytest.raises(ValueError):
        s.solve_batch([f, f], [g, g], x0=[x, x])                                  # x0 without l0
    with pytest.raises(ValueError):
        s.solve_batch([f, f], [g, g], l0=[l, l])                                  # l0 without x0
    with pytest.raises(ValueError):
        s.solve_batch([f, f], [g, g], warm=[True, False])                         # flags without a start
    with pytest.raises(ValueError):
        s.solve_batch([f, f], [g, g], x0=[x], l0=[l, l])                          # x0 count
    with pytest.raises(ValueError):
        s.solve_batch([f, f], [g, g], x0=[x, x], l0=[l, l, l])                    # l0 count
    with pytest.raises(ValueError):
        s.solve_batch([f, f], [g, g], x0=[x, x], l0=[l, l], warm=[True])          # flag count
    with pytest.raises(ValueError):
        s.solve_batch([f, f], [g, g], x0=[x, np.zeros(n + 1)], l0=[l, l])         # x0 length
    with pytest.raises(ValueError):
        s.solve_batch([f, f], [g, g], x0=[x, x], l0=[np.zeros(m - 1), l])         # l0 length
    with pytest.raises(ValueError):
        s.solve_batch([f, f], [g, g], x0=[x, None], l0=[l, l])                    # None at a warm member
    with pytest.raises(ValueError):
        s.solve_batch([f, f], [g, g], x0=[x, x], l0=[None, l], warm=[True, False])
    # None is fine where the flag is false: this gets as far as the library
    with pytest.raises(AssertionError, match="the library was called"):
        s.solve_batch([f, f], [g, g], x0=[x, None], l0=[l, None], warm=[True, False])
