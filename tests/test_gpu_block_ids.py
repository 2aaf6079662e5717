"""The dense one-pass iteration kernels deal rows and partial-sum slots by a LOGICAL workgroup id (csrc/stream.h:
logical_block_id) under which the workgroups that share an XCD own a contiguous id range.  The id must be a
permutation of the grid for every grid size -- a slot written twice or never is a wrong sum -- and nothing else may
depend on it: the solves below run the kernels at the grid shapes where the map is not the trivial one (grids that are
no multiple of the group, fewer row steps than workgroups, several steps per workgroup with a partial last round and a
partial last block) against the CPU oracle, with the tolerances and iteration-count checks of tests/test_gpu_dense.py
for the same problem families, and twice with identical bytes demanded.
"""
import numpy as np
import pytest

import oracle_binding as ob
from helpers import relerr, soa
from test_gpu_dense import _check_solution, _relerr_same_iteration, _xtol32

pytestmark = pytest.mark.gpu

KEYS = ("x", "y", "l")


def _pogs():
    import pogs_amd

    return pogs_amd


def _num_cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _same_bytes(a, b):
    assert a["iterations"] == b["iterations"] and a["status"] == b["status"]
    assert np.float64(a["optval"]).tobytes() == np.float64(b["optval"]).tobytes()
    for k in KEYS:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def _solve_twice_against_oracle(A, f, g, dtype, tight=None, **kw):
    pogs = _pogs()
    got = pogs._solve_graph_form(A, f, g, dtype=dtype, **kw)
    again = pogs._solve_graph_form(A, f, g, dtype=dtype, **kw)
    _same_bytes(got, again)
    want = ob.oracle_solve(A, soa(f), soa(g), dtype=dtype, **kw)
    _check_solution(A, f, g, got, want, dtype, tight=(dtype == np.float64) if tight is None else tight)
    return got, want


@pytest.mark.parametrize("grid", list(range(1, 20)) + [63, 64, 65, 255, 256, 257, 511, 512, 768, 1000, 2048, 2432, 2433])
def test_logical_ids_are_a_permutation_of_every_grid(grid):
    """Every id of [0, grid) exactly once; blocks of one residue class take one contiguous, ascending id range, the
    classes in order -- which is the formula of the issue: p = #{b' < grid : b' % G < b % G} + b // G."""
    from pogs_amd import _lib

    ids, group = _lib.block_id_check(grid)
    assert sorted(ids.tolist()) == list(range(grid))
    assert group == 8   # (0: a build with blockIdx.x as the id -- an A / B build, not the shipped one)
    b = np.arange(grid)
    below = np.array([np.count_nonzero((b % group) < x) for x in b % group])
    assert np.array_equal(ids, below + b // group)


@pytest.mark.parametrize("shape", [(301, 40), (301, 1200)])
def test_fewer_row_steps_than_workgroups(shape):
    """301 rows at eight rows per step (64 x 1 and 256 x 2 plans): 38 workgroups -- a grid that is no multiple of 8 --
    one step each, the last block with five of its eight rows."""
    pogs = _pogs()
    from pogs_amd import synth

    m, n = shape
    A, b, _ = synth.dense_lasso(m, n, seed=19, dtype=np.float32)
    f, g = pogs.graph.lasso_functions(b, 0.1, n)
    _solve_twice_against_oracle(A, f, g, np.float32)


@pytest.fixture(scope="module")
def tall_narrow():
    """8 columns (the 64 x 1 plan: eight rows per step, eight workgroups per CU), three full rounds of the grid and a
    37-row tail: several steps per workgroup, a last round that only some workgroups take, a partial last block.
    (Every coefficient of x_true non-zero: with eight columns the usual 10 % would leave b pure noise.)"""
    from pogs_amd import synth

    m = 3 * (_num_cu() * 8) * 8 + 37
    A, b, _ = synth.dense_lasso(m, 8, seed=23, dtype=np.float64, density=1.0)
    return A, b


def test_tall_narrow_several_steps_per_workgroup_fp64(tall_narrow):
    pogs = _pogs()
    A, b = tall_narrow
    f, g = pogs.graph.lasso_functions(b, 0.1, 8)
    _solve_twice_against_oracle(A, f, g, np.float64, tight=False)


def test_tall_narrow_several_steps_per_workgroup_fp32(tall_narrow):
    """In fp32 the two engines cross the stopping threshold eleven iterations apart on this matrix (124 against 135,
    with blockIdx.x as the id just the same): columns of 5e4 elements summed in fp32, by the oracle in plain loops.
    So the comparison is the one tests/test_gpu_dense.py makes in that situation: the iteration counts within 10 %,
    then both sides stopped at the SAME iteration (_relerr_same_iteration) under the fp32 bound _xtol32."""
    pogs = _pogs()
    A, b = tall_narrow
    A, b = A.astype(np.float32), b.astype(np.float32)
    f, g = pogs.graph.lasso_functions(b, 0.1, 8)
    got = pogs._solve_graph_form(A, f, g, dtype=np.float32)
    again = pogs._solve_graph_form(A, f, g, dtype=np.float32)
    _same_bytes(got, again)
    want = ob.oracle_solve(A, soa(f), soa(g), dtype=np.float32)
    assert got["status"] == want["status"] == 0
    assert abs(int(got["iterations"]) - int(want["iterations"])) <= max(3, int(0.1 * want["iterations"]))
    rel = _relerr_same_iteration(got, want, lambda k: pogs._solve_graph_form(A, f, g, dtype=np.float32, max_iter=k),
                                 lambda k: ob.oracle_solve(A, soa(f), soa(g), dtype=np.float32, max_iter=k))
    print("iterations %d / %d, rel err x at the same iteration %.3e" % (got["iterations"], want["iterations"], rel))
    assert rel < _xtol32(got["iterations"], want["iterations"])


def test_logistic_on_the_prefetching_kernel():
    """n = 5000: rows of 1250 float4 vectors, the 256 x 5 plan, where an fp32 logistic solve takes
    stream_rows2_pf_kernel; 3001 rows are 1501 steps of two rows over two workgroups per CU, the last a single row."""
    pogs = _pogs()
    from pogs_amd import synth

    m, n = 3001, 5000
    A, y, _ = synth.dense_logistic(m, n, seed=29, dtype=np.float32, logit_std=2.0)
    lam = 0.05 * float(np.max(np.abs(A.T @ y)))
    f, g = pogs.graph.logistic_functions(y, lam, n)
    _solve_twice_against_oracle(A, f, g, np.float32)


def test_wide_problem_on_the_mirrored_functor():
    """40 x 301: transposed storage, the one-pass kernel streams the 301 x-coordinates as its rows (FusedIterOp XSIDE)."""
    pogs = _pogs()
    from pogs_amd import synth

    A, b, _ = synth.dense_lasso(40, 301, seed=31, dtype=np.float32)
    f, g = pogs.graph.lasso_functions(b, 0.1, 301)
    _solve_twice_against_oracle(A, f, g, np.float32)


@pytest.mark.parametrize("max_iter", [1, 2, 3])
def test_first_iterations_follow_the_oracle(tall_narrow, max_iter):
    """Solves capped at 1, 2 and 3 iterations against the oracle capped the same way, on the tall matrix (several
    steps per workgroup): what one launch writes is what the next one reads.  Both sides stop at the same iteration,
    so they differ by rounding only: 2e-5 in fp32 (the same-iteration bound of tests/test_gpu_dense.py: _xtol32), on
    x and y together (x alone may still be zero), and ten times that on the dual, on the scale _check_solution
    measures it."""
    pogs = _pogs()
    A, b = tall_narrow
    A, b = A.astype(np.float32), b.astype(np.float32)
    f, g = pogs.graph.lasso_functions(b, 0.1, 8)
    got = pogs._solve_graph_form(A, f, g, dtype=np.float32, max_iter=max_iter)
    again = pogs._solve_graph_form(A, f, g, dtype=np.float32, max_iter=max_iter)
    _same_bytes(got, again)
    want = ob.oracle_solve(A, soa(f), soa(g), dtype=np.float32, max_iter=max_iter)
    assert got["status"] == want["status"] == 3
    assert got["iterations"] == want["iterations"] == max_iter - 1
    xy = lambda r: np.concatenate([np.asarray(r["x"], np.float64), np.asarray(r["y"], np.float64)])
    print("max_iter %d: rel err (x, y) %.3e" % (max_iter, relerr(xy(got), xy(want))))
    assert relerr(xy(got), xy(want)) < 2e-5
    l_scale = max(np.linalg.norm(want["l"]), 1e-2 * np.linalg.norm(want["y"]))
    assert np.linalg.norm(got["l"].astype(np.float64) - want["l"]) / l_scale < 2e-4
