"""One line per call through every multi-problem entry of the Python boundary (pogs_amd/graph.py), with a sha256 over
the call's outputs: two builds that print the same lines hand the same arguments to the same kernels.  Small lassos
from a seeded generator, both dtypes:
    Solver.solve                      dense 40 x 20, sparse 300 x 80
    Solver.solve_batch                k = 3, cold and warm-started, dense and sparse
    Solver.solve_chain                6 problems in 2 slots
    solve_many                        k = 3 of 40 x 20 and of 20 x 40
    solve_many_ragged                 (40, 20), (20, 40), (33, 7): a list, and a packed buffer in either order
    ManySolver, ManySolver.from_ragged  cold, then warm, then last
    chunked                           POGS_AMD_MANY_WORKSPACE_MB=0.25 and host matrices: solve_many on k = 37 of 90 x 40,
                                      solve_many_ragged and ManySolver.from_ragged on ten shapes from 1 x 4 to 300 x 129
                                      (the shapes of the chunking tests in tests/test_gpu_many*.py)
Each line: entry, shape, dtype, iterations, status, sha256 over x, y, l, mu, optval (and rho where returned).  A
one-shot many-problem call is followed by its verbose summary with the three times masked (chunks, launches, shape
text), a handle's solve by resident_bytes, launches and problem_iters of info().
    python scripts/boundary_digests.py [--tree DIR] [--out FILE]
--tree: import pogs_amd from another checkout's root (to compare its lines with this one's)."""
import argparse
import contextlib
import hashlib
import os
import re
import sys
import tempfile

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import scipy.sparse as sp  # noqa: E402

import pogs_amd  # noqa: E402
from pogs_amd import graph  # noqa: E402

LINES = []


def problem(m, n, seed, lam=0.2, sparse=False):
    """(A, f, g) of a lasso with lambda = lam * max|A^T b|"""
    rng = np.random.default_rng(seed)
    # (the sparse matrix: a tenth of the entries plus a diagonal, so that no row or column is empty)
    if sparse:
        A = (sp.random(m, n, density=0.1, random_state=seed) + sp.eye(m, n)).tocsr()
    else:
        A = rng.standard_normal((m, n))
    x = rng.standard_normal(n) * (rng.random(n) < 0.3)
    b = np.asarray(A @ x).ravel() + 0.1 * rng.standard_normal(m)
    f, g = graph.lasso_functions(b, lam * float(np.max(np.abs(A.T @ b))), n)
    return A, f, g


def members(res):
    """any result container as a list of per-problem dictionaries"""
    if isinstance(res, list):
        return res
    if np.ndim(res["optval"]) == 0:
        return [res]
    return [{key: res[key][j] for key in res} for j in range(len(res["optval"]))]


def line(entry, shape, dt, res):
    ms = members(res)
    h = hashlib.sha256()
    for r in ms:
        for key in ("x", "y", "l", "mu", "optval", "rho"):
            if key in r:
                h.update(np.ascontiguousarray(r[key]).tobytes())
    text = "%-34s %-28s %-7s it %-22s st %-14s %s" % (entry, shape, np.dtype(dt).name,
                                                       ",".join(str(int(r["iterations"])) for r in ms),
                                                       ",".join(str(int(r["status"])) for r in ms), h.hexdigest())
    LINES.append(text)
    print(text, flush=True)


@contextlib.contextmanager
def library_stdout():
    """what the library prints (C stdio) during the block, as a list of lines filled when the block ends"""
    got = []
    sys.stdout.flush()
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(1)
        os.dup2(tmp.fileno(), 1)
        try:
            yield got
        finally:
            os.dup2(keep, 1)
            os.close(keep)
            tmp.seek(0)
            got.extend(tmp.read().decode().splitlines())


def one_shot(entry, shape, dt, call, **kw):
    """a one-shot many-problem call: its digest line, then its verbose summary without the times"""
    with library_stdout() as said:
        res = call(dtype=dt, verbose=1, **kw)
    line(entry, shape, dt, res)
    for text in said:
        text = "    " + re.sub(r"(setup|loop|total) \S+ s", r"\1 * s", text)
        LINES.append(text)
        print(text, flush=True)


def run(dt):
    # ---- one matrix: solve, solve_batch, solve_chain -----------------------------------------------------------------
    for kind, (m, n) in (("dense", (40, 20)), ("sparse", (300, 80))):
        shape = "%s %dx%d" % (kind, m, n)
        A, f, g = problem(m, n, 1, sparse=kind == "sparse")
        pairs = [problem(m, n, 1, lam, sparse=kind == "sparse")[1:] for lam in (0.3, 0.2, 0.1)]
        fs, gs = [p[0] for p in pairs], [p[1] for p in pairs]
        with pogs_amd.Solver(A, dtype=dt) as s:
            line("Solver.solve", shape, dt, s.solve(f, g))
            cold = s.solve_batch(fs, gs, rho=[1.0, 0.5, 2.0])
            line("solve_batch cold", shape + " k=3", dt, cold)
            line("solve_batch warm", shape + " k=3", dt,
                 s.solve_batch(fs[::-1], gs[::-1], rho=1.5, x0=[r["x"] for r in cold], l0=[r["l"] for r in cold],
                               warm=[True, False, True]))
            if kind == "dense":
                path = [problem(m, n, 1, lam)[1:] for lam in (0.5, 0.4, 0.3, 0.2, 0.1, 0.05)]
                line("solve_chain 2 slots", shape + " P=6", dt,
                     s.solve_chain([p[0] for p in path], [p[1] for p in path], slots=2))
    # ---- a matrix per problem, one shape -----------------------------------------------------------------------------
    for m, n in ((40, 20), (20, 40)):
        ps = [problem(m, n, 10 + j) for j in range(3)]
        As, fs, gs = np.stack([p[0] for p in ps]), [p[1] for p in ps], [p[2] for p in ps]
        one_shot("solve_many", "k=3 %dx%d" % (m, n), dt, pogs_amd.solve_many, A=As, fs=fs, gs=gs, rho=[1.0, 0.5, 2.0])
    with pogs_amd.ManySolver(As, dtype=dt) as s:
        handle("ManySolver", "k=3 20x40", dt, s, fs, gs, np.stack)
    # ---- a matrix per problem, ragged --------------------------------------------------------------------------------
    shapes = [(40, 20), (20, 40), (33, 7)]
    ps = [problem(m, n, 20 + j) for j, (m, n) in enumerate(shapes)]
    As, fs, gs = [p[0] for p in ps], [p[1] for p in ps], [p[2] for p in ps]
    name = "40x20,20x40,33x7"
    one_shot("solve_many_ragged list", name, dt, pogs_amd.solve_many_ragged, As=As, fs=fs, gs=gs, rho=[1.0, 0.5, 2.0])
    for order in "CF":
        packed = np.concatenate([a.ravel(order=order) for a in As])
        one_shot("solve_many_ragged packed " + order, name, dt, pogs_amd.solve_many_ragged, As=packed, fs=fs, gs=gs,
                 shapes=shapes, order=order)
    with pogs_amd.ManySolver.from_ragged(As, dtype=dt) as s:
        handle("ManySolver.from_ragged", name, dt, s, fs, gs, list)
    # ---- a workspace cap of 0.25 MB and host matrices: several chunks ------------------------------------------------
    os.environ["POGS_AMD_MANY_WORKSPACE_MB"] = "0.25"
    ps = [problem(90, 40, 40 + j) for j in range(37)]
    one_shot("solve_many chunked", "k=37 90x40", dt, pogs_amd.solve_many, A=np.stack([p[0] for p in ps]),
             fs=[p[1] for p in ps], gs=[p[2] for p in ps])
    shapes = [(7, 3), (3, 7), (5, 5), (1, 4), (4, 1), (130, 64), (64, 130), (300, 129), (200, 128), (70, 257)]
    ps = [problem(m, n, 80 + j) for j, (m, n) in enumerate(shapes)]
    As, fs, gs = [p[0] for p in ps], [p[1] for p in ps], [p[2] for p in ps]
    one_shot("solve_many_ragged chunked", "ten shapes", dt, pogs_amd.solve_many_ragged, As=As, fs=fs, gs=gs)
    s = pogs_amd.ManySolver.from_ragged(As, dtype=dt)          # its setup runs in upload chunks
    del os.environ["POGS_AMD_MANY_WORKSPACE_MB"]
    with s:
        handle("from_ragged chunked upload", "ten shapes", dt, s, fs, gs, list)


def handle(entry, shape, dt, s, fs, gs, starts):
    """cold, then warm from the cold solution at other rho, then last; after each, what info() counts"""
    def solved(start, res):
        line(entry + " " + start, shape, dt, res)
        info = s.info()
        text = "    resident_bytes %d launches %d problem_iters %d" % (info["resident_bytes"], info["launches"],
                                                                       info["problem_iters"])
        LINES.append(text)
        print(text, flush=True)

    cold = s.solve(fs, gs)
    solved("cold", cold)
    k = len(fs)
    x0, l0 = starts([cold["x"][j] for j in range(k)]), starts([cold["l"][j] for j in range(k)])
    solved("warm", s.solve(fs, gs, rho=list(np.resize([0.5, 1.0, 2.0], k)), start="warm", x0=x0, l0=l0))
    solved("last", s.solve(fs, gs, rho=None, start="last"))


for dtype in (np.float64, np.float32):
    run(dtype)
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
