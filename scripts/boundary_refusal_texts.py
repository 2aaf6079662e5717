"""One line per refused call of the many-problem C entries (PogsAmdManyCreate, PogsAmdSolveManyFn,
PogsAmdManyCreateRagged, PogsAmdSolveManyRaggedFn): entry, the faulty arguments, return code, *out after a create, and
the message up to the source position.  Every call is refused on its arguments, before any device work, so this runs
without a GPU; two builds that print the same lines refuse the same calls in the same words and order of checks.
Cases: k = 0, k < 0, unknown ord / dtype / mem, null A, m = 0, both envelope bounds, a CGLS projector, two calls with
several faults at once, and each ragged call once more with a null m.
    python scripts/boundary_refusal_texts.py [--tree DIR] [--out FILE]
--tree: import pogs_amd from another checkout's root (to compare its lines with this one's)."""
import argparse
import ctypes
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

from pogs_amd import _lib  # noqa: E402

L = _lib.lib
CASES = [dict(k=0), dict(k=-2), dict(ord=7), dict(dtype=7), dict(mem=5), dict(A=None), dict(m=0), dict(m=513, n=513),
         dict(m=16385, n=1), dict(projector=2), dict(k=0, projector=2, dtype=7), dict(dtype=7, ord=7, mem=5)]
LINES = []


def note(entry, case, rc, out=None):
    text = _lib.last_error().rsplit(" at ", 1)[0]
    LINES.append("%-26s %-40s rc %d%s  %s" % (entry, case, rc, "" if out is None else " out %s" % out.value, text))
    print(LINES[-1])


buf = np.ones(64)
for case in CASES:
    c = dict(dict(k=1, m=6, n=4, dtype=1, ord=1, mem=0, projector=1, A=buf.ctypes.data), **case)
    cnt = max(c["k"], 1)
    fa, ga = (_lib.PogsAmdFn * cnt)(), (_lib.PogsAmdFn * cnt)()
    x, it, st = np.zeros(64), np.zeros(cnt, np.uint32), np.zeros(cnt, np.int32)
    opt = _lib.PogsAmdOptions(device=-1, projector=c["projector"])
    head = (c["dtype"], c["ord"], c["k"])
    solve = (ctypes.byref(opt), fa, ga, None, 1e-4, 1e-4, 10, 0, 1, 1, x.ctypes.data, None, None, None, None,
             it.ctypes.data, st.ctypes.data)
    h = ctypes.c_void_p(5)
    note("PogsAmdManyCreate", case, L.PogsAmdManyCreate(ctypes.byref(h), *head, c["m"], c["n"], c["A"], c["mem"],
                                                        ctypes.byref(opt)), h)
    note("PogsAmdSolveManyFn", case, L.PogsAmdSolveManyFn(*head, c["m"], c["n"], c["A"], c["mem"], *solve))
    ms, ns = (ctypes.c_size_t * cnt)(*[c["m"]] * cnt), (ctypes.c_size_t * cnt)(*[c["n"]] * cnt)
    for marr, tag in ((ms, ""), (None, " + null m")):
        h = ctypes.c_void_p(5)
        note("PogsAmdManyCreateRagged", str(case) + tag,
             L.PogsAmdManyCreateRagged(ctypes.byref(h), *head, marr, ns, c["A"], c["mem"], ctypes.byref(opt)), h)
        note("PogsAmdSolveManyRaggedFn", str(case) + tag,
             L.PogsAmdSolveManyRaggedFn(*head, marr, ns, c["A"], c["mem"], *solve))
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
