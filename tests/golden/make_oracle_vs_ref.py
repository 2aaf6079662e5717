"""Generates tests/golden/oracle_vs_ref.npz: the compiled reference's solutions (oracle/_ref/libpogs_cpu.so,
built by `make -C oracle ref`) of the problems of tests/test_oracle_vs_ref.py (CASES there), each run in a
clean subprocess (oracle_binding.ref_solve).  Seconds in the build container:

    python tests/golden/make_oracle_vs_ref.py

Only the outputs are stored (x, optval, final_iter, status per case); the problems are regenerated from
their seeds by the test."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import numpy as np  # noqa: E402

import oracle_binding as ob  # noqa: E402
import test_oracle_vs_ref as t  # noqa: E402
from helpers import soa  # noqa: E402


def main():
    assert ob.ref_available(), "oracle/_ref/libpogs_cpu.so not built (make -C oracle ref)"
    out = {}
    for name in t.CASES:
        A, f, g, dtype, kw = t.problem(name)
        r = ob.ref_solve(A, soa(f), soa(g), dtype=dtype, timeout=300, **kw)
        out.update({name + "_x": r["x"].astype(dtype), name + "_optval": r["optval"],
                    name + "_iterations": r["iterations"], name + "_status": r["status"]})
        print("%s: status %d, final_iter %d, optval %.12g" % (name, r["status"], r["iterations"], r["optval"]))
    np.savez_compressed(t.FIXTURE, **out)


if __name__ == "__main__":
    main()
