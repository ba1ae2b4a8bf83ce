#!/usr/bin/env python3
"""One rank of the two-rank test of option poly_step (tests/test_gpu_poly_step.py): the solver test's shifted operand as column
panels, ChebyshevPolynomial.Compute and ComputeExponential with option poly_step = 2 (each panel's step tail in one pass), 1 (the
exponential's squarings in the panel session) and 0 in the same processes.
RANK / WORLD_SIZE / NTPOLY_AMD_COMM come from the environment; the ranks share ONE GPU and exchange through the shared-memory test
transport.

    python tests/poly_step_worker.py <out-prefix>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out = sys.argv[1]
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    import ntpoly_amd as nt
    from test_gpu_poly_step import KEYS, SOLVES, run_solver, solve_triplets
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    n, thr = SOLVES["shifted"][0], SOLVES["shifted"][3]
    A = nt.Matrix_ps(n)
    c0, c1 = A.local_columns()
    t = nt.TripletList_r()
    t.set_arrays(*solve_triplets("shifted", c0, c1))
    A.FillFromTripletList(t, prepartitioned=True)
    res = {}
    for kind in ("cheby", "exp"):
        for option in (2, 1, 0):
            nt.set_option("poly_step", option)
            r = run_solver(nt, kind, A, n, thr)
            col, row, val = r["out"]
            name = "%s_%%s_%d" % (kind, option)
            res.update({name % "col": col, name % "row": row, name % "val": val, name % "counts": np.array([r["counts"][q] for q in KEYS])})
    nt.set_option("poly_step", 0)
    np.savez(out + ".%d.npz" % rank, **res)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
