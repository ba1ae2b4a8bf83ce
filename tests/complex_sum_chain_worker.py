#!/usr/bin/env python3
"""One rank of the two-rank test of option complex_sum_chain (tests/test_gpu_complex_sum_chain.py): the solver test's complex
operands as column panels, Cosine and ComputeInverseRoot(5) with the option at 2 (each panel's sum chains in one pass each) and at 1
(the same sessions, the vocabulary calls) in the same processes.
RANK / WORLD_SIZE / NTPOLY_AMD_COMM come from the environment; the ranks share ONE GPU and exchange through the shared-memory test
transport.

    python tests/complex_sum_chain_worker.py <out-prefix>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KEYS = ("sessions", "passes", "refused")


def main():
    out = sys.argv[1]
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    import ntpoly_amd as nt
    from test_gpu_complex_sum_chain import ITERATIONS, SIZES, SOLVERS, THR, THRESHOLDS, WORKER_KINDS, solve_triplets, srt
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    n, h = SIZES[0]
    res = {}
    for kind in WORKER_KINDS:
        A = nt.Matrix_ps(n)
        c0, c1 = A.local_columns()
        t = nt.TripletList_c()
        t.set_arrays(*solve_triplets(kind, n, h, c0, c1))
        A.FillFromTripletList(t, prepartitioned=True)
        for option in (2, 1):
            nt.set_option("complex_sum_chain", option)
            p = nt.SolverParameters()
            p.SetThreshold(THRESHOLDS.get(kind, THR))
            p.SetConvergeDiff(1e-30)
            p.SetMaxIterations(ITERATIONS.get(kind, 8))
            p.SetMonitorConvergence(False)
            K = nt.Matrix_ps(n)
            before, real_before = nt.complex_sum_chain_counts(), nt.sum_chain_counts()
            if kind == "cos":
                nt.TrigonometrySolvers.Cosine(A, K, p)
            else:
                nt.RootSolvers.ComputeInverseRoot(A, K, SOLVERS[kind][1], p)
            after = nt.complex_sum_chain_counts()
            assert nt.sum_chain_counts() == real_before
            col, row, val = srt(K.triplets())
            name = "%s_%%s_%d" % (kind, option)
            res.update({name % "col": col, name % "row": row, name % "val": val, name % "counts": np.array([after[q] - before[q] for q in KEYS])})
    nt.set_option("complex_sum_chain", 0)
    np.savez(out + ".%d.npz" % rank, **res)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
