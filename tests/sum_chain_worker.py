#!/usr/bin/env python3
"""One rank of the two-rank test of option sum_chain (tests/test_gpu_sum_chain.py): the solver test's operands as column panels,
Cosine and the factorized Chebyshev evaluation with option sum_chain = 1 (each panel's sum chains in one pass each) and 0 in the
same processes; the result of option 1 is also gathered whole on every rank.
RANK / WORLD_SIZE / NTPOLY_AMD_COMM come from the environment; the ranks share ONE GPU and exchange through the shared-memory test
transport.

    python tests/sum_chain_worker.py <out-prefix>
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
    from test_gpu_sum_chain import KEYS, SIZES, WORKER_KINDS, THR, SOLVERS, coefficients, solve_triplets, srt
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    n, h = SIZES[0]
    res = {}
    for kind in WORKER_KINDS:
        A = nt.Matrix_ps(n)
        c0, c1 = A.local_columns()
        t = nt.TripletList_r()
        t.set_arrays(*solve_triplets(kind, n, h, c0, c1))
        A.FillFromTripletList(t, prepartitioned=True)
        for option in (1, 0):
            nt.set_option("sum_chain", option)
            p = nt.SolverParameters()
            p.SetThreshold(THR)
            p.SetConvergeDiff(1e-30)
            p.SetMaxIterations(8)
            p.SetMonitorConvergence(False)
            K = nt.Matrix_ps(n)
            before = nt.sum_chain_counts()
            if kind == "cos":
                nt.TrigonometrySolvers.Cosine(A, K, p)
            else:
                arg = SOLVERS[kind][1]
                poly = nt.ChebyshevPolynomial(arg)
                for k, v in enumerate(coefficients(arg)):
                    poly.SetCoefficient(k, v)
                poly.ComputeFactorized(A, K, p)
            after = nt.sum_chain_counts()
            col, row, val = srt(K.triplets())
            name = "%s_%%s_%d" % (kind, option)
            res.update({name % "col": col, name % "row": row, name % "val": val, name % "counts": np.array([after[q] - before[q] for q in KEYS])})
            if option == 1:
                col, row, val = srt(K.GatherMatrixToProcess().triplets())
                res.update({kind + "_all_col": col, kind + "_all_row": row, kind + "_all_val": val})
    nt.set_option("sum_chain", 0)
    np.savez(out + ".%d.npz" % rank, **res)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
