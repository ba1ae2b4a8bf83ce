#!/usr/bin/env python3
"""One rank of the ComputeExponentialPade-across-ranks test (tests/test_gpu_pade_session.py): the solver test's shifted operand as
column panels, solved with option pade_session = 2 (both groups of merges in one pass each per panel), 1 (the vocabulary calls in
the session) and 0 (compressed columns) in the same processes, without and with a load balancer's permutation (the reverse one).
RANK / WORLD_SIZE / NTPOLY_AMD_COMM come from the environment; the ranks share ONE GPU and exchange through the shared-memory test
transport.

    python tests/pade_session_worker.py <out-prefix>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
KEYS = ("solves", "sum_passes", "pair_passes", "refused")


def main():
    out = sys.argv[1]
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    import ntpoly_amd as nt
    from test_gpu_pade_session import CONV, SOLVES, solve_triplets
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    n, thr = SOLVES["shifted"][0], SOLVES["shifted"][3]
    A = nt.Matrix_ps(n)
    c0, c1 = A.local_columns()
    t = nt.TripletList_r()
    t.set_arrays(*solve_triplets("shifted", c0, c1))
    A.FillFromTripletList(t, prepartitioned=True)
    res = {}
    perm = nt.Permutation(n)
    perm.SetReversePermutation()
    for option, balanced in ((2, False), (1, False), (0, False), (2, True), (1, True), (0, True)):
        nt.set_option("pade_session", option)
        p = nt.SolverParameters()
        p.SetThreshold(thr)
        p.SetConvergeDiff(CONV)
        if balanced:
            p.SetLoadBalance(perm)
        K = nt.Matrix_ps(n)
        before, cg_before = nt.pade_session_counts(), nt.cg_dots_counts()
        nt.ExponentialSolvers.ComputeExponentialPade(A, K, p)
        after, cg_after = nt.pade_session_counts(), nt.cg_dots_counts()
        col, row, val = K.triplets()
        name = "%d" % option
        pre = "lb_" if balanced else ""
        res.update({pre + "col_" + name: col, pre + "row_" + name: row, pre + "val_" + name: val,
                    pre + "counts_" + name: np.array([after[q] - before[q] for q in KEYS]),
                    pre + "passes_" + name: np.array([cg_after["passes"] + cg_after["refused"] - cg_before["passes"] - cg_before["refused"]])})
    nt.set_option("pade_session", 0)
    np.savez(out + ".%d.npz" % rank, **res)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
