#!/usr/bin/env python3
"""One rank of the PurificationExtrapolate-across-ranks test (tests/test_gpu_purify_session.py): the solver test's density and
overlap as column panels, solved with option purify_session = 2 (the tail of an iteration in one pass per panel), 1 (the vocabulary
calls in the session) and 0 (compressed columns) in the same processes.  RANK / WORLD_SIZE / NTPOLY_AMD_COMM come from the
environment; the ranks share ONE GPU and exchange through the shared-memory test transport.

    python tests/purify_session_worker.py <out-prefix>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
KEYS = ("solves", "fold_passes", "plain_passes", "refused")


def main():
    out = sys.argv[1]
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    import ntpoly_amd as nt
    from test_gpu_purify_session import CONV, MAXIT, SOLVE_N, THR, TRACE, solve_operands
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    n = SOLVE_N
    D, S = nt.Matrix_ps(n), nt.Matrix_ps(n)
    c0, c1 = D.local_columns()
    for M, (col, row, val) in zip((D, S), solve_operands(n, c0, c1)):
        t = nt.TripletList_r()
        t.set_arrays(col, row, val)
        M.FillFromTripletList(t, prepartitioned=True)
    res = {}
    for option in (2, 1, 0):
        nt.set_option("purify_session", option)
        p = nt.SolverParameters()
        p.SetThreshold(THR)
        p.SetConvergeDiff(CONV)
        p.SetMaxIterations(MAXIT)
        p.SetMonitorConvergence(False)
        K = nt.Matrix_ps(n)
        before = nt.purify_session_counts()
        nt.GeometryOptimization.PurificationExtrapolate(D, S, TRACE, K, p)
        after = nt.purify_session_counts()
        tr = nt.solver_trace()
        col, row, val = K.triplets()
        name = "%d" % option
        res.update({"col_" + name: col, "row_" + name: row, "val_" + name: val, "iters_" + name: np.array([tr["iterations"]]),
                    "norm_" + name: np.asarray(tr["value"]).copy(), "sigma_" + name: np.asarray(tr["sigma"]).copy(),
                    "trace_" + name: np.asarray(tr["energy"]).copy(), "nnz_" + name: np.asarray(tr["nnz"]).copy(),
                    "counts_" + name: np.array([after[q] - before[q] for q in KEYS])})
    nt.set_option("purify_session", 0)
    np.savez(out + ".%d.npz" % rank, **res)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
