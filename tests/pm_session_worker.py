#!/usr/bin/env python3
"""One rank of the PM-session-across-ranks test (tests/test_gpu_pm_session.py): the PM loop on a banded operand with its iterate
kept as a column panel in slab form and the stored zeros carried in a per-panel list (option pm_session).  RANK / WORLD_SIZE /
NTPOLY_AMD_COMM come from the environment; the ranks share ONE GPU and exchange through the shared-memory test transport.

    python tests/pm_session_worker.py <out-prefix>
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
    n, h, nel = 512, 10, 256.0
    import ntpoly_amd as nt
    from gen import banded_triplets
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    H = nt.Matrix_ps(n)
    c0, c1 = H.local_columns()
    t = nt.TripletList_r()
    t.set_arrays(*banded_triplets(n, h, c0=c0, c1=c1))
    H.FillFromTripletList(t, prepartitioned=True)
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    p = nt.SolverParameters()
    p.SetThreshold(1e-8)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(14)
    p.SetMonitorConvergence(False)
    K = nt.Matrix_ps(n)
    before = nt.pm_session_counts()
    nt.DensityMatrixSolvers.PM(H, I, nel, K, p)
    after = nt.pm_session_counts()
    tr = nt.solver_trace()
    col, row, val = K.triplets()
    np.savez(out + ".%d.npz" % rank, col=col, row=row, val=val, nnz=tr["nnz"], iters=np.array([tr["iterations"]]),
             counts=np.array([after[k] - before[k] for k in ("sigma", "updates", "zeros", "left")]))
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
