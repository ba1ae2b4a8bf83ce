#!/usr/bin/env python3
"""One rank of the ScaleAndFold-across-ranks test (tests/test_gpu_scale_fold_step.py): ScaleAndFold purification of a real band with
the loop's matrices kept as column panels in slab form, once with the update, the energy and the next trace of an iteration in
one pass per panel (option scale_fold_step = 1) and once with the vocabulary calls (0).  RANK / WORLD_SIZE / NTPOLY_AMD_COMM come
from the environment; the ranks share ONE GPU and exchange through the shared-memory test transport.

    python tests/scale_fold_step_worker.py <out-prefix>
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
    n, h, iters = 4096, 20, 12
    import ntpoly_amd as nt
    from gen import banded_triplets
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    H = nt.Matrix_ps(n)
    c0, c1 = H.local_columns()
    col, row, val = banded_triplets(n, h, c0=c0, c1=c1)
    k = val != 0   # (no stored zeros: slab form does not hold them)
    t = nt.TripletList_r()
    t.set_arrays(col[k], row[k], val[k])
    H.FillFromTripletList(t, prepartitioned=True)
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    res = {}
    for name, option in (("off", 0), ("on", 1)):
        nt.set_option("scale_fold_step", option)
        p = nt.SolverParameters()
        p.SetThreshold(1e-8)
        p.SetConvergeDiff(1e-30)
        p.SetMaxIterations(iters)
        p.SetMonitorConvergence(False)
        K = nt.Matrix_ps(n)
        before = nt.scale_fold_step_counts()
        nt.DensityMatrixSolvers.ScaleAndFold(H, I, n / 2.0, K, -0.05, 0.05, p)
        after = nt.scale_fold_step_counts()
        tr = nt.solver_trace()
        col, row, val = K.triplets()
        res.update({"col_" + name: col, "row_" + name: row, "val_" + name: val, "iters_" + name: np.array([tr["iterations"]]),
                    "sigma_" + name: np.asarray(tr["sigma"]).copy(), "energy_" + name: np.asarray(tr["energy"]).copy(),
                    "nnz_" + name: np.asarray(tr["nnz"]).copy(),
                    "counts_" + name: np.array([after[q] - before[q] for q in ("updates", "dot_traces", "refused")])})
    np.savez(out + ".%d.npz" % rank, **res)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
