#!/usr/bin/env python3
"""One rank of the square-root-chain-across-ranks test (tests/test_gpu_isr_chain.py): InverseSquareRoot (order 5) of a real band
with the loop's matrices kept as column panels in slab form and the step's polynomial chain in one pass per panel (option
isr_chain).  RANK / WORLD_SIZE / NTPOLY_AMD_COMM come from the environment; the ranks share ONE GPU and exchange through the
shared-memory test transport.

    python tests/isr_chain_worker.py <out-prefix>
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
    n, h = 2500, 20
    import ntpoly_amd as nt
    from gen import banded_triplets
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    S = nt.Matrix_ps(n)
    c0, c1 = S.local_columns()
    col, row, val = banded_triplets(n, h, shift=2.0, c0=c0, c1=c1)
    k = val != 0   # (no stored zeros: slab form does not hold them)
    t = nt.TripletList_r()
    t.set_arrays(col[k], row[k], val[k])
    S.FillFromTripletList(t, prepartitioned=True)
    p = nt.SolverParameters()
    p.SetThreshold(1e-8)
    p.SetConvergeDiff(1e-8)
    Om = nt.Matrix_ps(n)
    before = nt.isr_chain_counts()
    nt.SquareRootSolvers.with_order(S, Om, p, True, 5)
    after = nt.isr_chain_counts()
    tr = nt.solver_trace()
    col, row, val = Om.triplets()
    np.savez(out + ".%d.npz" % rank, col=col, row=row, val=val, iters=np.array([tr["iterations"]]),
             counts=np.array([after[k] - before[k] for k in ("order5", "order3", "refused")]))
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
