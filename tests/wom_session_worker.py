#!/usr/bin/env python3
"""One rank of the WOM-across-ranks test (tests/test_gpu_wom_session.py): WOM_GC and WOM_C of a real band with the loop's matrices
kept as column panels in slab form, once with the vocabulary calls in the session (option wom_session = 1) and once with the tail
of a Heun trial and the canonical step's dots in one pass per panel (2).  RANK / WORLD_SIZE / NTPOLY_AMD_COMM come from the
environment; the ranks share ONE GPU and exchange through the shared-memory test transport.

    python tests/wom_session_worker.py <out-prefix>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
KEYS = ("solves", "heun_passes", "c_dot_passes", "refused")


def main():
    out = sys.argv[1]
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    n, h = 2048, 20
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
    for kind in ("gc", "c"):
        for option in (1, 2):
            name = "%s_%d" % (kind, option)
            nt.set_option("wom_session", option)
            p = nt.SolverParameters()
            p.SetThreshold(1e-8)
            K = nt.Matrix_ps(n)
            before = nt.wom_session_counts()
            if kind == "gc":
                e = nt.FermiOperator.WOM_GC(H, I, K, 0.0, 2.0, p)
            else:
                e = nt.FermiOperator.WOM_C(H, I, K, n / 2.0, 2.0, p)
            after = nt.wom_session_counts()
            tr = nt.solver_trace()
            col, row, val = K.triplets()
            res.update({"col_" + name: col, "row_" + name: row, "val_" + name: val, "e_" + name: np.array([e]),
                        "iters_" + name: np.array([tr["iterations"]]), "value_" + name: np.asarray(tr["value"]).copy(),
                        "sigma_" + name: np.asarray(tr["sigma"]).copy(), "energy_" + name: np.asarray(tr["energy"]).copy(),
                        "nnz_" + name: np.asarray(tr["nnz"]).copy(), "counts_" + name: np.array([after[q] - before[q] for q in KEYS])})
    nt.set_option("wom_session", 0)
    np.savez(out + ".%d.npz" % rank, **res)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
