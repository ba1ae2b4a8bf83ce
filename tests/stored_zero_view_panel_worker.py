#!/usr/bin/env python3
"""One rank of tests/test_gpu_stored_zero_view_panels.py: a degree-8 Chebyshev polynomial of the generator's complex band with
its two STORED ZEROS (n = 2048, h = 24, Gershgorin radius 0.9) with options stored_zero_views = 1 and complex_poly_sessions = 2.
Across ranks the input's panel enters the session as a read-only view (its compressed columns kept, the halo carries its runs
as they are).  RANK / WORLD_SIZE / NTPOLY_AMD_COMM come from the environment; the ranks share ONE GPU and exchange through the
shared-memory test transport.

    python tests/stored_zero_view_panel_worker.py <out-prefix>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, H = 2048, 24
CHEBY = [0.7, -0.4, 0.3, 0.25, -0.2, 0.15, 0.1, -0.05, 0.02]   # (degree 8)


def main():
    out = sys.argv[1]
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    import ntpoly_amd as nt
    from gen import banded_triplets
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    nt.set_option("spgemm_fma", 1)
    nt.set_option("complex_poly_sessions", 2)
    nt.set_option("stored_zero_views", 1)
    col, row, val = banded_triplets(N, H, complex_=True)
    g = np.zeros(N)
    np.add.at(g, col - 1, np.abs(val))
    val = val * (0.9 / g.max())
    assert (val == 0).sum() == 2
    A = nt.Matrix_ps(N)
    c0, c1 = A.local_columns()
    mine = (col > c0) & (col <= c1)
    t = nt.TripletList_c()
    t.set_arrays(col[mine], row[mine], val[mine])
    A.FillFromTripletList(t, prepartitioned=True)
    p = nt.SolverParameters()
    p.SetThreshold(0.0)
    poly = nt.ChebyshevPolynomial(len(CHEBY))
    for k, v in enumerate(CHEBY):
        poly.SetCoefficient(k, v)
    Out = nt.Matrix_ps(N)
    v0, s0, q0 = nt.slab_view_counts(), nt.slab_algebra_counts(), nt.panel_product_counts()
    poly.Compute(A, Out, p)
    v1, s1, q1 = nt.slab_view_counts(), nt.slab_algebra_counts(), nt.panel_product_counts()
    res = {"view": np.array([v1[k] - v0[k] for k in ("built", "products", "taken", "declined")]),
           "slab": np.array([s1[k] - s0[k] for k in ("products", "merges", "others", "refusals")]),
           "panel": np.array([q1["slab"] - q0["slab"], q1["declined"] - q0["declined"]]),
           "stored_zeros": np.array(int((val[mine] == 0).sum()))}
    res["col"], res["row"], res["val"] = Out.triplets()
    res["in_col"], res["in_row"], res["in_val"] = A.triplets()
    res["want_in_val"] = val[mine]
    np.savez(out + ".%d.npz" % rank, **res)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
