#!/usr/bin/env python3
"""One rank of the two-rank case of tests/test_gpu_complex_poly_sessions.py: a degree-8 Chebyshev polynomial and
ComputeExponential of a complex Hermitian band (n = 2048, h = 24) with option complex_poly_sessions = 2 -- across ranks the
evaluations' matrices are complex column panels in slab form (option complex_panels), the recurrence step is the fused kernel
on each rank's panel.  RANK / WORLD_SIZE / NTPOLY_AMD_COMM come from the environment; the ranks share ONE GPU and exchange
through the shared-memory test transport.

    python tests/complex_poly_session_worker.py <out-prefix>
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
    res = {}

    def banded(scale):
        M = nt.Matrix_ps(N)
        c0, c1 = M.local_columns()
        col, row, val = banded_triplets(N, H, complex_=True, shift=1e-3, c0=c0, c1=c1)
        t = nt.TripletList_c()
        t.set_arrays(col, row, val * scale)
        M.FillFromTripletList(t, prepartitioned=True)
        return M

    def counted(tag, fn, M):
        p0, s0, f0 = nt.panel_product_counts(), nt.slab_algebra_counts(), nt.recurrence_step_count()
        fn()
        p1, s1 = nt.panel_product_counts(), nt.slab_algebra_counts()
        res[tag + "_fused"] = np.array(nt.recurrence_step_count() - f0)
        res[tag + "_panel"] = np.array([p1["slab"] - p0["slab"], p1["declined"] - p0["declined"]])
        res[tag + "_slab"] = np.array([s1[k] - s0[k] for k in ("products", "merges", "others", "refusals")])
        res[tag + "_col"], res[tag + "_row"], res[tag + "_val"] = M.triplets()

    # (the band's Gershgorin radius is below 2.4: spectral radius below 1 for the polynomial, about 6 for the exponential --
    # negated, since PowerBounds' estimate for the band itself, whose dominant eigenvalue is negative, is negative and the
    # exponential then squares nothing)
    A, B = banded(0.4), banded(-2.5)
    p = nt.SolverParameters()
    p.SetThreshold(0.0)
    poly = nt.ChebyshevPolynomial(len(CHEBY))
    for k, v in enumerate(CHEBY):
        poly.SetCoefficient(k, v)
    O1 = nt.Matrix_ps(N)
    counted("cheby", lambda: poly.Compute(A, O1, p), O1)
    p.SetThreshold(1e-9)
    O2 = nt.Matrix_ps(N)
    counted("exp", lambda: nt.ExponentialSolvers.ComputeExponential(B, O2, p), O2)
    np.savez(out + ".%d.npz" % rank, **res)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
