#!/usr/bin/env python3
"""One rank of the complex-block-scope test (tests/test_gpu_block_scope_complex.py): solvers on a complex Hermitian 3-D lattice
(no runs, no band) on several ranks, run in the pattern's BLOCK order with every panel product on the complex tile products of the
block path (csrc/band_scope.cpp, option block_scope_complex; psmatrix.cpp multiply_panel).  RANK / WORLD_SIZE / NTPOLY_AMD_COMM
come from the environment; the ranks share ONE GPU and exchange through the shared-memory test transport.

    python tests/block_scope_complex_worker.py <out-prefix> [solves|trs2|band|order]

solves: SignFunction of H, Invert and InverseSquareRoot of H + 2.5 I (H: the complex Hermitian L^3 lattice, L =
        NTPOLY_AMD_BSC_L, default 20; NTPOLY_AMD_BSC_SOLVES picks some of sign,inv,isq)
trs2:   six TRS2 iterations on H with the real identity as ISQ (monitor off)
band:   Invert of a shifted complex Hermitian band under a random relabelling (the band search recovers it: the band scope)
order:  (one rank) the block order of the complex lattice's pattern and of the real matrix with its pattern and moduli
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SOLVES = ("sign", "inv", "isq")


def hermitian(trip, phase=0.1):
    """a Hermitian complex operand with the pattern and |values| of a real symmetric one: H(r, c) = v exp(i phase (r - c))"""
    c, r, v = trip
    return c, r, v * np.exp(1j * phase * (r.astype(np.float64) - c.astype(np.float64)))


def main():
    out = sys.argv[1]
    mode = sys.argv[2] if len(sys.argv) > 2 else "solves"
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    L = int(os.environ.get("NTPOLY_AMD_BSC_L", "20"))
    import ntpoly_amd as nt
    from gen import lattice_triplets, permuted_banded_triplets
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    for kv in filter(None, os.environ.get("NTPOLY_AMD_TEST_OPTIONS", "").split(",")):   # (name=value,...: options of this run)
        k, v = kv.split("=")
        nt.set_option(k, int(v))
    res = {}

    def matrix(n, gen, cplx=True):
        M = nt.Matrix_ps(n)
        c0, c1 = M.local_columns()
        t = nt.TripletList_c() if cplx else nt.TripletList_r()
        t.set_arrays(*gen(c0, c1))
        M.FillFromTripletList(t, prepartitioned=True)
        return M

    def keep(tag, O, H):
        """entries of this rank's panel and a few sums (this rank's part; trace, norm and dot are the engine's, global)"""
        c, r, v = O.triplets()
        v = np.asarray(v, dtype=np.complex128)
        res[tag + "_nnz"] = np.array([len(v)])
        res[tag + "_sums"] = np.array([np.sum(v.real), np.sum(v.imag), np.sum(np.abs(v) ** 2)])
        dot = complex(O.Dot(H))
        res[tag + "_glob"] = np.array([O.Trace(), O.Norm(), dot.real, dot.imag])
        res[tag + "_col"], res[tag + "_row"], res[tag + "_val"] = c, r, v

    def counted(tag, fn):
        k0, b0 = nt.block_scope_counts(), nt.band_scope_counts()
        fn()
        k1, b1 = nt.block_scope_counts(), nt.band_scope_counts()
        tr = nt.solver_trace()
        res[tag + "_block_scope"] = np.array([k1["solves"] - k0["solves"], k1["products"] - k0["products"]])
        res[tag + "_band_scope"] = np.array([b1["solves"] - b0["solves"]])
        res[tag + "_iters"] = np.array([tr["iterations"]])
        res[tag + "_iter_nnz"] = np.asarray(tr["nnz"], dtype=np.int64)   # (this rank's panel of every iterate)
        res[tag + "_energy"] = np.asarray(tr["energy"], dtype=np.float64)

    p = nt.SolverParameters()
    p.SetThreshold(1e-8)
    p.SetConvergeDiff(1e-7)
    n = L ** 3
    if mode == "solves":
        pick = os.environ.get("NTPOLY_AMD_BSC_SOLVES", ",".join(SOLVES)).split(",")
        H = matrix(n, lambda c0, c1: hermitian(lattice_triplets(L, c0=c0, c1=c1)))
        S = matrix(n, lambda c0, c1: hermitian(lattice_triplets(L, c0=c0, c1=c1, shift=2.5)))
        for tag, fn, M in (("sign", nt.SignSolvers.ComputeSign, H), ("inv", nt.InverseSolvers.Invert, S),
                           ("isq", nt.SquareRootSolvers.InverseSquareRoot, S)):
            if tag not in pick:
                continue
            O = nt.Matrix_ps(n)
            counted(tag, lambda: fn(M, O, p))
            keep(tag, O, M)
            del O
    elif mode == "trs2":
        H = matrix(n, lambda c0, c1: hermitian(lattice_triplets(L, c0=c0, c1=c1)))
        ISQ = nt.Matrix_ps(n)
        ISQ.FillIdentity()
        q = nt.SolverParameters()
        q.SetThreshold(1e-8)
        q.SetConvergeDiff(1e-30)
        q.SetMaxIterations(6)
        q.SetMonitorConvergence(False)
        K = nt.Matrix_ps(n)
        counted("trs2", lambda: res.__setitem__("trs2_scal", np.array(nt.DensityMatrixSolvers.TRS2(H, ISQ, n / 2.0, K, q))))
        res["trs2_sigma"] = np.asarray(nt.solver_trace()["sigma"], dtype=np.float64)
        keep("trs2", K, H)
    elif mode == "band":
        nb = 8192
        B = matrix(nb, lambda c0, c1: permuted_banded_triplets(nb, 10, 42, c0=c0, c1=c1, shift=3.0, complex_=True))
        O = nt.Matrix_ps(nb)
        counted("band", lambda: nt.InverseSolvers.Invert(B, O, p))
        keep("band", O, B)
    elif mode == "order":
        L = 16
        n = L ** 3
        hc = hermitian(lattice_triplets(L))
        Hc = nt.Matrix_ps.from_triplets(n, *hc)
        Hr = nt.Matrix_ps.from_triplets(n, hc[0], hc[1], np.abs(hc[2]))   # (the real matrix with its pattern and moduli)
        nt.drop_block_caches()
        oc = nt.block_order_of_pattern(Hc)
        nt.drop_block_caches()
        orr = nt.block_order_of_pattern(Hr)
        again = nt.block_order_of_pattern(Hc)   # (kept under the pattern's fingerprint: found again, not made again)
        for tag, o in (("complex", oc), ("real", orr), ("again", again)):
            res["order_" + tag + "_ok"] = np.array([int(o is not None)])
            if o is not None:
                res["order_" + tag + "_pos"], res["order_" + tag + "_ns"] = o[0], np.array([o[1]])
    np.savez(out + ".%d.npz" % rank, **res)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
