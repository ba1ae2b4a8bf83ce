#!/usr/bin/env python3
"""One rank of the complex-slab-session-across-ranks test (tests/test_gpu_panel_sessions_complex.py): the sign, inverse,
square-root and inverse-square-root loops on a complex Hermitian band, with their iterates kept as complex column panels in
slab form and the products exchanging complex runs (psmatrix.cpp panel_slab_multiply on the complex tile kernel).
RANK / WORLD_SIZE / NTPOLY_AMD_COMM come from the environment; the ranks share ONE GPU and exchange through the
shared-memory test transport.

    python tests/complex_panel_session_worker.py <out-prefix> [loops|refuse|single]

loops:  the four loops on the band (N = NTPOLY_AMD_PANEL_N, default 16 384)
refuse: Invert on the shifted band with a few dense columns in the panel of rank 1 of two: that rank cannot take its panel
        products in slab form, every rank must decline them together
single: the four loops in ONE process (no RCCL-less ranks: NTPOLY_AMD_FORCE_RCCL decides whether a 1-rank communicator is made)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOOPS = ("sign", "inv", "sqrt", "isq")
DENSE_FRACTION = 0.75   # refuse: the dense columns sit at this fraction of the dimension (rank 1's panel of two)


def main():
    out = sys.argv[1]
    mode = sys.argv[2] if len(sys.argv) > 2 else "loops"
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    n = int(os.environ.get("NTPOLY_AMD_PANEL_N", "16384"))
    import ntpoly_amd as nt
    from gen import banded_triplets
    if mode == "single":
        nt.init_comm()
    else:
        nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world if mode != "single" else 1, 1)
    for kv in filter(None, os.environ.get("NTPOLY_AMD_TEST_OPTIONS", "").split(",")):   # (name=value,...: options of this run)
        k, v = kv.split("=")
        nt.set_option(k, int(v))
    res = {}

    def banded(h, shift, dense=()):
        M = nt.Matrix_ps(n)
        c0, c1 = M.local_columns()
        col, row, val = banded_triplets(n, h, complex_=True, shift=shift, c0=c0, c1=c1)
        extra = [j for j in dense if c0 <= j - 1 < c1]
        if extra:   # (dense columns: every row outside the band, small values; column-major order kept)
            ec, er, ev = [col], [row], [val]
            for j in extra:
                r = np.arange(1, n + 1, dtype=np.int32)
                r = r[np.abs(r - j) > h]
                ec.append(np.full(len(r), j, dtype=np.int32))
                er.append(r)
                ev.append(1e-4 * (1.0 + 0.5j) * np.ones(len(r)))
            col, row, val = np.concatenate(ec), np.concatenate(er), np.concatenate(ev)
            o = np.lexsort((row, col))
            col, row, val = col[o], row[o], val[o]
        t = nt.TripletList_c()
        t.set_arrays(col, row, val)
        M.FillFromTripletList(t, prepartitioned=True)
        return M

    def keep(tag, M):
        c, r, v = M.triplets()
        res[tag + "_col"], res[tag + "_row"], res[tag + "_val"] = c, r, v

    def counted(tag, fn):
        p0, s0 = nt.panel_product_counts(), nt.slab_algebra_counts()
        fn()
        p1, s1 = nt.panel_product_counts(), nt.slab_algebra_counts()
        res[tag + "_panel"] = np.array([p1["slab"] - p0["slab"], p1["declined"] - p0["declined"], p1["host_syncs"] - p0["host_syncs"]])
        res[tag + "_slab"] = np.array([s1[k] - s0[k] for k in ("products", "merges", "others", "refusals")])
        tr = nt.solver_trace()
        res[tag + "_iters"] = np.array([tr["iterations"]])
        res[tag + "_norms"] = np.asarray(tr["value"], dtype=np.float64)

    p = nt.SolverParameters()
    p.SetThreshold(1e-8)
    p.SetConvergeDiff(1e-7)
    if mode == "refuse":
        d0 = int(DENSE_FRACTION * n)
        A = banded(20, 3.0, dense=(d0, d0 + 1, d0 + 2))
        Iv = nt.Matrix_ps(n)
        counted("inv", lambda: nt.InverseSolvers.Invert(A, Iv, p))
        keep("inv", Iv)
    else:
        # (sign: the indefinite band, shifted by half a step of its diagonal so that no diagonal entry is an exact zero -- a
        # stored zero is what slab form cannot hold, on one rank as on many; the others: shifted, positive definite)
        H = banded(20, 1e-3)
        S = banded(20, 3.0)
        for tag, fn, M in (("sign", nt.SignSolvers.ComputeSign, H), ("inv", nt.InverseSolvers.Invert, S),
                           ("sqrt", nt.SquareRootSolvers.SquareRoot, S), ("isq", nt.SquareRootSolvers.InverseSquareRoot, S)):
            O = nt.Matrix_ps(n)
            counted(tag, lambda: fn(M, O, p))
            keep(tag, O)
            del O
    np.savez(out + ".%d.npz" % rank, **res)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
