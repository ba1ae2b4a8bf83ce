#!/usr/bin/env python3
"""One rank of the multi-rank vocabulary test (tests/test_gpu_multirank_vocabulary.py): RANK / WORLD_SIZE /
NTPOLY_AMD_COMM come from the environment as for tests/multirank_worker.py, the ranks are processes sharing ONE GPU and
exchange through the shared-memory test transport (csrc/comm.cpp), the grid is 1 x world x 1.  Runs EVERY case of
tests/vocab_cases.py in this one process (a run costs one process start per rank, not one per case) and writes this
rank's results -- local triplets and scalars, keys "<case>.<tag>" -- to <out>.<rank>.npz.

    python tests/multirank_vocab_worker.py <out-prefix>
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out = sys.argv[1]
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    import ntpoly_amd as nt
    import vocab_cases as V
    from ntpoly_amd.capi import i
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    res = {}

    for case in V.cases():
        cid, n, cplx = case["id"], case["n"], case["cplx"]
        TList = nt.TripletList_c if cplx else nt.TripletList_r

        def keep(tag, M):
            c, r, v = M.triplets()
            res["%s.%s_col" % (cid, tag)], res["%s.%s_row" % (cid, tag)], res["%s.%s_val" % (cid, tag)] = c, r, v

        def keep_list(tag, t):
            c, r, v = t.arrays()
            res["%s.%s_col" % (cid, tag)], res["%s.%s_row" % (cid, tag)], res["%s.%s_val" % (cid, tag)] = c, r, v

        def scalar(tag, *v):
            res["%s.%s" % (cid, tag)] = np.array(v)

        def columns(tag, M):
            scalar(tag + "_panel", M.GetActualDimension(), *M.local_columns())

        def tlist(t):
            tl = nt.TripletList_c() if np.iscomplexobj(t[2]) else nt.TripletList_r()
            tl.set_arrays(*t)
            return tl

        def fill(t):
            """this rank's own columns of the operand, prepartitioned"""
            M = nt.Matrix_ps(n)
            c0, c1 = M.local_columns()
            sel = (t[0] > c0) & (t[0] <= c1)
            M.FillFromTripletList(tlist((t[0][sel], t[1][sel], t[2][sel])), prepartitioned=True)
            return M

        mats = {name: fill(t) for name, t in case["ops"].items() if name not in case["transposed"]}
        for name, src in case["transposed"].items():
            mats[name] = nt.Matrix_ps(n)
            mats[name].Transpose(mats[src])
        A, B = mats["A"], mats["B"]
        columns("A", A)
        keep("A", A)

        # ---- products
        for tag, left, right, alpha, beta, thr, prefill in V.product_runs(case):
            Cm = fill(case["ops"][prefill]) if prefill else nt.Matrix_ps(n)
            Cm.Gemm(mats[left], mats[right], None, alpha, beta, thr)
            keep(tag, Cm)

        # ---- the plain product under every setting of the overlapped halo exchange
        try:
            for ov in V.HALO_OVERLAP:
                nt.set_option("halo_overlap", ov)
                for left, right in case["overlap_pairs"]:
                    Cm = nt.Matrix_ps(n)
                    Cm.Gemm(mats[left], mats[right], None, 1.0, 0.0, 0.0)
                    keep("ov%d_%s_%s" % (ov, left, right), Cm)
        finally:
            nt.set_option("halo_overlap", 1)

        # ---- element-wise calls
        T = nt.Matrix_ps(n)
        T.Transpose(A)
        keep("transpose", T)
        if cplx:
            Cj = nt.Matrix_ps(A)
            Cj.Conjugate()
            keep("conjugate", Cj)
        for k, (alpha, thr) in enumerate(V.INCREMENT_PARAMS):
            for seq in V.INCREMENT_SEQ:
                nt.set_option("increment_force_seq", seq)
                try:
                    R = nt.Matrix_ps(B)
                    R.Increment(A, alpha, thr)
                finally:
                    nt.set_option("increment_force_seq", 0)
                keep("inc%d_seq%d" % (k, seq), R)
        Pw = nt.Matrix_ps(n)
        Pw.PairwiseMultiply(A, B)
        keep("pairwise", Pw)
        Sc = nt.Matrix_ps(A)
        Sc.Scale(-2.0)
        keep("scale", Sc)

        # ---- scalars and predicates
        d = A.Dot(B)
        scalar("dot", np.real(d), np.imag(d))
        scalar("trace", B.Trace())
        scalar("norm", B.Norm())
        scalar("size", A.GetSize())
        if not cplx:
            scalar("gershgorin", *nt.EigenBounds.GershgorinBounds(B))
        scalar("asymmetry", A.MeasureAsymmetry())
        Sy = nt.Matrix_ps(A)
        Sy.Symmetrize()
        keep("symmetrize", Sy)
        scalar("is_identity", int(A.IsIdentity()))
        Id = nt.Matrix_ps(n)
        Id.FillIdentity()
        keep("identity", Id)
        scalar("identity_scalars", int(Id.IsIdentity()), Id.Trace(), Id.Norm())

        # ---- relabelling
        perm = nt.Permutation(n)
        perm.set_lookup(case["lookup"])
        Pm = nt.Matrix_ps(n)
        nt.LoadBalancer.PermuteMatrix(A, Pm, perm)
        keep("permute", Pm)
        Un = nt.Matrix_ps(n)
        nt.LoadBalancer.UndoPermuteMatrix(Pm, Un, perm)
        keep("unpermute", Un)
        PR = nt.Matrix_ps(n)
        PR.FillPermutation(perm, True)
        keep("fill_permutation", PR)
        PA = nt.Matrix_ps(n)
        PA.Gemm(PR, A, None, 1.0, 0.0, 0.0)
        keep("permutation_product", PA)

        # ---- fill from anywhere: rank r passes the triplets at the positions i of the whole list with i % world == r
        Any = nt.Matrix_ps(n)
        Any.FillFromTripletList(tlist(V.split_for_rank(case["ops"]["A"], rank, world)), prepartitioned=False)
        keep("fill_anywhere", Any)

        # ---- slice, resize, block, diagonal scale (the entry points of the C++ layer)
        if n >= 3:
            Sl = nt.Matrix_ps(1)
            nt.lib.GetMatrixSlice_wrp(A.ih, Sl.ih, i(2), i(n - 1), i(1), i((n + 1) // 2))
            columns("slice", Sl)
            keep("slice", Sl)
        for tag, size in (("resize_down", (n + 1) // 2), ("resize_up", n + 3)):
            Rz = nt.Matrix_ps(A)
            nt.lib.ResizeMatrix_ps_wrp(Rz.ih, i(size))
            columns(tag, Rz)
            keep(tag, Rz)
        tb = TList()
        getattr(nt.lib, "GetMatrixBlock_ps%s_wrp" % ("c" if cplx else "r"))(A.ih, tb.ih, i(1), i(n + 1), i(1 + rank), i(n + 1))
        keep_list("block", tb)
        Ds = nt.Matrix_ps(A)
        td = tlist(case["diag"])
        getattr(nt.lib, "MatrixDiagonalScale_ps%s_wrp" % ("c" if cplx else "r"))(Ds.ih, td.ih)
        keep("diagonal_scale", Ds)

        # ---- gather: the whole matrix on every rank, and on one rank only
        keep("gather_all", A.GatherMatrixToProcess())
        target = min(1, world - 1)
        Lone = A.GatherMatrixToProcess(target)
        scalar("gather_one_here", int(Lone is not None))
        if Lone is not None:
            keep("gather_one", Lone)

    nt.barrier()
    np.savez(out + ".%d.npz" % rank, **res)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
