#!/usr/bin/env python3
"""One rank of the thin-operand panel test (tests/test_gpu_thin_panels.py): slab sessions across ranks whose products take the
gather kernels of csrc/spgemm_thin.hip through the halo of the left operand (psmatrix.cpp panel_slab_multiply; the decision
is made on the entry counts of the whole operands, the same on every rank).  RANK / WORLD_SIZE / NTPOLY_AMD_COMM come from the
environment; the ranks share ONE GPU and exchange through the shared-memory test transport.

    python tests/thin_panel_worker.py <out-prefix> [loops|products]

loops:    InverseSquareRoot on a complex Hermitian and on a real symmetric positive definite band (N = NTPOLY_AMD_PANEL_N,
          default 4096)
products: inside one session (nt.solver_session) C = T B and C = B T with a thin complex T, three columns of which -- all in
          the panel of the last rank -- list 65, 130 and 200 entries
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LONG = ((0.70, 65), (0.80, 130), (0.90, 200))   # (position as a fraction of the dimension, entries)


def thin_triplets(n, seed):
    """all columns of the thin operand (every rank generates the same): a diagonal plus about two entries per column within
    reach 4 of it, and the long columns"""
    rng = np.random.default_rng(seed)
    j = np.arange(1, n + 1)
    cols, rows = [j], [j]
    for _ in range(2):
        off = rng.integers(1, 5, n) * rng.choice([-1, 1], n)
        ok = (j + off >= 1) & (j + off <= n)
        cols.append(j[ok])
        rows.append((j + off)[ok])
    for (frac, m) in LONG:
        cj = int(frac * n)
        cols.append(np.full(m, cj))
        rows.append(np.arange(cj - m // 2, cj - m // 2 + m))
    col, row = np.concatenate(cols), np.concatenate(rows)
    key = np.unique(col.astype(np.int64) * (n + 1) + row)
    col, row = (key // (n + 1)).astype(np.int32), (key % (n + 1)).astype(np.int32)
    val = np.where(col == row, 1.0, 0.05) * (rng.uniform(0.5, 1.5, len(col)) + 1j * rng.uniform(-0.7, 0.7, len(col)))
    return col, row, val


def main():
    out = sys.argv[1]
    mode = sys.argv[2] if len(sys.argv) > 2 else "loops"
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    n = int(os.environ.get("NTPOLY_AMD_PANEL_N", "4096"))
    import ntpoly_amd as nt
    from gen import banded_triplets
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    for kv in filter(None, os.environ.get("NTPOLY_AMD_TEST_OPTIONS", "").split(",")):   # (name=value,...: options of this run)
        k, v = kv.split("=")
        nt.set_option(k, int(v))
    res = {}

    def fill(col, row, val, cplx):
        M = nt.Matrix_ps(n)
        c0, c1 = M.local_columns()
        k = (col - 1 >= c0) & (col - 1 < c1) & (val != 0)   # (no stored zeros: slab form does not hold them)
        t = nt.TripletList_c() if cplx else nt.TripletList_r()
        t.set_arrays(col[k], row[k], val[k])
        M.FillFromTripletList(t, prepartitioned=True)
        return M

    def keep(tag, M):
        c, r, v = M.triplets()
        res[tag + "_col"], res[tag + "_row"], res[tag + "_val"] = c, r, v

    def counted(tag, fn):
        p0, t0 = nt.panel_product_counts(), nt.thin_slab_counts()
        fn()
        p1, t1 = nt.panel_product_counts(), nt.thin_slab_counts()
        res[tag + "_panel"] = np.array([p1[k] - p0[k] for k in ("slab", "declined", "host_syncs")])
        res[tag + "_thin"] = np.array([t1[k] - t0[k] for k in ("real_left", "real_right", "complex_left", "complex_right", "panel_real",
                                                               "panel_complex")])

    if mode == "products":
        B = fill(*banded_triplets(n, 20, complex_=True, shift=0.37), True)
        T = fill(*thin_triplets(n, 5), True)
        for tag, X, Y in (("tb", T, B), ("bt", B, T)):
            Cm = nt.Matrix_ps(n)

            def product():
                with nt.solver_session(True):
                    Cm.Gemm(X, Y, None, -0.5, 0.0, 1e-8)
            counted(tag, product)
            keep(tag, Cm)
    else:
        p = nt.SolverParameters()
        p.SetThreshold(1e-8)
        p.SetConvergeDiff(1e-7)
        for tag, cplx in (("isq_c", True), ("isq_r", False)):
            S = fill(*banded_triplets(n, 20, complex_=cplx, shift=3.0), cplx)
            Om = nt.Matrix_ps(n)
            counted(tag, lambda: nt.SquareRootSolvers.InverseSquareRoot(S, Om, p))
            tr = nt.solver_trace()
            res[tag + "_iters"] = np.array([tr["iterations"]])
            keep(tag, Om)
            del Om
    np.savez(out + ".%d.npz" % rank, **res)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
