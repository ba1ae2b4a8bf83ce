#!/usr/bin/env python3
"""Child process of tests/test_gpu_cg_dots.py (option cg_dots).

    python tests/cg_dots_worker.py ranks <out-prefix>
        one rank of the several-ranks test: RANK / WORLD_SIZE / NTPOLY_AMD_COMM come from the environment, the ranks share ONE GPU
        and exchange through the shared-memory test transport.  CGSolver on the first solve of the one-rank test (n = 257) and on
        n = 5, in both arithmetic modes, with the option at 0 and at 1; per case the digest of the local panel of X (the sum of its
        value bits modulo 2^64 plus its entry count), the growth of the counters, and the panel's triplets (<out-prefix>.<rank>.npz).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name: (n, h, threshold, converge_diff, max_iterations)
CASES = {"solve257": (257, 24, 1e-5, 1e-30, 8), "n5": (5, 2, 0.0, 1e-30, 3)}
SLOTS = ("solves", "passes", "refused", "not_formed")


def panel(nt, n, triplets_of):
    """the matrix from this rank's own columns"""
    A = nt.Matrix_ps(n)
    c0, c1 = A.local_columns()
    col, row, val = triplets_of(c0, c1)
    t = nt.TripletList_r()
    t.set_arrays(col, row, val)
    A.FillFromTripletList(t, prepartitioned=True)
    return A, c1 - c0


def digest(val):
    b = np.ascontiguousarray(val, dtype=np.float64).view(np.uint64)
    return int((int(np.sum(b, dtype=np.uint64)) + len(b)) % (1 << 64))


def ranks(out):
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    import ntpoly_amd as nt
    from gen import banded_triplets
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    res, arrays = {}, {}
    for name, (n, h, thr, conv, maxit) in CASES.items():
        A, width = panel(nt, n, lambda c0, c1: banded_triplets(n, h, shift=2.5, c0=c0, c1=c1))
        B, _ = panel(nt, n, lambda c0, c1: banded_triplets(n, max(2, h // 3), shift=0.5, c0=c0, c1=c1))
        res[name + "_width"] = int(width)
        p = nt.SolverParameters()
        p.SetThreshold(thr)
        p.SetConvergeDiff(conv)
        p.SetMaxIterations(maxit)
        p.SetMonitorConvergence(False)
        for arith, mode in (("fma", 1), ("unfused", 0)):
            nt.set_option("spgemm_fma", mode)
            for opt in (0, 1):
                nt.set_option("cg_dots", opt)
                X = nt.Matrix_ps(n)
                before = nt.cg_dots_counts()
                nt.LinearSolvers.CGSolver(A, X, B, p)
                after = nt.cg_dots_counts()
                col, row, val = X.triplets()
                key = "%s_%s_%d" % (name, arith, opt)
                res[key] = dict(digest=digest(val), entries=int(len(val)), counts=[after[k] - before[k] for k in SLOTS])
                for what, a in (("col", col), ("row", row), ("val", val)):
                    arrays[key + "_" + what] = a
    np.savez(out + ".%d.npz" % rank, **arrays)
    with open(out + ".%d.json" % rank, "w") as f:
        json.dump(res, f)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    ranks(sys.argv[2])
