#!/usr/bin/env python3
"""Complex solver loops with their iterates in block form (complex_sessions = 1: products, merges, scalings, copies and
norms on complex tiles, csrc/spgemm_block.hip) against the same loops with every product converted back to compressed
columns (complex_sessions = 0): SignFunction (shift 0) and InverseSquareRoot (shift 2.5) on complex Hermitian L^3 lattices,
which take the block path under the automatic rule.  The two settings alternate in one process; each configuration runs
one untimed solve first (after drop_block_caches).  Milliseconds per iteration from a host clock around each solve,
ending in a device synchronise; prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", default="32,48")
    ap.add_argument("--solvers", default="sign,inverse_square_root")
    ap.add_argument("--settings", default="1,0", help="complex_sessions values, alternated in this order")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=1e-6)
    args = ap.parse_args()
    import ntpoly_amd as nt
    from gen import lattice_triplets
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("spgemm_fma", 1)
    nt.set_option("complex_tile", 1)
    nt.set_option("block_complex", 1)
    nt.set_option("block_path", 1)
    nt.set_option("slab_algebra", 1)
    settings = [int(x) for x in args.settings.split(",")]

    def solve(solver, H, n):
        p = nt.SolverParameters()
        p.SetThreshold(args.threshold)
        p.SetConvergeDiff(1e-7)
        Out = nt.Matrix_ps(n)
        nt.synchronize()
        t0 = time.perf_counter()
        if solver == "sign":
            nt.SignSolvers.ComputeSign(H, Out, p)
        else:
            nt.SquareRootSolvers.InverseSquareRoot(H, Out, p)
        nt.synchronize()
        return (time.perf_counter() - t0) * 1e3, nt.solver_trace()["iterations"]

    out = {}
    for L in (int(x) for x in args.lattices.split(",")):
        n = L ** 3
        for solver in args.solvers.split(","):
            c, r, v = lattice_triplets(L, shift=0.0 if solver == "sign" else 2.5)
            H = nt.Matrix_ps.from_triplets(n, c, r, v * np.exp(0.1j * (r.astype(np.float64) - c.astype(np.float64))))
            for s in settings:   # (untimed: the block order, the caches, the kernels' first launches)
                nt.set_option("complex_sessions", s)
                nt.drop_block_caches()
                solve(solver, H, n)
            rec = {s: [] for s in settings}
            for _ in range(args.reps):
                for s in settings:
                    nt.set_option("complex_sessions", s)
                    c0 = nt.block_algebra_counts()["operations"]
                    ms, it = solve(solver, H, n)
                    rec[s].append((ms / max(1, it), it, nt.block_algebra_counts()["operations"] - c0))
            key = "%s_%d" % (solver, L)
            out[key] = {("session_%d" % s): dict(ms_per_iter=min(x[0] for x in rec[s]), iterations=rec[s][0][1],
                                                 block_ops_per_solve=rec[s][0][2]) for s in settings}
            print("%s: %s" % (key, out[key]), file=sys.stderr, flush=True)
    nt.set_option("complex_sessions", 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
