#!/usr/bin/env python3
"""Complex TRS2 with its iterate kept out of compressed columns (complex_density = 1, csrc/psmatrix.cpp complex_trs2_step: complex
slab form for run-like iterates -- X*X on the complex tile kernel, then the merge pass, then one energy / trace pass -- and complex
block form for iterates without runs) against the compressed-column path (complex_density = 0), on configs[4]'s operand
(Hermitian complex banded N = 131 072, h = 50, nel = N / 2) and on a complex Hermitian 48^3 lattice (block form under the
automatic rule); the real TRS2 at the same N as a yardstick.  The two settings alternate in one process; each configuration
runs one untimed solve first.  Milliseconds per iteration from a host clock around each solve, ending in a device synchronise;
prints one JSON line."""
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
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--h", type=int, default=50)
    ap.add_argument("--lattice", type=int, default=48, help="0: no lattice workload")
    ap.add_argument("--settings", default="1,0", help="complex_density values, alternated in this order")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=1e-8)
    args = ap.parse_args()
    import ntpoly_amd as nt
    from gen import banded_triplets, lattice_triplets
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("spgemm_fma", 1)
    nt.set_option("complex_tile", 1)
    nt.set_option("complex_sessions", 1)
    settings = [int(x) for x in args.settings.split(",")]

    def solve(H, n):
        p = nt.SolverParameters()
        p.SetThreshold(args.threshold)
        p.SetConvergeDiff(1e-10)
        I = nt.Matrix_ps(n)
        I.FillIdentity()
        K = nt.Matrix_ps(n)
        nt.synchronize()
        t0 = time.perf_counter()
        nt.DensityMatrixSolvers.TRS2(H, I, n / 2.0, K, p)
        nt.synchronize()
        return (time.perf_counter() - t0) * 1e3, nt.solver_trace()["iterations"]

    work = []
    c, r, v = banded_triplets(args.n, args.h, complex_=True)
    work.append(("trs2_complex_banded_%d" % args.n, args.n, (c, r, v), settings))
    if args.lattice:
        L = args.lattice
        c, r, v = lattice_triplets(L)
        work.append(("trs2_complex_lattice_%d" % L, L ** 3, (c, r, v * np.exp(0.1j * (r.astype(np.float64) - c.astype(np.float64)))), settings))
    c, r, v = banded_triplets(args.n, args.h)
    work.append(("trs2_real_banded_%d" % args.n, args.n, (c, r, v), settings[:1]))
    out = {}
    for key, n, trip, sets in work:
        H = nt.Matrix_ps.from_triplets(n, *trip)
        for s in sets:   # (untimed: caches, the kernels' first launches)
            nt.set_option("complex_density", s)
            solve(H, n)
        rec = {s: [] for s in sets}
        for _ in range(args.reps):
            for s in sets:
                nt.set_option("complex_density", s)
                c0 = nt.complex_fusion_counts()
                ms, it = solve(H, n)
                c1 = nt.complex_fusion_counts()
                rec[s].append((ms / max(1, it), it, c1["square"] + c1["update"] - c0["square"] - c0["update"]))
        out[key] = {("complex_density_%d" % s): dict(ms_per_iter=round(min(x[0] for x in rec[s]), 3), iterations=rec[s][0][1],
                                                     steps_out_of_columns=rec[s][0][2]) for s in sets}
        print("%s: %s" % (key, out[key]), file=sys.stderr, flush=True)
        del H
    nt.set_option("complex_density", 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
