#!/usr/bin/env python3
"""Complex operands without runs across ranks, solved in the pattern's block order (csrc/band_scope.cpp, option
block_scope_complex), measured in ONE process through a 1-rank RCCL communicator (NTPOLY_AMD_FORCE_RCCL=1: the scope, the
gathers and every panel product take the several-rank code; nothing has to travel) -- the method of profiles/README.md item 91.
Input: the complex Hermitian 48^3 lattice (the hermitian() construction of tests/test_gpu_block_complex.py on gen.lattice_triplets),
threshold 1e-8; SignFunction of H, InverseSquareRoot of H + 2.5 I (positive definite).  Three configurations, each in a fresh
child process:

  scope_1    1-rank RCCL communicator, block_scope_complex = 1 (block order, panel products on k_bs_numeric_c)
  scope_0    1-rank RCCL communicator, block_scope_complex = 0 (the gathered operand on the complex LDS hash, as before)
  one_rank   no communicator: the complex session of one rank (iterates in block form)

Each child runs every solve once untimed, then --reps timed solves; milliseconds per iteration from a host clock around a
solve that ends in a device synchronise (best of the repetitions).  Then one more solve with option time_kernels: the SpGEMM
calls' device time inside the numeric kernel and in the whole call (conversions to and from tiles included), against the
solve's wall time.  Prints one JSON line.

    python tools/bench_complex_block_scope.py [--L 48] [--reps 2]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"scope_1": ("1", "1"), "scope_0": ("1", "0"), "one_rank": ("0", "1")}   # (FORCE_RCCL, block_scope_complex)


def hermitian(trip, phase=0.1):
    c, r, v = trip
    return c, r, v * np.exp(1j * phase * (r.astype(np.float64) - c.astype(np.float64)))


def child(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ntpoly_amd as nt
    from gen import lattice_triplets
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("spgemm_fma", 1)
    nt.set_option("block_scope_complex", args.block_scope_complex)
    n = args.L ** 3
    out = {}
    for solver, shift in (("sign", 0.0), ("inverse_square_root", 2.5)):
        H = nt.Matrix_ps.from_triplets(n, *hermitian(lattice_triplets(args.L, shift=shift)))

        def solve():
            p = nt.SolverParameters()
            p.SetThreshold(args.threshold)
            p.SetConvergeDiff(1e-7)
            O = nt.Matrix_ps(n)
            nt.synchronize()
            k0 = nt.block_scope_counts()
            t0 = time.perf_counter()
            if solver == "sign":
                nt.SignSolvers.ComputeSign(H, O, p)
            else:
                nt.SquareRootSolvers.InverseSquareRoot(H, O, p)
            nt.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            k1 = nt.block_scope_counts()
            it = nt.solver_trace()["iterations"]
            print("  %s: %d iterations, %.1f ms" % (solver, it, ms), file=sys.stderr, flush=True)   # (progress of a long child)
            return ms / max(1, it), it, k1["solves"] - k0["solves"], k1["products"] - k0["products"], ms

        solve()   # (untimed: first launches, allocator pools, the block order)
        runs = [solve() for _ in range(args.reps)]
        best = min(runs)
        nt.set_option("time_kernels", 1)
        nt.reset_spgemm_accum()
        timed = solve()
        acc = nt.spgemm_accum()
        nt.set_option("time_kernels", 0)
        calls = max(1, acc["calls"])
        out[solver] = dict(ms_per_iter=round(best[0], 3), iterations=best[1], scope_solves=best[2], scope_products=best[3],
                           all_ms_per_iter=[round(r[0], 3) for r in runs],
                           timed=dict(spgemm_calls=acc["calls"], ms_numeric_per_call=round(acc["ms_numeric"] / calls, 3),
                                      ms_spgemm_per_call=round(acc["ms_total"] / calls, 3), ms_wall_per_call=round(timed[4] / calls, 3),
                                      share_outside_numeric_of_spgemm=round(1.0 - acc["ms_numeric"] / max(1e-9, acc["ms_total"]), 3),
                                      share_outside_numeric_of_wall=round(1.0 - acc["ms_numeric"] / max(1e-9, timed[4]), 3)))
        del H
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=48)
    ap.add_argument("--threshold", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--configs", default="scope_1,scope_0,one_rank")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--block-scope-complex", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per configuration")
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    res = {}
    for name in args.configs.split(","):
        force, bsc = CONFIGS[name]
        env = dict(os.environ, NTPOLY_AMD_FORCE_RCCL=force)
        env.pop("NTPOLY_AMD_COMM", None)
        env.pop("NTPOLY_AMD_BLOCK_SCOPE_COMPLEX", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--block-scope-complex", bsc, "--L", str(args.L),
               "--threshold", str(args.threshold), "--reps", str(args.reps)]
        print("%s:" % name, file=sys.stderr, flush=True)
        try:
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, cwd=ROOT, timeout=args.timeout)
        except subprocess.TimeoutExpired:   # (the child is killed; nothing more is started on the device)
            res[name] = {"error": "timeout after %d s" % args.timeout}
            break
        if r.returncode != 0:   # (a failed configuration ends the run: nothing more is started on the device)
            sys.stderr.write(r.stdout[-2000:])
            res[name] = {"error": r.returncode}
            break
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
        print("%s: %s" % (name, res[name]), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
