#!/usr/bin/env python3
"""Complex slab sessions across ranks, measured in ONE process through a 1-rank RCCL communicator (NTPOLY_AMD_FORCE_RCCL=1: every
collective of a panel product is a real RCCL call, nothing has to travel) -- the method of profiles/README.md item 91.
configs[4]: SignFunction of the complex Hermitian band H and InverseSquareRoot of H + 2 I, N = 131 072, h = 50, threshold 1e-8.
Three configurations, each in a fresh child process:

  panels_1   1-rank RCCL communicator, complex_panels = 1 (complex column panels in slab form, complex tile kernel)
  panels_0   1-rank RCCL communicator, complex_panels = 0 (every complex product on compressed columns, as before)
  one_rank   no communicator: the complex session of one rank

Each child runs every solve once untimed, then --reps timed solves; milliseconds per iteration from a host clock around a
solve that ends in a device synchronise (best of the repetitions).  Prints one JSON line.

    python tools/bench_complex_panel_sessions.py [--n 131072] [--reps 2]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"panels_1": ("1", "1"), "panels_0": ("1", "0"), "one_rank": ("0", "1")}   # (FORCE_RCCL, complex_panels)


def child(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ntpoly_amd as nt
    from gen import banded_triplets
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("spgemm_fma", 1)
    nt.set_option("complex_panels", args.complex_panels)
    n = args.n
    out = {}
    for solver, shift in (("sign", 0.0), ("inverse_square_root", 2.0)):
        H = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, args.h, complex_=True, shift=shift))

        def solve():
            p = nt.SolverParameters()
            p.SetThreshold(args.threshold)
            p.SetConvergeDiff(1e-7)
            O = nt.Matrix_ps(n)
            nt.synchronize()
            c0 = nt.panel_product_counts()
            t0 = time.perf_counter()
            if solver == "sign":
                nt.SignSolvers.ComputeSign(H, O, p)
            else:
                nt.SquareRootSolvers.InverseSquareRoot(H, O, p)
            nt.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            c1 = nt.panel_product_counts()
            it = nt.solver_trace()["iterations"]
            return ms / max(1, it), it, c1["slab"] - c0["slab"], c1["declined"] - c0["declined"]

        solve()   # (untimed: first launches, allocator pools)
        runs = [solve() for _ in range(args.reps)]
        best = min(runs)
        out[solver] = dict(ms_per_iter=round(best[0], 3), iterations=best[1], panel_products=best[2], declined=best[3],
                           all_ms_per_iter=[round(r[0], 3) for r in runs])
        del H
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--h", type=int, default=50)
    ap.add_argument("--threshold", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--configs", default="panels_1,panels_0,one_rank")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--complex-panels", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per configuration")
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    res = {}
    for name in args.configs.split(","):
        force, cp = CONFIGS[name]
        env = dict(os.environ, NTPOLY_AMD_FORCE_RCCL=force)
        env.pop("NTPOLY_AMD_COMM", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--complex-panels", cp, "--n", str(args.n), "--h", str(args.h),
               "--threshold", str(args.threshold), "--reps", str(args.reps)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=args.timeout)
        if r.returncode != 0:   # (a failed configuration ends the run: nothing more is started on the device)
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            res[name] = {"error": r.returncode}
            break
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
        print("%s: %s" % (name, res[name]), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
