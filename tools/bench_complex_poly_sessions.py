#!/usr/bin/env python3
"""Complex sessions of the polynomial and function families (option complex_poly_sessions), measured on configs[4]'s operand: the
complex Hermitian band H, N = 131 072, h = 50, threshold 1e-8.  Two workloads per block: ComputeExponential(-H) and a degree-16
Chebyshev polynomial of 0.4 H (spectral radius below 1).  (-H: the dominant eigenvalue of H is negative, about -1.75, PowerBounds'
estimate for it is negative too, and ComputeExponential(H) -- as the reference's -- then squares nothing; the estimate for -H is 2.8:
sigma = 4, two squarings behind the degree-15 fit.)  The generator's 131 diagonal entries that are exactly zero are not stored:
complex slab form cannot hold a stored zero, and an input with stored zeros has every product that reads it refused -- after five
refusals the session gives up and the evaluation runs on compressed columns whatever the option says (--stored-zeros 1 measures that).
With option stored_zero_views (--views 1, the default of the library) such an input enters the session as a read-only view instead;
--views 0 is the behaviour without views, and --views -1 leaves the option alone (a library built before the option existed,
NTPOLY_AMD_LIB).  The views' counters are reported where the library has them.

ONE configuration per invocation, in this process -- the caller runs the six lines (option 0, 1, 2; one rank, and a 1-rank RCCL
communicator: every collective of a panel product a real RCCL call, nothing has to travel) one after the other, each under its
own time limit, and stops at the first that fails:

    for rccl in 0 1; do for opt in 0 1 2; do
      timeout -k 10 900 python tools/bench_complex_poly_sessions.py --option $opt --rccl $rccl || break 2
    done; done

The block and median scheme of DESIGN.md section 6: one untimed warm-up block, then --blocks timed blocks (a block = each workload
once, a host clock around a call that ends in a device synchronise); the MEDIAN block is reported per workload, all blocks are
listed.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--option", type=int, choices=(0, 1, 2), required=True, help="complex_poly_sessions")
    ap.add_argument("--rccl", type=int, choices=(0, 1), default=0, help="1: through a 1-rank RCCL communicator")
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--h", type=int, default=50)
    ap.add_argument("--threshold", type=float, default=1e-8)
    ap.add_argument("--degree", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--stored-zeros", type=int, choices=(0, 1), default=0, help="1: keep the generator's zero-valued diagonal entries")
    ap.add_argument("--views", type=int, choices=(-1, 0, 1), default=-1, help="stored_zero_views; -1: leave the library's own setting")
    args = ap.parse_args()
    os.environ["NTPOLY_AMD_FORCE_RCCL"] = str(args.rccl)
    os.environ.pop("NTPOLY_AMD_COMM", None)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ntpoly_amd as nt
    from gen import banded_triplets
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("spgemm_fma", 1)
    nt.set_option("complex_poly_sessions", args.option)
    if args.views >= 0:
        nt.set_option("stored_zero_views", args.views)
    have_views = hasattr(nt.lib, "ntpoly_amd_slab_view_counts")
    n = args.n
    col, row, val = banded_triplets(n, args.h, complex_=True)
    if not args.stored_zeros:
        col, row, val = col[val != 0], row[val != 0], val[val != 0]
    Hn = nt.Matrix_ps.from_triplets(n, col, row, -val)
    Hs = nt.Matrix_ps.from_triplets(n, col, row, 0.4 * val)
    poly = nt.ChebyshevPolynomial(args.degree + 1)
    for k in range(args.degree + 1):
        poly.SetCoefficient(k, 0.8 / (1 + k) * (-1) ** k)
    p = nt.SolverParameters()
    p.SetThreshold(args.threshold)
    work = {"exponential": lambda O: nt.ExponentialSolvers.ComputeExponential(Hn, O, p),
            "chebyshev%d" % args.degree: lambda O: poly.Compute(Hs, O, p)}

    def timed(fn):
        O = nt.Matrix_ps(n)
        nt.synchronize()
        s0, q0 = nt.slab_algebra_counts(), nt.panel_product_counts()
        v0 = nt.slab_view_counts() if have_views else {}
        t0 = time.perf_counter()
        fn(O)
        nt.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        s1, q1 = nt.slab_algebra_counts(), nt.panel_product_counts()
        v1 = nt.slab_view_counts() if have_views else {}
        return ms, {k: s1[k] - s0[k] for k in s0}, q1["slab"] - q0["slab"], O.GetSize(), {k: v1[k] - v0[k] for k in v0}

    out = {"option": args.option, "rccl": args.rccl, "n": n, "h": args.h, "threshold": args.threshold, "blocks": args.blocks,
           "stored_zeros": args.stored_zeros, "views": nt.get_option("stored_zero_views") if have_views else None,
           "library": os.environ.get("NTPOLY_AMD_LIB", "")}
    for name, fn in work.items():
        timed(fn)   # (untimed: first launches, allocator pools)
    blocks = {name: [] for name in work}
    last = {}
    for _ in range(args.blocks):
        for name, fn in work.items():
            ms, slab, panel, nnz, views = timed(fn)
            blocks[name].append(ms)
            last[name] = (slab, panel, nnz, views)
    for name in work:
        out[name] = dict(ms=round(statistics.median(blocks[name]), 3), blocks_ms=[round(x, 3) for x in blocks[name]],
                         slab_operations=last[name][0], panel_products=last[name][1], nnz=last[name][2], view_operations=last[name][3])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
