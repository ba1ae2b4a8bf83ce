#!/usr/bin/env python3
"""PM purification with its iterate kept in slab form (option pm_session), measured: a PM solve on the headline operand -- the
banded Hamiltonian of bench.py, N = 262 144, h = 100, threshold 1e-8, ISQ = I, trace = N / 2 -- for a fixed 20 iterations in FMA
arithmetic, option 0 (the loop on compressed columns: two products expanded and packed back, three merges, three reductions per
iteration) against option 1 (the session: products in slab form, one sigma pass, one update pass, the stored zeros in a list).

The block and median scheme of DESIGN.md section 6: one untimed warm-up block, then --blocks timed blocks; a block = the solve
once with each option.  The figure is the solver's own loop time (solver_trace loop_ms: host clock from the first iteration to the
end of the last, ending in a device synchronise) per iteration; the MEDIAN block is reported per option, all blocks are listed,
the spread is (max - min) / median.  One more block per option runs with the engine's event timers on (option time_kernels) and
gives the kernel share: time inside the SpGEMM numeric launches / loop time.  With option 1 the counters say how many stored
zeros were carried (summed over the updates) and how long the list grew.  Prints one JSON line per option and writes them to
--out when given:

    timeout -k 10 900 python tools/bench_pm_session.py --out profiles/pm_session_bench.json

--no-option: a library that does not know the option (the commit before it) is measured the same way, one line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--h", type=int, default=100)
    ap.add_argument("--threshold", type=float, default=1e-8)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--no-option", action="store_true", help="the library does not know pm_session: one line, labelled 'parent'")
    ap.add_argument("--out", default="", help="file the JSON lines are written to (replaced)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ntpoly_amd as nt
    from gen import banded_triplets
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("spgemm_fma", 1)
    n = args.n
    H = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, args.h))
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    options = [None] if args.no_option else [0, 1]

    def solve(opt, timers=False):
        if opt is not None:
            nt.set_option("pm_session", opt)
        nt.set_option("time_kernels", 1 if timers else 0)
        p = nt.SolverParameters()
        p.SetThreshold(args.threshold)
        p.SetConvergeDiff(1e-30)
        p.SetMaxIterations(args.iterations)
        p.SetMonitorConvergence(False)
        K = nt.Matrix_ps(n)
        c0 = nt.pm_session_counts() if opt is not None else None
        nt.reset_spgemm_accum()
        e = nt.DensityMatrixSolvers.PM(H, I, n / 2.0, K, p)
        nt.synchronize()
        acc = nt.spgemm_accum()
        tr = nt.solver_trace()
        c1 = nt.pm_session_counts() if opt is not None else None
        counts = {k: c1[k] - c0[k] for k in c1} if c1 else {}
        return dict(loop_ms=tr["loop_ms"], setup_ms=tr["setup_ms"], iters=tr["iterations"], energy=e[0] if isinstance(e, tuple) else e,
                    nnz=[int(v) for v in tr["nnz"]], sigma=[float(v) for v in tr["sigma"]], kernel_ms=acc["ms_numeric"], counts=counts)

    for opt in options:
        solve(opt)   # (untimed: first launches, allocator pools, kept transposes)
    runs = {opt: [] for opt in options}
    for _ in range(args.blocks):
        for opt in options:
            runs[opt].append(solve(opt))
    lines = []
    for opt in options:
        timed = solve(opt, timers=True)
        per = [r["loop_ms"] / r["iters"] for r in runs[opt]]
        med = statistics.median(per)
        last = runs[opt][-1]
        lines.append(json.dumps(dict(
            workload="PM solve, banded N=%d halfband=%d, threshold=%g, ISQ=I, trace=N/2, %d iterations, FMA arithmetic" % (
                n, args.h, args.threshold, args.iterations),
            pm_session="parent" if opt is None else opt, blocks=args.blocks, iterations=last["iters"],
            ms_per_iteration=round(med, 3), blocks_ms_per_iteration=[round(x, 3) for x in per],
            spread=round((max(per) - min(per)) / med, 4), setup_ms=round(statistics.median(r["setup_ms"] for r in runs[opt]), 1),
            kernel_share=round(timed["kernel_ms"] / timed["loop_ms"], 3), kernel_ms_per_iteration=round(timed["kernel_ms"] / timed["iters"], 3),
            loop_ms_with_timers_per_iteration=round(timed["loop_ms"] / timed["iters"], 3),
            energy=last["energy"], nnz_end=last["nnz"][-1], sigma_first=round(last["sigma"][0], 6), sigma_last=round(last["sigma"][-1], 6),
            counts=last["counts"], zeros_carried=last["counts"].get("zeros"),
            longest_zero_list=nt.pm_session_longest_list() if opt == 1 else None)))
    for ln in lines:
        print(ln)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
