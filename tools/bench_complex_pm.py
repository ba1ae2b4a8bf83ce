#!/usr/bin/env python3
"""Complex PM in a complex slab session (option complex_pm), measured on configs[4]'s operand (tests/gen.py
banded_triplets(131072, 50, complex_=True)), FMA arithmetic, threshold 1e-8, 20 iterations, convergence monitor off, trace N / 2.

Three legs: option 1 (the loop's matrices in complex slab form with the rows of stored zeros in a list; sigma's trace and dot from
one pass, the scaling and both merges from another, the energy from a third), option 0 (compressed columns between the operations:
two products, copy, merge, trace and dot for sigma, scaling and two merges for the update, one more dot) and -- with --parent-root
DIR, a built checkout of the parent commit -- the parent's library, which does not know the option.  Each leg runs in a process of
its own, which imports the package (from DIR for the parent), builds the same operand once and then runs one solve per line it is
sent; it idles while another leg measures.  The block scheme of DESIGN.md section 6: one untimed warm-up block, then --blocks
timed blocks; a block = the solve once with each leg, in turn, so that whatever else the machine does meets all three alike.  Every
leg calls the solver through the C ABI (PM_wrp).

The figure is a host clock around the whole solver call, which ends in a device synchronise, divided by the iteration count
(set-up and the epilogue are inside, the same for every leg).  Per leg the MEDIAN block is reported, all blocks are listed,
spread = (max - min) / median.  One more solve per option runs with the engine's event timers on (time_kernels) and gives the
share of the call inside the SpGEMM numeric launches.  The last line states the medians' ratios and whether option 1 is faster
than option 0 and than the parent by more than the largest of the three spreads; it promises no ratio and decides no default.
Prints JSON lines and writes them to --out when given:

    timeout -k 10 900 python tools/bench_complex_pm.py --parent-root /path/to/parent --out profiles/complex_pm_bench.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("spgemm_fma", 1)
    return nt


def operand(nt, args):
    from gen import banded_triplets
    H = nt.Matrix_ps.from_triplets(args.n, *banded_triplets(args.n, args.h, complex_=True))
    I = nt.Matrix_ps(args.n)
    I.FillIdentity()
    return H, I


def solve(nt, args, H, I, opt, timers=False):
    if opt is not None:
        nt.set_option("complex_pm", opt)
    nt.set_option("time_kernels", 1 if timers else 0)
    p = nt.SolverParameters()
    p.SetThreshold(args.threshold)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(args.iterations)
    p.SetMonitorConvergence(False)
    K = nt.Matrix_ps(args.n)
    e, mu = C.c_double(), C.c_double()
    c0 = nt.complex_pm_counts() if opt is not None else None
    s0 = nt.slab_algebra_counts()
    nt.reset_spgemm_accum()
    nt.synchronize()
    t0 = time.perf_counter()
    nt.lib.PM_wrp(H.ih, I.ih, C.byref(C.c_double(args.n / 2.0)), K.ih, C.byref(e), C.byref(mu), p.ih)
    nt.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    acc = nt.spgemm_accum()
    tr = nt.solver_trace()
    c1 = nt.complex_pm_counts() if opt is not None else None
    s1 = nt.slab_algebra_counts()
    return dict(ms=ms, iters=int(tr["iterations"]), loop_ms=float(tr["loop_ms"]), kernel_ms=float(acc["ms_numeric"]),
                energy=float(e.value), nnz_end=int(tr["nnz"][-1]), sigma_first=float(tr["sigma"][0]), sigma_last=float(tr["sigma"][-1]),
                counts={k: c1[k] - c0[k] for k in c1} if c1 else None, slab={k: int(s1[k] - s0[k]) for k in s1})


def serve(args):
    """one leg: one solve per line on stdin ("solve" or "timed"), one JSON line back; ends at end of input"""
    nt = load(args.root)
    H, I = operand(nt, args)
    opt = None if args.serve_option < 0 else args.serve_option   # (the parent's library does not know the option)
    print(json.dumps(dict(ready=True)), flush=True)
    for line in sys.stdin:
        if not line.strip():
            break
        print(json.dumps(solve(nt, args, H, I, opt, timers=line.strip() == "timed")), flush=True)


class Leg:
    """a child process that measures one leg; it idles while the others measure"""

    def __init__(self, args, name, root, option):
        self.name = name
        # (a time limit of its own: a child that hangs ends, and the blocking read below then sees the end of its output)
        self.p = subprocess.Popen(["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--serve",
                                   "--serve-option", str(option), "--root", os.path.abspath(root), "--n", str(args.n), "--h", str(args.h),
                                   "--threshold", repr(args.threshold), "--iterations", str(args.iterations)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def line(self):
        while True:
            ln = self.p.stdout.readline()
            if not ln:
                raise RuntimeError("the process of leg %s ended early (exit code %s)" % (self.name, self.p.poll()))
            if ln.startswith("{"):
                return json.loads(ln)

    def run(self, timers=False):
        self.p.stdin.write("timed\n" if timers else "solve\n")
        self.p.stdin.flush()
        return self.line()

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=120)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--h", type=int, default=50)
    ap.add_argument("--threshold", type=float, default=1e-8)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--options", type=int, nargs="+", default=[1, 0], choices=[0, 1], help="the option's values measured, in block order")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit: measured as a third leg")
    ap.add_argument("--child-timeout", type=int, default=800, help="seconds after which a leg's process is ended")
    ap.add_argument("--out", default="", help="file the JSON lines are written to (replaced)")
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--serve-option", type=int, default=-1, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        return serve(args)
    legs = list(dict.fromkeys(args.options)) + (["parent"] if args.parent_root else [])
    procs = {}
    lines, medians, spreads = [], {}, {}
    try:
        for v in legs:   # (one after the other: each builds its operand while nothing is being timed)
            procs[v] = Leg(args, str(v), args.parent_root if v == "parent" else ROOT, -1 if v == "parent" else v)
            procs[v].line()   # (ready)
        for v in legs:
            procs[v].run()   # (untimed: first launches, allocator pools, the operand cache)
        runs = {v: [] for v in legs}
        for _ in range(args.blocks):
            for v in legs:
                runs[v].append(procs[v].run())
        for v in legs:
            per = [r["ms"] / r["iters"] for r in runs[v]]
            med = statistics.median(per)
            last = runs[v][-1]
            timed = procs[v].run(timers=True)
            medians[v], spreads[v] = med, (max(per) - min(per)) / med
            lines.append(json.dumps(dict(
                workload="PM: complex banded N=%d halfband=%d, threshold=%g, trace N/2, %d iterations, monitor off, FMA arithmetic" % (
                    args.n, args.h, args.threshold, args.iterations),
                complex_pm=v, blocks=args.blocks, iterations=last["iters"], ms_per_iteration=round(med, 3),
                blocks_ms_per_iteration=[round(x, 3) for x in per], spread=round(spreads[v], 4),
                call_ms=round(statistics.median(r["ms"] for r in runs[v]), 2),
                loop_ms_per_iteration=round(statistics.median(r["loop_ms"] / r["iters"] for r in runs[v]), 3),
                kernel_share=round(timed["kernel_ms"] / timed["ms"], 3), kernel_ms_per_iteration=round(timed["kernel_ms"] / timed["iters"], 3),
                energy=last["energy"], nnz_end=last["nnz_end"], sigma_first=last["sigma_first"], sigma_last=last["sigma_last"],
                complex_pm_counts=last["counts"], slab_algebra_counts=last["slab"])))
    finally:
        for leg in procs.values():
            leg.close()
    spread = max(spreads[v] for v in legs)
    summary = dict(summary="medians compared; the option's default is 0 whatever these say", largest_spread=round(spread, 4),
                   parent_measured="parent" in medians)
    if 0 in medians and "parent" in medians:
        summary["option_0_over_parent"] = round(medians[0] / medians["parent"] - 1.0, 4)
        summary["option_0_equals_parent_within_spread"] = bool(abs(medians[0] - medians["parent"]) / medians["parent"] <= spread)
    if 1 in medians:
        gains = {str(v): round((medians[v] - medians[1]) / medians[v], 4) for v in legs if v != 1}
        summary["gain_of_1_over"] = gains
        summary["option_1_faster_than_all_by_more_than_the_spread"] = bool(gains and all(g > spread for g in gains.values()))
    lines.append(json.dumps(summary))
    for ln in lines:
        print(ln)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
