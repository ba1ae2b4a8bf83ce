#!/usr/bin/env python3
"""CGSolver with its traces from column dot passes (option cg_dots), measured on the headline operand shifted to be positive
definite (tests/gen.py banded_triplets(262144, 100, shift=2.5)), B = I, threshold 1e-6, six fixed iterations, convergence monitor
off, default (FMA) arithmetic.

Three legs: option 1 (a slab session, one product and two dot passes per iteration), option 0 (four products, three transposes
and three traces per iteration on compressed columns) and -- with --parent-root DIR, a built checkout of the parent commit -- the
parent's library, which does not know the option.  Each leg runs in a process of its own, which imports the package (from DIR for
the parent), builds the same operands once and then runs one call per line it is sent; it idles while another leg measures.  The
block scheme of DESIGN.md section 6: one untimed warm-up block, then --blocks timed blocks; a block = the call once with each
leg, in turn.  Every leg calls the solver through the C ABI (CGSolver_wrp).

The figure is a host clock around the whole call, which ends in a device synchronise, divided by the iterations.  Per leg the
MEDIAN block is reported, all blocks are listed, spread = (max - min) / median.  A leg whose process ends early is recorded as
failed and not tried again.  A fourth process times k_cg_dots alone: one solve with option 1 under option time_kernels with
NTPOLY_AMD_DEBUG_SPGEMM set, in which the library prints every pass's time between two HIP events and the bytes of the runs it
read; the launches with two pairs are reported with bytes / time as a fraction of the 8 TB/s HBM peak.  The last line applies the
rule that decides the default: option 1 if it is faster than option 0 AND than the parent by more than the largest block spread
while option 0 and the parent agree within it; it promises no ratio.
Prints JSON lines and writes them to --out when given:

    timeout -k 10 900 python tools/bench_cg_dots.py --parent-root /path/to/parent --out profiles/cg_dots_bench.json
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0


def load(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


def operands(nt, args):
    from gen import banded_triplets
    A = nt.Matrix_ps.from_triplets(args.n, *banded_triplets(args.n, args.h, shift=2.5))
    B = nt.Matrix_ps(args.n)
    B.FillIdentity()
    return A, B


def solve(nt, args, A, B, opt):
    if opt is not None:
        nt.set_option("cg_dots", opt)
    p = nt.SolverParameters()
    p.SetThreshold(args.threshold)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(args.steps)
    p.SetMonitorConvergence(False)
    X = nt.Matrix_ps(args.n)
    c0 = nt.cg_dots_counts() if opt is not None else None
    nt.synchronize()
    t0 = time.perf_counter()
    nt.lib.CGSolver_wrp(A.ih, X.ih, B.ih, p.ih)
    nt.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    c1 = nt.cg_dots_counts() if opt is not None else None
    return dict(ms=ms, entries=int(X.GetSize()), trace=float(X.Trace()), counts={k: c1[k] - c0[k] for k in c1} if c1 else None)


def serve(args):
    """one leg: one call per line on stdin, one JSON line back; ends at end of input"""
    nt = load(args.root)
    A, B = operands(nt, args)
    nt.synchronize()
    opt = None if args.serve_option < 0 else args.serve_option   # (the parent's library does not know the option)
    print(json.dumps(dict(ready=True)), flush=True)
    for line in sys.stdin:
        if not line.strip():
            break
        print(json.dumps(solve(nt, args, A, B, opt)), flush=True)


def serve_pass(args):
    """k_cg_dots alone: one solve with option 1, every pass between two HIP events"""
    os.environ["NTPOLY_AMD_DEBUG_SPGEMM"] = "1"
    nt = load(args.root)
    A, B = operands(nt, args)
    solve(nt, args, A, B, 1)   # (untimed: first launches, allocator pools)
    nt.set_option("time_kernels", 1)
    nt.synchronize()
    with tempfile.TemporaryFile(mode="w+") as f:   # (the library writes the figures to stderr)
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            for _ in range(args.blocks):
                solve(nt, args, A, B, 1)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read()
    nt.set_option("time_kernels", 0)
    out = {}
    for pairs in (2, 1):
        got = [(float(m.group(1)), float(m.group(2))) for m in re.finditer(r"\[cg dots\] timed: n \d+ pairs %d bytes (\d+) ms ([0-9.]+)" % pairs, text)]
        if got:
            med = statistics.median(g[1] for g in got)
            byts = statistics.median(g[0] for g in got)
            out["pairs_%d" % pairs] = dict(launches=len(got), pass_ms=round(med, 4), pass_ms_min_max=[min(g[1] for g in got), max(g[1] for g in got)],
                                           bytes=int(byts), gbs=round(byts / med / 1e6, 1), hbm_fraction=round(byts / med / 1e6 / HBM_PEAK_GBS, 4))
    print(json.dumps(out), flush=True)


class Leg:
    """a child process that measures one leg; it idles while the others measure"""

    def __init__(self, args, name, root, option, mode="--serve"):
        self.name = name
        self.failed = None
        # (a time limit of its own: a child that hangs ends, and the blocking read below then sees the end of its output)
        self.p = subprocess.Popen(["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), mode,
                                   "--serve-option", str(option), "--root", os.path.abspath(root), "--n", str(args.n), "--h", str(args.h),
                                   "--threshold", repr(args.threshold), "--steps", str(args.steps), "--blocks", str(args.blocks)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def line(self):
        while True:
            ln = self.p.stdout.readline()
            if not ln:
                self.failed = "the process ended early (exit code %s)" % self.p.wait()
                return None
            if ln.startswith("{"):
                return json.loads(ln)

    def run(self):
        if self.failed:
            return None
        try:
            self.p.stdin.write("solve\n")
            self.p.stdin.flush()
        except OSError:
            self.failed = "the process ended early (exit code %s)" % self.p.wait()
            return None
        return self.line()

    def close(self):
        try:
            self.p.stdin.close()
        except OSError:
            pass
        self.p.wait(timeout=120)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--h", type=int, default=100)
    ap.add_argument("--threshold", type=float, default=1e-6)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--options", type=int, nargs="+", default=[1, 0], choices=[0, 1], help="the option's values measured, in block order")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit: measured as a third leg")
    ap.add_argument("--no-pass", action="store_true", help="skip the process that times k_cg_dots alone")
    ap.add_argument("--child-timeout", type=int, default=800, help="seconds after which a leg's process is ended")
    ap.add_argument("--out", default="", help="file the JSON lines are written to (replaced)")
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--serve-pass", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--serve-option", type=int, default=-1, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        return serve(args)
    if args.serve_pass:
        return serve_pass(args)
    legs = list(dict.fromkeys(args.options)) + (["parent"] if args.parent_root else [])
    procs = {}
    lines, medians, spreads = [], {}, {}
    what = "CGSolver: real banded N=%d halfband=%d shift=2.5, B = I, threshold=%g, %d fixed iterations, monitor off, FMA arithmetic" % (
        args.n, args.h, args.threshold, args.steps)
    try:
        for v in legs:   # (one after the other: each builds its operands while nothing is being timed)
            procs[v] = Leg(args, str(v), args.parent_root if v == "parent" else ROOT, -1 if v == "parent" else v)
            procs[v].line()   # (ready)
        for v in legs:
            procs[v].run()   # (untimed: first launches, allocator pools)
        runs = {v: [] for v in legs}
        for _ in range(args.blocks):
            for v in legs:
                r = procs[v].run()   # (a leg that failed is not tried again)
                if r is not None:
                    runs[v].append(r)
                print("leg %s: %s" % (v, "%.3f ms" % r["ms"] if r else procs[v].failed), file=sys.stderr, flush=True)
        for v in legs:
            if procs[v].failed or not runs[v]:
                lines.append(json.dumps(dict(workload=what, cg_dots=v, failed=procs[v].failed or "no block completed", blocks_completed=len(runs[v]))))
                continue
            per = [r["ms"] / args.steps for r in runs[v]]
            med = statistics.median(per)
            last = runs[v][-1]
            medians[v], spreads[v] = med, (max(per) - min(per)) / med
            lines.append(json.dumps(dict(workload=what, cg_dots=v, blocks=len(per), ms_per_iteration=round(med, 3),
                                         blocks_ms_per_iteration=[round(x, 3) for x in per], spread=round(spreads[v], 4),
                                         entries_of_x=last["entries"], trace_of_x=last["trace"], cg_dots_counts=last["counts"])))
    finally:
        for leg in procs.values():
            leg.close()
    if not args.no_pass:
        leg = Leg(args, "pass", ROOT, 1, "--serve-pass")
        got = leg.line()
        leg.close()
        lines.append(json.dumps(dict(workload=what, k_cg_dots=got if got is not None else leg.failed)))
    summary = dict(summary="medians compared", legs_failed=[str(v) for v in legs if v not in medians])
    if medians:
        spread = max(spreads.values())
        summary["largest_spread"] = round(spread, 4)
        if 1 in medians:
            gains = {str(v): round((medians[v] - medians[1]) / medians[v], 4) for v in medians if v != 1}
            summary["gain_of_1_over"] = gains
            summary["option_1_faster_than_all_by_more_than_the_spread"] = bool(gains and all(g > spread for g in gains.values()))
            if 0 in medians and "parent" in medians:
                apart = abs(medians[0] - medians["parent"]) / medians["parent"]
                summary["option_0_and_parent_apart"] = round(apart, 4)
                summary["default"] = 1 if (summary["option_1_faster_than_all_by_more_than_the_spread"] and apart <= spread) else 0
    lines.append(json.dumps(summary))
    for ln in lines:
        print(ln)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
