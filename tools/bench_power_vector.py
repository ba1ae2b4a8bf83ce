#!/usr/bin/env python3
"""PowerBounds on one vector (option power_vector), measured on the headline operand (tests/gen.py banded_triplets(262144, 100)),
FMA arithmetic, threshold 1e-8, ten fixed steps (what ComputeExponential asks for), convergence monitor off.

Three legs: option 1 (one column as a dense array: the gather form built once, a sparse matrix-vector product per step), option 0
(the reference's N x N iterate: a distributed product, two dots, a norm and a scaling per step) and -- with --parent-root DIR, a
built checkout of the parent commit -- the parent's library, which does not know the option.  Each leg runs in a process of its
own, which imports the package (from DIR for the parent), builds the same operand once and then runs one call per line it is sent;
it idles while another leg measures.  The block scheme of DESIGN.md section 6: one untimed warm-up block, then --blocks timed
blocks; a block = the call once with each leg, in turn.  Every leg calls the solver through the C ABI (PowerBounds_wrp).

The figure is a host clock around the whole call, which ends in a device synchronise (the gather form's construction is inside).
Per leg the MEDIAN block is reported, all blocks are listed, spread = (max - min) / median, and the in-use + cached device bytes
after the call minus those before the first one (the operand itself is not counted).  A leg whose process ends early -- the
N-column loop that cannot hold its iterates -- is recorded as failed and not tried again.  The last line states whether option 1
is faster than every other leg by more than the largest spread and holds less memory; it promises no ratio.
Prints JSON lines and writes them to --out when given:

    timeout -k 10 900 python tools/bench_power_vector.py --parent-root /path/to/parent --out profiles/power_vector_bench.json
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


def solve(nt, args, A, opt, base):
    if opt is not None:
        nt.set_option("power_vector", opt)
    p = nt.SolverParameters()
    p.SetThreshold(args.threshold)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(args.steps)
    p.SetMonitorConvergence(False)
    v = C.c_double()
    c0 = nt.power_vector_counts() if opt is not None else None
    nt.synchronize()
    t0 = time.perf_counter()
    nt.lib.PowerBounds_wrp(A.ih, C.byref(v), p.ih)
    nt.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    c1 = nt.power_vector_counts() if opt is not None else None
    return dict(ms=ms, bound=float(v.value), bytes=int(sum(nt.memory()) - base),
                counts={k: c1[k] - c0[k] for k in c1} if c1 else None)


def serve(args):
    """one leg: one call per line on stdin, one JSON line back; ends at end of input"""
    nt = load(args.root)
    from gen import banded_triplets
    A = nt.Matrix_ps.from_triplets(args.n, *banded_triplets(args.n, args.h))
    nt.synchronize()
    base = sum(nt.memory())
    opt = None if args.serve_option < 0 else args.serve_option   # (the parent's library does not know the option)
    print(json.dumps(dict(ready=True)), flush=True)
    for line in sys.stdin:
        if not line.strip():
            break
        print(json.dumps(solve(nt, args, A, opt, base)), flush=True)


class Leg:
    """a child process that measures one leg; it idles while the others measure"""

    def __init__(self, args, name, root, option):
        self.name = name
        self.failed = None
        # (a time limit of its own: a child that hangs ends, and the blocking read below then sees the end of its output)
        self.p = subprocess.Popen(["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--serve",
                                   "--serve-option", str(option), "--root", os.path.abspath(root), "--n", str(args.n), "--h", str(args.h),
                                   "--threshold", repr(args.threshold), "--steps", str(args.steps)],
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
    ap.add_argument("--threshold", type=float, default=1e-8)
    ap.add_argument("--steps", type=int, default=10)
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
    lines, medians, spreads, held = [], {}, {}, {}
    what = "PowerBounds: real banded N=%d halfband=%d, threshold=%g, %d fixed steps, monitor off, FMA arithmetic" % (
        args.n, args.h, args.threshold, args.steps)
    try:
        for v in legs:   # (one after the other: each builds its operand while nothing is being timed)
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
                lines.append(json.dumps(dict(workload=what, power_vector=v, failed=procs[v].failed or "no block completed",
                                             blocks_completed=len(runs[v]))))
                continue
            per = [r["ms"] for r in runs[v]]
            med = statistics.median(per)
            last = runs[v][-1]
            medians[v], spreads[v], held[v] = med, (max(per) - min(per)) / med, last["bytes"]
            lines.append(json.dumps(dict(workload=what, power_vector=v, blocks=len(per), ms_per_call=round(med, 3),
                                         blocks_ms_per_call=[round(x, 3) for x in per], spread=round(spreads[v], 4),
                                         bytes_in_use_and_cached_after_the_call=last["bytes"], bound=last["bound"],
                                         power_vector_counts=last["counts"])))
    finally:
        for leg in procs.values():
            leg.close()
    summary = dict(summary="medians compared", legs_failed=[str(v) for v in legs if v not in medians])
    if medians:
        spread = max(spreads.values())
        summary["largest_spread"] = round(spread, 4)
        if 1 in medians:
            gains = {str(v): round((medians[v] - medians[1]) / medians[v], 4) for v in medians if v != 1}
            summary["gain_of_1_over"] = gains
            summary["option_1_faster_than_all_by_more_than_the_spread"] = bool(gains and all(g > spread for g in gains.values()))
            summary["option_1_holds_less_memory_than_all"] = bool(gains and all(held[1] < held[v] for v in medians if v != 1))
    lines.append(json.dumps(summary))
    for ln in lines:
        print(ln)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
