#!/usr/bin/env python3
"""The polynomial chain of the Taylor square-root step in one pass (option isr_chain), measured on the operands
tests/test_gpu_scale.py builds, FMA arithmetic, threshold 1e-8, convergence 1e-8, order 5:

  (a) real:    InverseSquareRoot of the headline operand plus 2 I (banded_triplets(262144, 100, shift=2));
  (b) complex: InverseSquareRoot of configs[4]'s H + 2 I (banded_triplets(131072, 50, complex_=True, shift=2)).

Three variants: option 0 (the vocabulary calls, one by one), option 1 (the fused chain) and -- with --parent-root DIR, a built
checkout of the parent commit -- the parent's library, which does not know the option.  The block scheme of DESIGN.md section 6:
one untimed warm-up block, then --blocks timed blocks; a block = the solve once with each variant, in turn, so that whatever else
the machine does meets all three alike.  The parent runs in ONE child process that imports the package from DIR, builds the same
operands once and then runs one solve per line it is sent; it idles while this process measures, and the other way round.

The figure is a host clock around the whole solver call, which ends in a device synchronise, divided by the iteration count
(the square-root loop keeps no loop clock of its own: set-up and the final scaling are inside, the same for every variant).  Per
variant the MEDIAN block is reported, all blocks are listed, spread = (max - min) / median.  One more solve per option runs with
the engine's event timers on (time_kernels) and gives the share of the call inside the SpGEMM numeric launches.  The last line
applies the rule that decides the default: 1 if option 1 is faster than option 0 AND than the parent by more than the block
spread on (a) and not slower than either on (b).  Prints JSON lines and writes them to --out when given:

    timeout -k 10 1100 python tools/bench_isr_chain.py --parent-root /path/to/parent --out profiles/isr_chain_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"real": dict(n=262144, h=100, cplx=False, what="real InverseSquareRoot, headline operand + 2 I"),
         "complex": dict(n=131072, h=50, cplx=True, what="complex InverseSquareRoot, configs[4] H + 2 I")}


def load(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("spgemm_fma", 1)
    return nt


def operand(nt, spec, scale):
    from gen import banded_triplets
    n = max(512, spec["n"] // scale)
    return n, nt.Matrix_ps.from_triplets(n, *banded_triplets(n, spec["h"], complex_=spec["cplx"], shift=2.0))


def solve(nt, n, H, opt, timers=False):
    if opt is not None:
        nt.set_option("isr_chain", opt)
    nt.set_option("time_kernels", 1 if timers else 0)
    p = nt.SolverParameters()
    p.SetThreshold(1e-8)
    p.SetConvergeDiff(1e-8)
    Out = nt.Matrix_ps(n)
    c0 = nt.isr_chain_counts() if opt is not None else None
    s0 = nt.slab_algebra_counts()
    nt.reset_spgemm_accum()
    nt.synchronize()
    t0 = time.perf_counter()
    nt.SquareRootSolvers.with_order(H, Out, p, True, 5)
    nt.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    acc = nt.spgemm_accum()
    tr = nt.solver_trace()
    c1 = nt.isr_chain_counts() if opt is not None else None
    s1 = nt.slab_algebra_counts()
    return dict(ms=ms, iters=int(tr["iterations"]), kernel_ms=float(acc["ms_numeric"]), nnz=int(Out.GetSize()),
                value=float(tr["value"][-1]), chain={k: c1[k] - c0[k] for k in c1} if c1 else None,
                slab={k: s1[k] - s0[k] for k in s1})


def serve(args):
    """the parent's library: one solve per line "<case>" on stdin, one JSON line back; ends at end of input"""
    nt = load(args.root)
    ops = {name: operand(nt, CASES[name], args.scale) for name in args.cases}
    print(json.dumps(dict(ready=True)), flush=True)
    for line in sys.stdin:
        name = line.strip()
        if not name:
            break
        n, H = ops[name]
        print(json.dumps(solve(nt, n, H, None)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--cases", nargs="+", default=["real", "complex"], choices=sorted(CASES))
    ap.add_argument("--scale", type=int, default=1, help="divide the dimensions by this (rehearsals)")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit: measured as a third variant")
    ap.add_argument("--child-timeout", type=int, default=900, help="seconds after which the parent's process is ended")
    ap.add_argument("--no-option", action="store_true", help="this library does not know isr_chain: one variant, labelled 'parent'")
    ap.add_argument("--out", default="", help="file the JSON lines are written to (replaced)")
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        return serve(args)
    nt = load(ROOT)
    child = None
    if args.parent_root:
        # (a time limit of its own: a child that hangs ends, and the blocking read below then sees the end of its output)
        child = subprocess.Popen(["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--serve", "--root", os.path.abspath(args.parent_root), "--scale",
                                  str(args.scale), "--cases"] + args.cases, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

        def child_line():
            while True:
                ln = child.stdout.readline()
                if not ln:
                    raise RuntimeError("the parent's process ended early (exit code %s)" % child.poll())
                if ln.startswith("{"):
                    return json.loads(ln)
        child_line()   # (ready: its operands are built)
    variants = (["parent"] if args.no_option else [0, 1]) + (["parent-root"] if child else [])

    def run(name, n, H, v, timers=False):
        if v == "parent-root":
            child.stdin.write(name + "\n")
            child.stdin.flush()
            return child_line()
        return solve(nt, n, H, None if v == "parent" else v, timers)

    lines, medians, spreads = [], {}, {}
    try:
        for name in args.cases:
            spec = CASES[name]
            n, H = operand(nt, spec, args.scale)
            for v in variants:
                run(name, n, H, v)   # (untimed: first launches, allocator pools, kept transposes)
            runs = {v: [] for v in variants}
            for _ in range(args.blocks):
                for v in variants:
                    runs[v].append(run(name, n, H, v))
            for v in variants:
                per = [r["ms"] / r["iters"] for r in runs[v]]
                med = statistics.median(per)
                last = runs[v][-1]
                timed = run(name, n, H, v, timers=True) if v in (0, 1) else None
                label = "parent" if v in ("parent", "parent-root") else v
                medians[(name, label)], spreads[(name, label)] = med, (max(per) - min(per)) / med
                lines.append(json.dumps(dict(
                    workload="%s: banded N=%d halfband=%d shift=2, threshold=1e-8, convergence=1e-8, order 5, FMA arithmetic" % (
                        spec["what"], n, spec["h"]),
                    case=name, isr_chain=label, blocks=args.blocks, iterations=last["iters"], ms_per_iteration=round(med, 3),
                    blocks_ms_per_iteration=[round(x, 3) for x in per], spread=round((max(per) - min(per)) / med, 4),
                    call_ms=round(statistics.median(r["ms"] for r in runs[v]), 2),
                    kernel_share=round(timed["kernel_ms"] / timed["ms"], 3) if timed else None,
                    kernel_ms_per_iteration=round(timed["kernel_ms"] / timed["iters"], 3) if timed else None,
                    call_ms_with_timers_per_iteration=round(timed["ms"] / timed["iters"], 3) if timed else None,
                    nnz_result=last["nnz"], last_norm=last["value"], isr_chain_counts=last["chain"], slab_algebra_counts=last["slab"])))
            del H
    finally:
        if child:
            child.stdin.close()
            child.wait(timeout=120)
    # the rule for the default
    if not args.no_option:
        rule = dict(rule="default 1 iff option 1 beats option 0 and the parent by more than the block spread on (a) and is not slower on (b)")
        ok = True
        for name in args.cases:
            others = [l for l in (0, "parent") if (name, l) in medians]
            m1 = medians[(name, 1)]
            spread = max(spreads[(name, l)] for l in [1] + others)
            gains = {str(l): round((medians[(name, l)] - m1) / medians[(name, l)], 4) for l in others}
            rule[name] = dict(gain_of_1_over=gains, block_spread=round(spread, 4))
            if name == "real":
                ok = ok and all(g > spread for g in gains.values())
            else:
                ok = ok and all(g >= -spread for g in gains.values())
        rule["parent_measured"] = bool(child)
        rule["default"] = 1 if ok and set(args.cases) == set(CASES) and child else 0
        lines.append(json.dumps(rule))
    for ln in lines:
        print(ln)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
