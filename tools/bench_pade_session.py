#!/usr/bin/env python3
"""ComputeExponentialPade in a slab session (option pade_session), measured on the banded family of tests/gen.py at size: N = 262 144,
H_ii = -1 + 2 ((i 7919) mod 1000) / 1000 + shift, H_ij = -0.25 exp(-0.05 k) / k for 0 < k = |i - j| <= --h (100), shift 2 (the norm
is 4.5, so sigma = 8 and three squarings follow CG), threshold 1e-6 (the powers prune: at n = 2500 a dense restatement gives longest
columns of 227 / 203 / 76 / 425 rows for B1 / B2 / B3 / P2), converge_diff 1e-6, FMA arithmetic.

Four legs: option 2 (the session with each group of merges in one pass), option 1 (the session with the vocabulary calls), option
0 (the call on compressed columns) and -- with --parent-root DIR, a built checkout of the parent commit -- the parent's library,
which does not know the option.  The block scheme of DESIGN.md section 6: --warmup-blocks untimed warm-up blocks (one; two where a
leg's second call is still slow), then --blocks timed blocks; a block = the call once with each leg, in turn, so that whatever
else the machine does meets all legs alike.  The parent runs in ONE
child process that imports the package from DIR, builds the same operand once and then runs one call per line it is sent; it idles
while this process measures, and the other way round.  Every leg calls the solver through the C ABI (ComputeExponentialPade_wrp).

The figure is a host clock around the whole call, which ends in a device synchronise.  Per leg the MEDIAN block is reported, all
blocks are listed, spread = (max - min) / median.  Each pass alone is timed through its diagnostic entry point on the powers and
products of the same operand (passes below), with its fraction of the HBM peak over the runs it moves (the inputs read, two
outputs written).  The last line applies the rule that decides the default: the fastest non-zero value iff it is faster than
option 0 AND than the parent by more than the largest block spread, and option 0 equals the parent within that spread (2 only if
it also beats 1 by more than the spread).  Prints JSON lines and writes them to --out when given:

    timeout -k 10 1100 python tools/bench_pade_session.py --parent-root /path/to/parent --out profiles/pade_session_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0   # MI355X
PADE_S = (17297280.0, 8648640.0)
PADE_C = ((1995840.0, 25200.0, 56.0), (277200.0, 1512.0, 1.0))


def load(root):
    sys.path.insert(0, root)
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("spgemm_fma", 1)
    return nt


def operand(nt, args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gen import banded_triplets
    return nt.Matrix_ps.from_triplets(args.n, *banded_triplets(args.n, args.h, shift=args.shift))


def solve(nt, args, A, opt):
    if opt is not None:
        nt.set_option("pade_session", opt)
    p = nt.SolverParameters()
    p.SetThreshold(args.threshold)
    p.SetConvergeDiff(args.converge_diff)
    K = nt.Matrix_ps(args.n)
    c0 = nt.pade_session_counts() if opt is not None else None
    g0, s0 = nt.cg_dots_counts(), nt.slab_algebra_counts()
    nt.synchronize()
    t0 = time.perf_counter()
    nt.lib.ComputeExponentialPade_wrp(A.ih, K.ih, p.ih)
    nt.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    g1, s1 = nt.cg_dots_counts(), nt.slab_algebra_counts()
    out = dict(ms=ms, nnz_result=int(K.GetSize()), norm_result=float(K.Norm()), trace_result=float(K.Trace()),
               cg_iterations=int(g1["passes"] + g1["refused"] - g0["passes"] - g0["refused"]) // 2, slab={k: int(s1[k] - s0[k]) for k in s1})
    if opt is not None:
        c1 = nt.pade_session_counts()
        out["counts"] = {k: c1[k] - c0[k] for k in c1}
    return out


def passes(nt, args, A):
    """each pass alone: the powers and P2 of the same operand at the call's inner threshold, --pass-reps calls of the diagnostic
    entry point"""
    nt.set_option("pade_session", 2)
    n = args.n
    norm = A.Norm()
    sigma = 1.0
    while norm / sigma > 1.0:
        sigma *= 2
    thr = args.threshold / sigma
    S = nt.Matrix_ps(A)
    S.Scale(1.0 / sigma)
    I, B1, B2, B3, P1, T, P2, L, R = (nt.Matrix_ps(n) for _ in range(9))
    I.FillIdentity()
    B1.Gemm(S, S, None, 1.0, 0.0, thr)
    B2.Gemm(B1, B1, None, 1.0, 0.0, thr)
    B3.Gemm(B2, B2, None, 1.0, 0.0, thr)
    out = dict(sigma=sigma, note="a host clock around the diagnostic call: the span and scan launches, the pass, its read-back AND the packing of "
               "both outputs into the result handles -- an upper bound of the pass's own time")
    with nt.solver_session(False):
        for tag, base, addends, s, c, o1, o2 in (("sum", I, (B1, B2, B3), PADE_S, PADE_C, P1, T), ("pair", P1, (P2,), (1.0, 1.0), ((-1.0,), (1.0,)), L, R)):
            if tag == "pair":
                P2.Gemm(S, T, None, 1.0, 0.0, thr)
            got = nt.pade_chain_step(base, addends, s, c, o1, o2)   # (untimed: the operands enter slab form)
            if got is None:
                out[tag] = "refused"
                continue
            times = []
            for _ in range(args.pass_reps):
                nt.synchronize()
                t0 = time.perf_counter()
                nt.pade_chain_step(base, addends, s, c, o1, o2)
                nt.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            ms = statistics.median(times)
            read = [int(M.GetSize()) for M in (base,) + tuple(addends)]
            written = [int(o1.GetSize()), int(o2.GetSize())]
            gb = 8.0 * (sum(read) + sum(written)) / 1e9
            out[tag] = dict(pass_ms=round(ms, 3), pass_blocks=[round(t, 3) for t in times], entries_read=read, entries_written=written,
                            gb_moved_counted_on_entries=round(gb, 3), fraction_of_hbm_peak=round(gb / (ms * 1e-3) / HBM_PEAK_GBS, 3))
    return out


def serve(args):
    """the parent's library: one call per line on stdin, one JSON line back; ends at end of input"""
    nt = load(args.root)
    A = operand(nt, args)
    print(json.dumps(dict(ready=True)), flush=True)
    for line in sys.stdin:
        if not line.strip():
            break
        print(json.dumps(solve(nt, args, A, None)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--h", type=int, default=100)
    ap.add_argument("--shift", type=float, default=2.0)
    ap.add_argument("--threshold", type=float, default=1e-6)
    ap.add_argument("--converge-diff", type=float, default=1e-6)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup-blocks", type=int, default=1, help="untimed blocks before the timed ones")
    ap.add_argument("--pass-reps", type=int, default=5)
    ap.add_argument("--options", type=int, nargs="+", default=[2, 1, 0], choices=[0, 1, 2], help="the option's values measured in this process, in block order")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit: measured as a further leg")
    ap.add_argument("--child-timeout", type=int, default=1000, help="seconds after which the parent's process is ended")
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
        child = subprocess.Popen(["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--serve", "--root",
                                  os.path.abspath(args.parent_root), "--n", str(args.n), "--h", str(args.h), "--shift", repr(args.shift),
                                  "--threshold", repr(args.threshold), "--converge-diff", repr(args.converge_diff)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

        def child_line():
            while True:
                ln = child.stdout.readline()
                if not ln:
                    raise RuntimeError("the parent's process ended early (exit code %s)" % child.poll())
                if ln.startswith("{"):
                    return json.loads(ln)
        child_line()   # (ready: its operand is built)
    legs = list(dict.fromkeys(args.options)) + (["parent"] if child else [])
    A = operand(nt, args)

    def run(v):
        if v == "parent":
            child.stdin.write("solve\n")
            child.stdin.flush()
            return child_line()
        return solve(nt, args, A, v)

    lines, medians, spreads = [], {}, {}
    try:
        for w in range(args.warmup_blocks):
            for v in legs:
                r = run(v)   # (untimed: first launches, allocator pools)
                print("warm-up block", w, "leg", v, "%.1f ms" % r["ms"], file=sys.stderr, flush=True)
        runs = {v: [] for v in legs}
        for b in range(args.blocks):
            for v in legs:
                runs[v].append(run(v))
                print("block", b, "leg", v, "%.1f ms" % runs[v][-1]["ms"], file=sys.stderr, flush=True)
        for v in legs:
            per = [r["ms"] for r in runs[v]]
            med = statistics.median(per)
            last = runs[v][-1]
            medians[v], spreads[v] = med, (max(per) - min(per)) / med
            lines.append(json.dumps(dict(
                workload="ComputeExponentialPade: N=%d, halfband=%d, shift=%g, threshold=%g, converge_diff=%g, FMA arithmetic" % (
                    args.n, args.h, args.shift, args.threshold, args.converge_diff),
                pade_session=v, blocks=args.blocks, warmup_blocks=args.warmup_blocks, call_ms=round(med, 2), blocks_call_ms=[round(x, 2) for x in per], spread=round(spreads[v], 4),
                cg_iterations=last["cg_iterations"], nnz_result=last["nnz_result"], norm_result=last["norm_result"],
                trace_result=last["trace_result"], pade_session_counts=last.get("counts"), slab_algebra_counts=last["slab"])))
        if 2 in legs:
            lines.append(json.dumps(passes(nt, args, A)))
    finally:
        if child:
            child.stdin.close()
            child.wait(timeout=120)
    spread = max(spreads[v] for v in legs)
    rule = dict(rule="default v > 0 iff option v beats option 0 and the parent by more than the largest block spread AND option 0 equals the parent "
                     "within it; 2 only if it also beats 1 by more than that spread",
                largest_spread=round(spread, 4), parent_measured=bool(child), unfused_arithmetic="not measured", two_ranks_at_size="not measured")
    if 0 in medians and child:
        rule["option_0_over_parent"] = round(medians[0] / medians["parent"] - 1.0, 4)
        rule["option_0_equals_parent_within_spread"] = bool(abs(medians[0] - medians["parent"]) / medians["parent"] <= spread)
    gain = lambda v, w: (medians[w] - medians[v]) / medians[w]
    for v in (1, 2):
        if v in medians:
            rule["gain_of_%d_over" % v] = {str(w): round(gain(v, w), 4) for w in legs if w != v}
    default = 0
    if child and 0 in medians and rule["option_0_equals_parent_within_spread"]:
        ok = {v: v in medians and gain(v, 0) > spread and gain(v, "parent") > spread for v in (1, 2)}
        if ok[2] and (1 not in medians or gain(2, 1) > spread):
            default = 2
        elif ok[1]:
            default = 1
    rule["default"] = default
    lines.append(json.dumps(rule))
    for ln in lines:
        print(ln)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
