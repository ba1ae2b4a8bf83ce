#!/usr/bin/env python3
"""The scaled sum chains of the real solver loops in one pass (option sum_chain), measured on the banded family of tests/gen.py at
size: N = 262 144, H_ii = -1 + 2 ((i 7919) mod 1000) / 1000 + shift, H_ij = -0.25 exp(-0.05 k) / k for 0 < k = |i - j| <= --h (100),
shift 2, threshold 1e-6, FMA arithmetic.  Three workloads:

    cos     Cosine_wrp on the operand (two Chebyshev sums and sigma_counter - 1 doublings around 6 + sigma_counter - 1 products)
    ps      PatersonStockmeyerCompute_wrp with --ps-coefficients (16) coefficients (-0.8)^q / (q + 1) (its products take no threshold)
    log     ComputeLogarithm_wrp on the band with --log-shift, which makes it positive definite (31 chains of the factorized
            Chebyshev evaluation, and the inverse-root iteration where PowerBounds chooses a root of 8 or more)

Three legs each: option 1 (every chain in one pass), option 0 and -- with --parent-root DIR, a built checkout of the parent commit --
the parent's library, which does not know the option.  The block scheme of DESIGN.md section 6: --warmup-blocks untimed warm-up
blocks, then --blocks timed blocks; a block = each workload once with each leg, in turn, so that whatever else the machine does meets
all legs alike.  The parent runs in ONE child process (under its own `timeout`) that imports the package from DIR, builds the same
operands once and then runs one call per line it is sent; it idles while this process measures, and the other way round.  Every leg
calls the solvers through the C ABI.

The figure is a host clock around the whole call, which ends in a device synchronise.  Per leg the MEDIAN block is reported, all
blocks are listed, spread = (max - min) / median.  The pass alone is timed through its diagnostic entry point nt.sum_chain on the
operands of Cosine's second sum (T8, T6, T4, T2, I and T8 R built with the vocabulary: M = 5), with its fraction of the 8 TB/s HBM
peak over the entries it moves (six inputs read, one output written).  The last line applies the rule that decides the default to
every workload: 1 iff option 1 is faster than option 0 AND than the parent by more than the largest block spread, and option 0
equals the parent within that spread.  Prints JSON lines and writes them to --out when given:

    timeout -k 10 1100 python tools/bench_sum_chain.py --parent-root /path/to/parent --out profiles/sum_chain_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0   # MI355X
COS = {1: 7.651976865579664e-01, 3: -2.298069698638004e-01, 5: 4.953277928219409e-03, 7: -4.187667600472235e-05, 9: 1.884468822397086e-07,
       11: -5.261224549346905e-10, 13: 9.999906645345580e-13, 15: -2.083597362700025e-15, 17: 9.181480886537484e-17}   # (Chebyshev coefficients of cos, 1-based)
ALL = ("cos", "ps", "log")


def load(root):
    sys.path.insert(0, root)
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("spgemm_fma", 1)
    return nt


def operands(nt, args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gen import banded_triplets
    ops = {}
    if "cos" in args.workloads or "ps" in args.workloads:
        ops["A"] = nt.Matrix_ps.from_triplets(args.n, *banded_triplets(args.n, args.h, shift=args.shift))
    if "log" in args.workloads:
        ops["L"] = nt.Matrix_ps.from_triplets(args.n, *banded_triplets(args.n, args.h, shift=args.log_shift))
    if "ps" in args.workloads:
        ops["poly"] = nt.Polynomial(args.ps_coefficients)
        for q in range(args.ps_coefficients):
            ops["poly"].SetCoefficient(q, (-0.8) ** q / (q + 1.0))
    return ops


def solve(nt, args, ops, workload, opt):
    if opt is not None:
        nt.set_option("sum_chain", opt)
    p = nt.SolverParameters()
    p.SetThreshold(args.threshold)
    K = nt.Matrix_ps(args.n)
    c0 = nt.sum_chain_counts() if opt is not None else None
    s0 = nt.slab_algebra_counts()
    nt.synchronize()
    t0 = time.perf_counter()
    if workload == "cos":
        nt.lib.Cosine_wrp(ops["A"].ih, K.ih, p.ih)
    elif workload == "ps":
        nt.lib.PatersonStockmeyerCompute_wrp(ops["A"].ih, K.ih, ops["poly"].ih, p.ih)
    else:
        nt.lib.ComputeLogarithm_wrp(ops["L"].ih, K.ih, p.ih)
    nt.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    s1 = nt.slab_algebra_counts()
    out = dict(ms=ms, nnz_result=int(K.GetSize()), norm_result=float(K.Norm()), trace_result=float(K.Trace()), slab={k: int(s1[k] - s0[k]) for k in s1})
    if opt is not None:
        c1 = nt.sum_chain_counts()
        out["counts"] = {k: c1[k] - c0[k] for k in c1}
    return out


def the_pass(nt, args, ops):
    """the pass alone: the operands of Cosine's second sum, built with the vocabulary; --pass-reps calls of the diagnostic entry point"""
    nt.set_option("sum_chain", 1)
    n, thr = args.n, args.threshold
    sigma = 1.0
    while ops["A"].Norm() / sigma > 1.0:   # (the 1-norm bounds Gershgorin's radius from above: at most one doubling more)
        sigma *= 2
    X = nt.Matrix_ps(ops["A"])
    X.Scale(1.0 / sigma)
    I, T2, T4, T6, T8, R, Temp, Out = (nt.Matrix_ps(n) for _ in range(8))
    I.FillIdentity()
    T2.Gemm(X, X, None, 2.0, 0.0, thr)
    T2.Increment(I, -1.0, 0.0)
    T4.Gemm(T2, T2, None, 2.0, 0.0, thr)
    T4.Increment(I, -1.0, 0.0)
    T6.Gemm(T4, T2, None, 2.0, 0.0, thr)
    T6.Increment(T2, -1.0, 0.0)
    T8.Gemm(T6, T2, None, 2.0, 0.0, thr)
    T8.Increment(T4, -1.0, 0.0)
    R = nt.Matrix_ps(T8)
    R.Scale(0.5 * COS[17])
    for T, k in ((T6, 15), (T4, 13), (T2, 11)):
        R.Increment(T, 0.5 * COS[k], 0.0)
    Temp.Gemm(T8, R, None, 1.0, 0.0, thr)
    addends = [T6, T4, T2, I, Temp]
    coeffs = [COS[7] + 0.5 * COS[11], COS[5] + 0.5 * COS[13], COS[3] + 0.5 * COS[15], COS[1] + 0.5 * COS[17], 1.0]
    out = dict(chain="Cosine's second sum, M = 5", note="a host clock around the diagnostic call: the span and scan launches, the pass, its read-back AND the "
               "packing of the output into the result handle -- an upper bound of the pass's own time")
    with nt.solver_session(False):
        if not nt.sum_chain(T8, COS[9], addends, coeffs, 1.0, Out):   # (untimed: the operands enter slab form)
            out["pass"] = "refused"
            return out
        times = []
        for _ in range(args.pass_reps):
            nt.synchronize()
            t0 = time.perf_counter()
            nt.sum_chain(T8, COS[9], addends, coeffs, 1.0, Out)
            nt.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    ms = statistics.median(times)
    read = [int(M.GetSize()) for M in [T8] + addends]
    written = [int(Out.GetSize())]
    gb = 8.0 * (sum(read) + sum(written)) / 1e9
    out.update(pass_ms=round(ms, 3), pass_blocks=[round(t, 3) for t in times], entries_read=read, entries_written=written,
               gb_moved_counted_on_entries=round(gb, 3), fraction_of_hbm_peak=round(gb / (ms * 1e-3) / HBM_PEAK_GBS, 3))
    return out


def serve(args):
    """the parent's library: one call per line on stdin (the workload's name), one JSON line back; ends at end of input"""
    nt = load(args.root)
    ops = operands(nt, args)
    print(json.dumps(dict(ready=True)), flush=True)
    for line in sys.stdin:
        if not line.strip():
            break
        print(json.dumps(solve(nt, args, ops, line.strip(), None)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--h", type=int, default=100)
    ap.add_argument("--shift", type=float, default=2.0)
    ap.add_argument("--log-shift", type=float, default=2.6, help="the shift of the logarithm's operand: positive definite by Gershgorin from 2.51 on at h = 100")
    ap.add_argument("--threshold", type=float, default=1e-6)
    ap.add_argument("--ps-coefficients", type=int, default=16)
    ap.add_argument("--workloads", nargs="+", default=list(ALL), choices=ALL)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup-blocks", type=int, default=2, help="untimed blocks before the timed ones")
    ap.add_argument("--pass-reps", type=int, default=5)
    ap.add_argument("--options", type=int, nargs="+", default=[1, 0], choices=[0, 1], help="the option's values measured in this process, in block order")
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
                                  "--log-shift", repr(args.log_shift), "--threshold", repr(args.threshold), "--ps-coefficients",
                                  str(args.ps_coefficients), "--workloads"] + list(args.workloads),
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

        def child_line():
            while True:
                ln = child.stdout.readline()
                if not ln:
                    raise RuntimeError("the parent's process ended early (exit code %s)" % child.poll())
                if ln.startswith("{"):
                    return json.loads(ln)
        child_line()   # (ready: its operands are built)
    legs = list(dict.fromkeys(args.options)) + (["parent"] if child else [])
    ops = operands(nt, args)

    def run(w, v):
        if v == "parent":
            child.stdin.write(w + "\n")
            child.stdin.flush()
            return child_line()
        return solve(nt, args, ops, w, v)

    lines, medians, spreads = [], {}, {}
    try:
        for b in range(args.warmup_blocks):
            for w in args.workloads:
                for v in legs:
                    r = run(w, v)   # (untimed: first launches, allocator pools)
                    print("warm-up block", b, w, "leg", v, "%.1f ms" % r["ms"], file=sys.stderr, flush=True)
        runs = {(w, v): [] for w in args.workloads for v in legs}
        for b in range(args.blocks):
            for w in args.workloads:
                for v in legs:
                    runs[w, v].append(run(w, v))
                    print("block", b, w, "leg", v, "%.1f ms" % runs[w, v][-1]["ms"], file=sys.stderr, flush=True)
        names = {"cos": "Cosine, shift=%g" % args.shift, "ps": "PatersonStockmeyerCompute, %d coefficients, shift=%g" % (args.ps_coefficients, args.shift),
                 "log": "ComputeLogarithm, shift=%g" % args.log_shift}
        for w in args.workloads:
            for v in legs:
                per = [r["ms"] for r in runs[w, v]]
                med = statistics.median(per)
                last = runs[w, v][-1]
                medians[w, v], spreads[w, v] = med, (max(per) - min(per)) / med
                lines.append(json.dumps(dict(
                    workload="%s: N=%d, halfband=%d, threshold=%g, FMA arithmetic" % (names[w], args.n, args.h, args.threshold),
                    name=w, sum_chain=v, blocks=args.blocks, warmup_blocks=args.warmup_blocks, call_ms=round(med, 2), blocks_call_ms=[round(x, 2) for x in per],
                    spread=round(spreads[w, v], 4), nnz_result=last["nnz_result"], norm_result=last["norm_result"], trace_result=last["trace_result"],
                    sum_chain_counts=last.get("counts"), slab_algebra_counts=last["slab"])))
        if 1 in legs and "cos" in args.workloads:
            lines.append(json.dumps(the_pass(nt, args, ops)))
    finally:
        if child:
            child.stdin.close()
            child.wait(timeout=120)
    spread = max(spreads.values())
    rule = dict(rule="default 1 iff on EVERY workload option 1 beats option 0 and the parent by more than the largest block spread AND option 0 equals "
                     "the parent within it", largest_spread=round(spread, 4), parent_measured=bool(child), unfused_arithmetic="not measured",
                two_ranks_at_size="not measured")
    gain = lambda w, v, u: (medians[w, u] - medians[w, v]) / medians[w, u]
    default = 1 if (child and (args.workloads[0], 0) in medians and (args.workloads[0], 1) in medians) else 0
    for w in args.workloads:
        if (w, 1) in medians:
            rule["%s_gain_of_1_over" % w] = {str(u): round(gain(w, 1, u), 4) for u in legs if u != 1}
        if child and (w, 0) in medians:
            rule["%s_option_0_over_parent" % w] = round(medians[w, 0] / medians[w, "parent"] - 1.0, 4)
            equal = bool(abs(medians[w, 0] - medians[w, "parent"]) / medians[w, "parent"] <= spread)
            rule["%s_option_0_equals_parent_within_spread" % w] = equal
            if not (equal and (w, 1) in medians and gain(w, 1, 0) > spread and gain(w, 1, "parent") > spread):
                default = 0
    rule["default"] = default
    lines.append(json.dumps(rule))
    for ln in lines:
        print(ln)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
