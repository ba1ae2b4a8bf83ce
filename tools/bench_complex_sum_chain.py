#!/usr/bin/env python3
"""The complex side of the scaled sum chains (option complex_sum_chain), measured on configs[4]'s family at size: the complex banded
family of tests/gen.py, N = 131 072, H_ii = -1 + 2 ((i 7919) mod 1000) / 1000 + shift, H_ij = -0.25 exp(-0.05 k) / k exp(0.1 i (i - j))
for 0 < k = |i - j| <= --h (50), threshold 1e-8, FMA arithmetic.  Three workloads:

    cos      Cosine_wrp at shift 0.001 (no stored zero on the diagonal: the operand is no view; two Chebyshev sums and the doublings)
    invroot  ComputeInverseRoot_wrp(5) at shift 3.5 (the inverse-root iteration: target_root + 2 = 7 products per iteration)
    log      ComputeLogarithm_wrp at shift 3.5 (ComputeRoot behind PowerBounds' choice, then 31 chains of the factorized Chebyshev
             evaluation)

Four legs each: level 2 (complex session in the inverse-root loop and every complex chain in one pass), level 1 (the session only),
level 0 and -- with --parent-root DIR, a built checkout of the parent commit -- the parent's library, which does not know the
option.  The block scheme of DESIGN.md section 6: --warmup-blocks untimed warm-up blocks, then --blocks timed blocks; a block = each
workload once with each leg, in turn, so that whatever else the machine does meets all legs alike.  The parent runs in ONE child
process (under its own `timeout`) that imports the package from DIR, builds the same operands once and then runs one call per line
it is sent; it idles while this process measures, and the other way round.  Every leg calls the solvers through the C ABI.

The figure is a host clock around the whole call, which ends in a device synchronise.  Per leg the MEDIAN block is reported, all
blocks are listed, spread = (max - min) / median.  The pass alone is timed through its diagnostic entry point nt.sum_chain on the
operands of Cosine's second sum (T8, T6, T4, T2, I and T8 R built with the vocabulary, T8 R inside the session: M = 5), with its fraction of the 8 TB/s HBM
peak over the bytes it moves (six inputs read, one output written, 16 B per entry) -- an upper bound of its time, packing
included.  The last line applies the rule that decides defaults to each level: adopted iff on EVERY workload it is faster than
level 0 AND than the parent by more than the largest block spread, and level 0 equals the parent within that spread.  Prints JSON
lines and writes them to --out when given:

    timeout -k 10 1100 python tools/bench_complex_sum_chain.py --parent-root /path/to/parent --out profiles/complex_sum_chain_bench.json
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
HBM_PEAK_GBS = 8000.0   # MI355X
COS = {1: 7.651976865579664e-01, 3: -2.298069698638004e-01, 5: 4.953277928219409e-03, 7: -4.187667600472235e-05, 9: 1.884468822397086e-07,
       11: -5.261224549346905e-10, 13: 9.999906645345580e-13, 15: -2.083597362700025e-15, 17: 9.181480886537484e-17}   # (Chebyshev coefficients of cos, 1-based)
ALL = ("cos", "invroot", "log")
OPTION = "complex_sum_chain"


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
    if "cos" in args.workloads:
        ops["A"] = nt.Matrix_ps.from_triplets(args.n, *banded_triplets(args.n, args.h, complex_=True, shift=args.shift))
    if "invroot" in args.workloads or "log" in args.workloads:
        ops["L"] = nt.Matrix_ps.from_triplets(args.n, *banded_triplets(args.n, args.h, complex_=True, shift=args.root_shift))
    return ops


def solve(nt, args, ops, workload, level):
    if level is not None:
        nt.set_option(OPTION, level)
    p = nt.SolverParameters()
    p.SetThreshold(args.threshold)
    K = nt.Matrix_ps(args.n)
    c0 = nt.complex_sum_chain_counts() if level is not None else None
    s0 = nt.slab_algebra_counts()
    nt.synchronize()
    t0 = time.perf_counter()
    if workload == "cos":
        nt.lib.Cosine_wrp(ops["A"].ih, K.ih, p.ih)
    elif workload == "invroot":
        nt.lib.ComputeInverseRoot_wrp(ops["L"].ih, K.ih, C.byref(C.c_int(args.root)), p.ih)
    else:
        nt.lib.ComputeLogarithm_wrp(ops["L"].ih, K.ih, p.ih)
    nt.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    s1 = nt.slab_algebra_counts()
    out = dict(ms=ms, nnz_result=int(K.GetSize()), norm_result=float(K.Norm()), slab={k: int(s1[k] - s0[k]) for k in s1})
    if level is not None:
        c1 = nt.complex_sum_chain_counts()
        out["counts"] = {k: c1[k] - c0[k] for k in c1}
    return out


def the_pass(nt, args, ops):
    """the pass alone: the operands of Cosine's second sum, built with the vocabulary; --pass-reps calls of the diagnostic entry point"""
    nt.set_option(OPTION, 2)
    n, thr = args.n, args.threshold
    sigma = 1.0
    while ops["A"].Norm() / sigma > 1.0:   # (the 1-norm bounds Gershgorin's radius from above: at most one doubling more)
        sigma *= 2
    X = nt.Matrix_ps(ops["A"])
    X.Scale(1.0 / sigma)
    import numpy as np
    T2, T4, T6, T8, R, Temp, Out = (nt.Matrix_ps(n) for _ in range(7))
    diagonal = np.arange(1, n + 1, dtype=np.int32)
    Ic = nt.Matrix_ps.from_triplets(n, diagonal, diagonal, np.ones(n, dtype=np.complex128))   # (the identity as a COMPLEX matrix: the chain takes no mixed operands)
    T2.Gemm(X, X, None, 2.0, 0.0, thr)
    T2.Increment(Ic, -1.0, 0.0)
    T4.Gemm(T2, T2, None, 2.0, 0.0, thr)
    T4.Increment(Ic, -1.0, 0.0)
    T6.Gemm(T4, T2, None, 2.0, 0.0, thr)
    T6.Increment(T2, -1.0, 0.0)
    T8.Gemm(T6, T2, None, 2.0, 0.0, thr)
    T8.Increment(T4, -1.0, 0.0)
    R = nt.Matrix_ps(T8)
    R.Scale(0.5 * COS[17])
    for T, k in ((T6, 15), (T4, 13), (T2, 11)):
        R.Increment(T, 0.5 * COS[k], 0.0)
    addends = [T6, T4, T2, Ic, Temp]
    coeffs = [COS[7] + 0.5 * COS[11], COS[5] + 0.5 * COS[13], COS[3] + 0.5 * COS[15], COS[1] + 0.5 * COS[17], 1.0]
    out = dict(chain="complex Cosine's second sum, M = 5", note="a host clock around the diagnostic call: the span and scan launches, the pass, its "
               "read-back AND the packing of the output into the result handle -- an upper bound of the pass's own time")
    names = ["T6", "T4", "T2", "I", "T8 R"]
    with nt.solver_session(True):
        # (T8 R inside the session, as Cosine forms it: on this operand nothing of it passes the threshold, and an EMPTY complex matrix
        # in compressed columns does not enter slab form (slab_enter_c), which refuses the pass; the session's product is born in
        # slab form, empty or not)
        Temp.Gemm(T8, R, None, 1.0, 0.0, thr)
        c0 = nt.complex_sum_chain_counts()
        if not nt.sum_chain(T8, COS[9], addends, coeffs, 1.0, Out):   # (untimed: the operands enter slab form)
            # not taken: say whether a gate or a refusal kept it out, and which addend a chain of its own with T8 does not take
            c1 = nt.complex_sum_chain_counts()
            alone = {}
            for name, M, c in zip(names, addends, coeffs):
                b0 = nt.complex_sum_chain_counts()["refused"]
                ok = nt.sum_chain(T8, COS[9], [M], [c], 1.0, Out)
                alone[name] = "taken" if ok else ("refused" if nt.complex_sum_chain_counts()["refused"] > b0 else "gated")
            out.update({"pass": "refused" if c1["refused"] > c0["refused"] else "gated", "not measured": "the diagnostic call did not take the chain",
                        "entries": {k: int(M.GetSize()) for k, M in zip(["T8"] + names, [T8] + addends)}, "each_addend_alone_with_T8": alone})
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
    gb = 16.0 * (sum(read) + sum(written)) / 1e9
    out.update(pass_ms=round(ms, 3), pass_blocks=[round(t, 3) for t in times], entries_read=read, entries_written=written,
               gb_moved_counted_on_entries=round(gb, 3), fraction_of_hbm_peak_upper_bound_of_time=round(gb / (ms * 1e-3) / HBM_PEAK_GBS, 3))
    return out


def serve(args):
    """the parent's library: one call per line on stdin (the workload's name), one JSON line back; ends at end of input"""
    nt = load(args.root_dir)
    ops = operands(nt, args)
    print(json.dumps(dict(ready=True)), flush=True)
    for line in sys.stdin:
        if not line.strip():
            break
        print(json.dumps(solve(nt, args, ops, line.strip(), None)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--h", type=int, default=50)
    ap.add_argument("--shift", type=float, default=0.001, help="Cosine's operand: stores no zero diagonal")
    ap.add_argument("--root-shift", type=float, default=3.5, help="the operand of the inverse root and the logarithm: positive definite")
    ap.add_argument("--root", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=1e-8)
    ap.add_argument("--workloads", nargs="+", default=list(ALL), choices=ALL)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup-blocks", type=int, default=2, help="untimed blocks before the timed ones")
    ap.add_argument("--pass-reps", type=int, default=5)
    ap.add_argument("--levels", type=int, nargs="+", default=[2, 1, 0], choices=[0, 1, 2], help="the option's values measured in this process, in block order")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit: measured as a further leg")
    ap.add_argument("--child-timeout", type=int, default=1000, help="seconds after which the parent's process is ended")
    ap.add_argument("--out", default="", help="file the JSON lines are written to (replaced)")
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root-dir", dest="root_dir", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        return serve(args)
    nt = load(ROOT)
    child = None
    if args.parent_root:
        # (a time limit of its own: a child that hangs ends, and the blocking read below then sees the end of its output)
        child = subprocess.Popen(["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--serve", "--root-dir",
                                  os.path.abspath(args.parent_root), "--n", str(args.n), "--h", str(args.h), "--shift", repr(args.shift),
                                  "--root-shift", repr(args.root_shift), "--root", str(args.root), "--threshold", repr(args.threshold),
                                  "--workloads"] + list(args.workloads),
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

        def child_line():
            while True:
                ln = child.stdout.readline()
                if not ln:
                    raise RuntimeError("the parent's process ended early (exit code %s)" % child.poll())
                if ln.startswith("{"):
                    return json.loads(ln)
        child_line()   # (ready: its operands are built)
    legs = list(dict.fromkeys(args.levels)) + (["parent"] if child else [])
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
        names = {"cos": "Cosine, shift=%g" % args.shift, "invroot": "ComputeInverseRoot(%d), shift=%g" % (args.root, args.root_shift),
                 "log": "ComputeLogarithm, shift=%g" % args.root_shift}
        for w in args.workloads:
            for v in legs:
                per = [r["ms"] for r in runs[w, v]]
                med = statistics.median(per)
                last = runs[w, v][-1]
                medians[w, v], spreads[w, v] = med, (max(per) - min(per)) / med
                lines.append(json.dumps(dict(
                    workload="%s: complex band, N=%d, halfband=%d, threshold=%g, FMA arithmetic" % (names[w], args.n, args.h, args.threshold),
                    name=w, complex_sum_chain=v, blocks=args.blocks, warmup_blocks=args.warmup_blocks, call_ms=round(med, 2),
                    blocks_call_ms=[round(x, 2) for x in per], spread=round(spreads[w, v], 4), nnz_result=last["nnz_result"],
                    norm_result=last["norm_result"], complex_sum_chain_counts=last.get("counts"), slab_algebra_counts=last["slab"])))
        if 2 in legs and "cos" in args.workloads:
            lines.append(json.dumps(the_pass(nt, args, ops)))
    finally:
        if child:
            child.stdin.close()
            child.wait(timeout=120)
    spread = max(spreads.values())
    rule = dict(rule="a level is adopted iff on EVERY workload it beats level 0 and the parent by more than the largest block spread AND level 0 "
                     "equals the parent within it; the default stays 0 in this change whatever the verdict",
                largest_spread=round(spread, 4), parent_measured=bool(child), two_ranks_at_size="not measured")
    gain = lambda w, v, u: (medians[w, u] - medians[w, v]) / medians[w, u]
    verdict = {v: bool(child) and all((w, 0) in medians and (w, v) in medians for w in args.workloads) for v in (1, 2) if v in legs}
    for w in args.workloads:
        for v in verdict:
            rule["%s_gain_of_%d_over" % (w, v)] = {str(u): round(gain(w, v, u), 4) for u in legs if u != v and (w, u) in medians}
        if child and (w, 0) in medians:
            rule["%s_level_0_over_parent" % w] = round(medians[w, 0] / medians[w, "parent"] - 1.0, 4)
            equal = bool(abs(medians[w, 0] - medians[w, "parent"]) / medians[w, "parent"] <= spread)
            rule["%s_level_0_equals_parent_within_spread" % w] = equal
            for v in verdict:
                if not (equal and gain(w, v, 0) > spread and gain(w, v, "parent") > spread):
                    verdict[v] = False
    rule["adopted_by_the_rule"] = {str(v): ok for v, ok in verdict.items()}
    rule["default"] = 0
    lines.append(json.dumps(rule))
    for ln in lines:
        print(ln)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
