#!/usr/bin/env python3
"""The real Chebyshev / Hermite step in one pass and ComputeExponential's squarings in a slab session (option poly_step), measured
on the banded family of tests/gen.py at size: N = 262 144, H_ii = -1 + 2 ((i 7919) mod 1000) / 1000 + shift, H_ij = -0.25 exp(-0.05 k) / k
for 0 < k = |i - j| <= --h (100), shift 2, threshold 1e-6, FMA arithmetic.  Two workloads:

    exp     ComputeExponential_wrp on the operand (PowerBounds, the scaling, 14 recurrence steps, the squarings)
    cheby   ChebyshevCompute_wrp with the 16 Chebyshev coefficients of exp on the operand scaled by 1 / sigma at threshold / sigma --
            the kind of evaluation the exponential makes, alone (sigma: the power of two above the operand's 1-norm, 8 at the
            default shift; ComputeExponential itself scales by PowerBounds' estimate of the spectral radius, 4 there)

Four legs each: option 2 (the step's tail in one pass, the squarings in a session), option 1 (the squarings in a session), option 0
and -- with --parent-root DIR, a built checkout of the parent commit -- the parent's library, which does not know the option.  The
block scheme of DESIGN.md section 6: --warmup-blocks untimed warm-up blocks, then --blocks timed blocks; a block = each workload
once with each leg, in turn, so that whatever else the machine does meets all legs alike.  The parent runs in ONE child process
(under its own `timeout`) that imports the package from DIR, builds the same operands once and then runs one call per line it is
sent; it idles while this process measures, and the other way round.  Every leg calls the solvers through the C ABI.

The figure is a host clock around the whole call, which ends in a device synchronise.  Per leg the MEDIAN block is reported, all
blocks are listed, spread = (max - min) / median.  The pass alone is timed through its diagnostic entry point nt.poly_step on step
--pass-step of the same evaluation, with its fraction of the 8 TB/s HBM peak over the entries it moves (three inputs read, two
outputs written).  The last line applies the rule that decides the default to the `exp` workload: value v > 0 iff it is faster than
option 0 AND than the parent by more than the largest block spread, and option 0 equals the parent within that spread; 2 only if it
also beats 1 by more than the spread (and is not slower than 0 on `cheby` by more than the spread).  Prints JSON lines and writes
them to --out when given:

    timeout -k 10 1100 python tools/bench_poly_step.py --parent-root /path/to/parent --out profiles/poly_step_bench.json
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
EXP_COEF = [1.266065877752007e+00, 1.130318207984970e+00, 2.714953395340771e-01, 4.433684984866504e-02, 5.474240442092110e-03,
            5.429263119148932e-04, 4.497732295351912e-05, 3.198436462630565e-06, 1.992124801999838e-07, 1.103677287249654e-08,
            5.505891628277851e-10, 2.498021534339559e-11, 1.038827668772902e-12, 4.032447357431817e-14, 2.127980007794583e-15,
            -1.629151584468762e-16]   # (Chebyshev coefficients of exp on [-1, 1]: I_0(1), 2 I_k(1))
WORKLOADS = ("exp", "cheby")


def load(root):
    sys.path.insert(0, root)
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("spgemm_fma", 1)
    return nt


def operands(nt, args):
    """the operand, and the one of the `cheby` workload: scaled into the Chebyshev interval as ComputeExponential scales it"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gen import banded_triplets
    A = nt.Matrix_ps.from_triplets(args.n, *banded_triplets(args.n, args.h, shift=args.shift))
    sigma = 1.0
    while A.Norm() / sigma > 1.0:
        sigma *= 2
    S = nt.Matrix_ps(A)
    S.Scale(1.0 / sigma)
    poly = nt.ChebyshevPolynomial(len(EXP_COEF))
    for k, v in enumerate(EXP_COEF):
        poly.SetCoefficient(k, v)
    return dict(A=A, S=S, sigma=sigma, poly=poly)


def solve(nt, args, ops, workload, opt):
    if opt is not None:
        nt.set_option("poly_step", opt)
    p = nt.SolverParameters()
    p.SetThreshold(args.threshold if workload == "exp" else args.threshold / ops["sigma"])
    K = nt.Matrix_ps(args.n)
    c0 = nt.poly_step_counts() if opt is not None else None
    s0 = nt.slab_algebra_counts()
    nt.synchronize()
    t0 = time.perf_counter()
    if workload == "exp":
        nt.lib.ComputeExponential_wrp(ops["A"].ih, K.ih, p.ih)
    else:
        nt.lib.ChebyshevCompute_wrp(ops["S"].ih, K.ih, ops["poly"].ih, p.ih)
    nt.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    s1 = nt.slab_algebra_counts()
    out = dict(ms=ms, nnz_result=int(K.GetSize()), norm_result=float(K.Norm()), trace_result=float(K.Trace()), slab={k: int(s1[k] - s0[k]) for k in s1})
    if opt is not None:
        c1 = nt.poly_step_counts()
        out["counts"] = {k: c1[k] - c0[k] for k in c1}
    return out


def the_pass(nt, args, ops):
    """the pass alone: the operands of step --pass-step of the `cheby` workload, built with the vocabulary; --pass-reps calls of the
    diagnostic entry point"""
    nt.set_option("poly_step", 2)
    n, thr, X = args.n, args.threshold / ops["sigma"], ops["S"]
    Tkm2, Tkm1, R, P, TkOut, ROut = (nt.Matrix_ps(n) for _ in range(6))
    Tkm2.FillIdentity()
    Tkm1 = nt.Matrix_ps(X)
    R.FillIdentity()
    R.Scale(EXP_COEF[0])
    R.Increment(Tkm1, EXP_COEF[1], 0.0)
    for k in range(2, args.pass_step):   # steps 2 .. pass_step - 1 with the vocabulary
        Tk = nt.Matrix_ps(n)
        Tk.Gemm(X, Tkm1, None, 2.0, 0.0, thr)
        Tk.Increment(Tkm2, -1.0, 0.0)
        R.Increment(Tk, EXP_COEF[k], 0.0)
        Tkm2, Tkm1 = Tkm1, Tk
    P.Gemm(X, Tkm1, None, 2.0, 0.0, thr)
    c = EXP_COEF[args.pass_step]
    out = dict(step=args.pass_step, note="a host clock around the diagnostic call: the span and scan launches, the pass, its read-back AND the packing "
               "of both outputs into the result handles -- an upper bound of the pass's own time")
    with nt.solver_session(False):
        if not nt.poly_step(P, Tkm2, R, -1.0, c, TkOut, ROut):   # (untimed: the operands enter slab form)
            out["pass"] = "refused"
            return out
        times = []
        for _ in range(args.pass_reps):
            nt.synchronize()
            t0 = time.perf_counter()
            nt.poly_step(P, Tkm2, R, -1.0, c, TkOut, ROut)
            nt.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    ms = statistics.median(times)
    read = [int(M.GetSize()) for M in (P, Tkm2, R)]
    written = [int(TkOut.GetSize()), int(ROut.GetSize())]
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
    ap.add_argument("--threshold", type=float, default=1e-6)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup-blocks", type=int, default=2, help="untimed blocks before the timed ones")
    ap.add_argument("--pass-reps", type=int, default=5)
    ap.add_argument("--pass-step", type=int, default=6, help="the recurrence step whose operands the pass alone is timed on (2 .. 15)")
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
                                  "--threshold", repr(args.threshold)],
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
            for w in WORKLOADS:
                for v in legs:
                    r = run(w, v)   # (untimed: first launches, allocator pools)
                    print("warm-up block", b, w, "leg", v, "%.1f ms" % r["ms"], file=sys.stderr, flush=True)
        runs = {(w, v): [] for w in WORKLOADS for v in legs}
        for b in range(args.blocks):
            for w in WORKLOADS:
                for v in legs:
                    runs[w, v].append(run(w, v))
                    print("block", b, w, "leg", v, "%.1f ms" % runs[w, v][-1]["ms"], file=sys.stderr, flush=True)
        for w in WORKLOADS:
            for v in legs:
                per = [r["ms"] for r in runs[w, v]]
                med = statistics.median(per)
                last = runs[w, v][-1]
                medians[w, v], spreads[w, v] = med, (max(per) - min(per)) / med
                lines.append(json.dumps(dict(
                    workload="%s: N=%d, halfband=%d, shift=%g, threshold=%g, sigma=%g, FMA arithmetic" % (
                        "ComputeExponential" if w == "exp" else "ChebyshevCompute, 16 coefficients of exp, operand / sigma, threshold / sigma",
                        args.n, args.h, args.shift, args.threshold, ops["sigma"]),
                    name=w, poly_step=v, blocks=args.blocks, warmup_blocks=args.warmup_blocks, call_ms=round(med, 2), blocks_call_ms=[round(x, 2) for x in per],
                    spread=round(spreads[w, v], 4), nnz_result=last["nnz_result"], norm_result=last["norm_result"], trace_result=last["trace_result"],
                    poly_step_counts=last.get("counts"), slab_algebra_counts=last["slab"])))
        if 2 in legs:
            lines.append(json.dumps(the_pass(nt, args, ops)))
    finally:
        if child:
            child.stdin.close()
            child.wait(timeout=120)
    spread = max(spreads.values())
    rule = dict(rule="on `exp`: default v > 0 iff option v beats option 0 and the parent by more than the largest block spread AND option 0 equals the "
                     "parent within it; 2 only if it also beats 1 by more than that spread and is not slower than 0 on `cheby` by more than it",
                largest_spread=round(spread, 4), parent_measured=bool(child), unfused_arithmetic="not measured", two_ranks_at_size="not measured")
    gain = lambda w, v, u: (medians[w, u] - medians[w, v]) / medians[w, u]
    have = lambda v: ("exp", v) in medians
    for w in WORKLOADS:
        if have(0) and child:
            rule["%s_option_0_over_parent" % w] = round(medians[w, 0] / medians[w, "parent"] - 1.0, 4)
        for v in (1, 2):
            if have(v):
                rule["%s_gain_of_%d_over" % (w, v)] = {str(u): round(gain(w, v, u), 4) for u in legs if u != v}
    default = 0
    if child and have(0):
        rule["option_0_equals_parent_within_spread"] = bool(abs(medians["exp", 0] - medians["exp", "parent"]) / medians["exp", "parent"] <= spread)
        if rule["option_0_equals_parent_within_spread"]:
            ok = {v: have(v) and gain("exp", v, 0) > spread and gain("exp", v, "parent") > spread for v in (1, 2)}
            if ok[2] and (not have(1) or gain("exp", 2, 1) > spread) and gain("cheby", 2, 0) > -spread:
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
