#!/usr/bin/env python3
"""PurificationExtrapolate in a slab session (option purify_session), measured on the family of tests/test_gpu_purify_session.py
at size: N = 262 144, D_ii = 0.9 where ((i 7919) mod 1000) < 500 else 0.1, D_ij = -0.02 exp(-0.05 k) / k for 0 < k = |i - j| <=
--h (100), S = I + 0.05 exp(-0.5 k) / k for 0 < k <= 3, trace = the number of occupied sites, threshold 1e-8, FMA arithmetic, a fixed
number of iterations (--iters, converge_diff tiny, no monitor).

Four legs: option 2 (the session with the tail of an iteration in one pass), option 1 (the session with the vocabulary calls),
option 0 (the loop on compressed columns) and -- with --parent-root DIR, a built checkout of the parent commit -- the parent's
library, which does not know the option.  The block scheme of DESIGN.md section 6: one untimed warm-up block, then --blocks timed
blocks; a block = the solve once with each leg, in turn, so that whatever else the machine does meets all legs alike.  The parent
runs in ONE child process that imports the package from DIR, builds the same operands once and then runs one solve per line it is
sent; it idles while this process measures, and the other way round.  Every leg calls the solver through the C ABI
(PurificationExtrapolate_wrp).

The figure is a host clock around the whole solver call, which ends in a device synchronise, divided by the number of iterations
(set-up and the load balancer's bookkeeping are inside, the same for every leg).  Per leg the MEDIAN block is reported, all blocks
are listed, spread = (max - min) / median.  The pass alone is timed through its diagnostic entry point, in either branch, on D, N =
the product D S D at the solve's threshold and S (tail_pass below), with its fraction of the HBM peak over the runs it moves (three
read, one written in the fold branch).  The last line applies the rule that decides the default: the fastest non-zero value iff it
is faster than option 0 AND than the parent by more than the largest block spread, and option 0 equals the parent within that
spread (2 only if it also beats 1 by more than the spread).  Prints JSON lines and writes them to --out when given:

    timeout -k 10 1100 python tools/bench_purify_session.py --parent-root /path/to/parent --out profiles/purify_session_bench.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0   # MI355X


def load(root):
    sys.path.insert(0, root)
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("spgemm_fma", 1)
    return nt


def band(n, h, diag, off):
    """(col, row, val), 1-based, sorted by column then row (tests/gen.py banded_triplets with other values)"""
    i = np.arange(1, n + 1, dtype=np.int64)
    offs = np.arange(-h, h + 1)
    col = np.repeat(i, len(offs))
    row = col + np.tile(offs, n)
    ok = (row >= 1) & (row <= n)
    col, row = col[ok], row[ok]
    dist = np.abs(row - col).astype(np.float64)
    val = np.where(dist == 0, diag[col - 1], off(np.maximum(dist, 1.0)))
    return col.astype(np.int32), row.astype(np.int32), val


def operand(nt, args):
    i = np.arange(1, args.n + 1, dtype=np.int64)
    occ = ((i * 7919) % 1000) < 500
    D = nt.Matrix_ps.from_triplets(args.n, *band(args.n, args.h, np.where(occ, 0.9, 0.1), lambda k: -0.02 * np.exp(-0.05 * k) / k))
    S = nt.Matrix_ps.from_triplets(args.n, *band(args.n, 3, np.ones(args.n), lambda k: 0.05 * np.exp(-0.5 * k) / k))
    return D, S, float(occ.sum())


def solve(nt, args, D, S, trace, opt):
    if opt is not None:
        nt.set_option("purify_session", opt)
    p = nt.SolverParameters()
    p.SetThreshold(args.threshold)
    p.SetConvergeDiff(1e-300)
    p.SetMaxIterations(args.iters)
    p.SetMonitorConvergence(False)
    K = nt.Matrix_ps(args.n)
    c0 = nt.purify_session_counts() if opt is not None else None
    s0 = nt.slab_algebra_counts()
    nt.synchronize()
    t0 = time.perf_counter()
    nt.lib.PurificationExtrapolate_wrp(D.ih, S.ih, C.byref(C.c_double(trace)), K.ih, p.ih)
    nt.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    c1 = nt.purify_session_counts() if opt is not None else None
    s1 = nt.slab_algebra_counts()
    out = dict(ms=ms, nnz_density=int(K.GetSize()), trace_density_overlap=float(K.Dot(S)), slab={k: int(s1[k] - s0[k]) for k in s1})
    if opt is not None:   # (the parent's solver records no trace)
        tr = nt.solver_trace()
        out.update(iterations=int(tr["iterations"]), branches="".join("+" if s > 0 else "-" for s in tr["sigma"]),
                   norm_end=float(tr["value"][-1]), counts={k: c1[k] - c0[k] for k in c1})
    return out


def tail_pass(nt, args, D, S):
    """the pass alone, either branch: N = the product D S D at the solve's threshold, --pass-reps calls of the diagnostic entry
    point timed on D, N and S"""
    nt.set_option("purify_session", 2)
    T, N, O = nt.Matrix_ps(args.n), nt.Matrix_ps(args.n), nt.Matrix_ps(args.n)
    T.Gemm(D, S, None, 1.0, 0.0, args.threshold)
    N.Gemm(T, D, None, 1.0, 0.0, args.threshold)
    read = [int(M.GetSize()) for M in (D, N, S)]
    out = dict(entries_read=read, note="a host clock around the diagnostic call: the span and scan launches (fold), the pass, its read-back AND the "
               "packing of N' into the result handle -- an upper bound of the pass's own time")
    with nt.solver_session(False):
        for fold, tag in ((1, "fold"), (0, "plain")):
            got = nt.purify_tail_step(D, N, S, fold, O)   # (untimed: the operands enter slab form)
            if got is None:
                out[tag] = "refused"
                continue
            times = []
            for _ in range(args.pass_reps):
                nt.synchronize()
                t0 = time.perf_counter()
                nt.purify_tail_step(D, N, S, fold, O)
                nt.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            ms = statistics.median(times)
            written = int(O.GetSize()) if fold else 0
            gb = 8.0 * (sum(read) + written) / 1e9
            out[tag] = dict(pass_ms=round(ms, 3), pass_blocks=[round(t, 3) for t in times], entries_written=written,
                            gb_moved_counted_on_entries=round(gb, 3), fraction_of_hbm_peak=round(gb / (ms * 1e-3) / HBM_PEAK_GBS, 3),
                            norm=got[0], next_trace=got[1])
    return out


def serve(args):
    """the parent's library: one solve per line on stdin, one JSON line back; ends at end of input"""
    nt = load(args.root)
    D, S, trace = operand(nt, args)
    print(json.dumps(dict(ready=True)), flush=True)
    for line in sys.stdin:
        if not line.strip():
            break
        print(json.dumps(solve(nt, args, D, S, trace, None)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--h", type=int, default=100)
    ap.add_argument("--threshold", type=float, default=1e-8)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=5)
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
                                  os.path.abspath(args.parent_root), "--n", str(args.n), "--h", str(args.h), "--threshold", repr(args.threshold),
                                  "--iters", str(args.iters)],
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
    D, S, trace = operand(nt, args)

    def run(v):
        if v == "parent":
            child.stdin.write("solve\n")
            child.stdin.flush()
            return child_line()
        return solve(nt, args, D, S, trace, v)

    lines, medians, spreads = [], {}, {}
    try:
        for v in legs:
            run(v)   # (untimed: first launches, allocator pools)
        runs = {v: [] for v in legs}
        for b in range(args.blocks):
            for v in legs:
                runs[v].append(run(v))
                print("block", b, "leg", v, "%.1f ms" % runs[v][-1]["ms"], file=sys.stderr, flush=True)
        for v in legs:
            its = [r.get("iterations", args.iters) for r in runs[v]]   # (the parent: no trace; the count is fixed by --iters)
            per = [r["ms"] / t for r, t in zip(runs[v], its)]
            med = statistics.median(per)
            last = runs[v][-1]
            medians[v], spreads[v] = med, (max(per) - min(per)) / med
            lines.append(json.dumps(dict(
                workload="PurificationExtrapolate: N=%d, D halfband=%d, S halfband=3, trace=%g, threshold=%g, %d iterations, FMA arithmetic" % (
                    args.n, args.h, trace, args.threshold, args.iters),
                purify_session=v, blocks=args.blocks, iterations=its[-1], branches=last.get("branches"), ms_per_iteration=round(med, 3),
                blocks_ms_per_iteration=[round(x, 3) for x in per], spread=round(spreads[v], 4),
                call_ms=round(statistics.median(r["ms"] for r in runs[v]), 2), nnz_density=last["nnz_density"],
                trace_density_overlap=last["trace_density_overlap"], norm_end=last.get("norm_end"), purify_session_counts=last.get("counts"),
                slab_algebra_counts=last["slab"])))
        if 2 in legs:
            lines.append(json.dumps(tail_pass(nt, args, D, S)))
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
