#!/usr/bin/env python3
"""WOM_GC in a slab session (option wom_session), measured on the headline operand (tests/gen.py banded_triplets(262144, 100)), FMA
arithmetic, ISQ = I, mu = 0, threshold 1e-8, step_thresh at its default, --inv-temp chosen so that at least four steps are accepted.

Four legs: option 2 (the session with the Heun tail and the dots in one pass each), option 1 (the session with the vocabulary
calls), option 0 (the loop on compressed columns) and -- with --parent-root DIR, a built checkout of the parent commit -- the
parent's library, which does not know the option.  The block scheme of DESIGN.md section 6: one untimed warm-up block, then
--blocks timed blocks; a block = the solve once with each leg, in turn, so that whatever else the machine does meets all legs
alike.  The parent runs in ONE child process that imports the package from DIR, builds the same operand once and then runs one
solve per line it is sent; it idles while this process measures, and the other way round.  Every leg calls the solver through the
C ABI (WOM_GC_wrp).

The figure is a host clock around the whole solver call, which ends in a device synchronise, divided by the number of TRIALS
(gradient evaluations minus accepted steps; set-up and the closing similarity transform are inside, the same for every leg: the
parent records no trace, so its trial count is taken from option 0's, whose loop it is).  Per leg the MEDIAN block is reported,
all blocks are listed, spread = (max - min) / median.  The Heun pass alone is timed through its diagnostic entry point on operands of the loop's kind
built here by the vocabulary (heun_pass below), with its fraction of the HBM peak over the five runs it moves.  The last
line applies the rule that decides the default: 2 iff option 2 is faster than option 0 AND than the parent by more than the
largest block spread, and option 0 equals the parent within that spread.  Prints JSON lines and writes them to --out when given:

    timeout -k 10 1100 python tools/bench_wom_session.py --parent-root /path/to/parent --out profiles/wom_session_bench.json
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
    H = nt.Matrix_ps.from_triplets(args.n, *banded_triplets(args.n, args.h))
    I = nt.Matrix_ps(args.n)
    I.FillIdentity()
    return H, I


def solve(nt, args, H, I, opt):
    if opt is not None:
        nt.set_option("wom_session", opt)
    p = nt.SolverParameters()
    p.SetThreshold(args.threshold)
    K = nt.Matrix_ps(args.n)
    dd = lambda x: C.byref(C.c_double(x))
    e = C.c_double()
    c0 = nt.wom_session_counts() if opt is not None else None
    s0 = nt.slab_algebra_counts()
    nt.synchronize()
    t0 = time.perf_counter()
    nt.lib.WOM_GC_wrp(H.ih, I.ih, K.ih, dd(args.mu), dd(args.inv_temp), C.byref(e), p.ih)
    nt.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    c1 = nt.wom_session_counts() if opt is not None else None
    s1 = nt.slab_algebra_counts()
    out = dict(ms=ms, energy=float(e.value), nnz_density=int(K.GetSize()), slab={k: int(s1[k] - s0[k]) for k in s1})
    if opt is not None:   # (the parent's solver records no trace)
        tr = nt.solver_trace()
        out.update(trials=int(tr["iterations"]), accepted=len(set(tr["energy"].tolist())), nnz_end=int(tr["nnz"][-1]),
                   steps=[float(s) for s in tr["sigma"]], counts={k: c1[k] - c0[k] for k in c1})
    return out


def heun_pass(nt, args, H, I):
    """the Heun pass alone.  The solver does not keep a trial's operands, so operands of the loop's kind are built here from the
    Hamiltonian by the vocabulary at the solve's threshold: W = I / sqrt(2) + 0.1 H, K0 = -0.5 H W, RK1 = W + h K0, K1 = -0.5 H RK1
    (runs two and three times the Hamiltonian's width), and --heun-reps calls of the diagnostic entry point are timed on them"""
    thr, h = args.threshold, 0.5
    nt.set_option("wom_session", 2)
    W = nt.Matrix_ps(I)
    W.Scale(2.0 ** -0.5)
    W.Increment(H, 0.1, thr)
    K0, K1, T = nt.Matrix_ps(args.n), nt.Matrix_ps(args.n), nt.Matrix_ps(args.n)
    K0.Gemm(H, W, None, -0.5, 0.0, thr)
    RK1 = nt.Matrix_ps(K0)
    RK1.Scale(h)
    RK1.Increment(W, 1.0, thr)
    K1.Gemm(H, RK1, None, -0.5, 0.0, thr)
    entries = [int(M.GetSize()) for M in (W, K0, K1, RK1)]
    times = []
    with nt.solver_session(False):
        got = nt.wom_heun_step(W, K0, K1, RK1, h, thr, T)   # (untimed: the operands enter slab form)
        if got is None:
            return dict(heun_pass="refused")
        for _ in range(args.heun_reps):
            nt.synchronize()
            t0 = time.perf_counter()
            nt.wom_heun_step(W, K0, K1, RK1, h, thr, T)
            nt.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    entries.append(int(T.GetSize()))
    ms = statistics.median(times)
    gb = 8.0 * sum(entries) / 1e9
    return dict(heun_pass_ms=round(ms, 3), heun_pass_blocks=[round(t, 3) for t in times], entries_moved=entries,
                note="a host clock around the diagnostic call: the span and scan launches, the pass, its read-back AND the packing of RK2 into the result handle -- an upper bound of the pass's own time",
                gb_moved_counted_on_entries=round(gb, 3), fraction_of_hbm_peak=round(gb / (ms * 1e-3) / HBM_PEAK_GBS, 3), err=got[0], err2=got[1])


def serve(args):
    """the parent's library: one solve per line on stdin, one JSON line back; ends at end of input"""
    nt = load(args.root)
    H, I = operand(nt, args)
    print(json.dumps(dict(ready=True)), flush=True)
    for line in sys.stdin:
        if not line.strip():
            break
        print(json.dumps(solve(nt, args, H, I, None)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--h", type=int, default=100)
    ap.add_argument("--threshold", type=float, default=1e-8)
    ap.add_argument("--mu", type=float, default=0.0)
    ap.add_argument("--inv-temp", type=float, default=1.0)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--heun-reps", type=int, default=5)
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
                                  "--mu", repr(args.mu), "--inv-temp", repr(args.inv_temp)],
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
    H, I = operand(nt, args)

    def run(v):
        if v == "parent":
            child.stdin.write("solve\n")
            child.stdin.flush()
            return child_line()
        return solve(nt, args, H, I, v)

    lines, medians, spreads = [], {}, {}
    try:
        for v in legs:
            run(v)   # (untimed: first launches, allocator pools)
        runs = {v: [] for v in legs}
        for b in range(args.blocks):
            for v in legs:
                runs[v].append(run(v))
                print("block", b, "leg", v, "%.1f ms" % runs[v][-1]["ms"], file=sys.stderr, flush=True)
        trials0 = runs[0][-1]["trials"] if 0 in runs else None
        for v in legs:
            trials = [r.get("trials", trials0) for r in runs[v]]
            if any(t is None for t in trials):
                raise RuntimeError("the parent's trial count needs option 0 among --options")
            per = [r["ms"] / t for r, t in zip(runs[v], trials)]
            med = statistics.median(per)
            last = runs[v][-1]
            medians[v], spreads[v] = med, (max(per) - min(per)) / med
            lines.append(json.dumps(dict(
                workload="WOM_GC: banded N=%d halfband=%d, ISQ = I, mu=%g, inv_temp=%g, threshold=%g, FMA arithmetic" % (
                    args.n, args.h, args.mu, args.inv_temp, args.threshold),
                wom_session=v, blocks=args.blocks, trials=trials[-1], accepted=last.get("accepted"), ms_per_trial=round(med, 3),
                blocks_ms_per_trial=[round(x, 3) for x in per], spread=round(spreads[v], 4),
                call_ms=round(statistics.median(r["ms"] for r in runs[v]), 2), energy=last["energy"], nnz_density=last["nnz_density"],
                nnz_rk2_end=last.get("nnz_end"), steps=last.get("steps"), wom_session_counts=last.get("counts"), slab_algebra_counts=last["slab"])))
        if 2 in legs:
            lines.append(json.dumps(heun_pass(nt, args, H, I)))
    finally:
        if child:
            child.stdin.close()
            child.wait(timeout=120)
    spread = max(spreads[v] for v in legs)
    rule = dict(rule="default 2 iff option 2 beats option 0 and the parent by more than the largest block spread AND option 0 equals the parent within it",
                largest_spread=round(spread, 4), parent_measured=bool(child), unfused_arithmetic="not measured", two_ranks_at_size="not measured")
    if 0 in medians and child:
        rule["option_0_over_parent"] = round(medians[0] / medians["parent"] - 1.0, 4)
        rule["option_0_equals_parent_within_spread"] = bool(abs(medians[0] - medians["parent"]) / medians["parent"] <= spread)
    if 2 in medians:
        gains = {str(v): round((medians[v] - medians[2]) / medians[v], 4) for v in legs if v != 2}
        rule["gain_of_2_over"] = gains
        rule["default"] = 2 if (child and 0 in medians and gains["0"] > spread and gains["parent"] > spread and
                                rule["option_0_equals_parent_within_spread"]) else 0
    lines.append(json.dumps(rule))
    for ln in lines:
        print(ln)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
