#!/usr/bin/env python3
"""PolarDecomposition in a slab session (option slab_transpose), measured on a non-Hermitian band: tests/gen.py
banded_triplets(n, max(hl, hu), shift=2.5) with the entries -hu <= row - col <= hl kept and those above the diagonal halved,
threshold 1e-8, convergence 1e-8, FMA arithmetic (--unfused: the real legs in unfused arithmetic).

Real legs (N = 262144, (hl, hu) = (100, 50)): option 0 (the loop on compressed columns: pack, sort-transpose, two products from
compressed columns, merge and norm per iteration), option 1 (the iterate stays in slab form: the tiled transpose of slab_extra.hip,
two products on the tile kernel's operand form) and -- with --parent-root DIR, a built checkout of the parent commit -- the parent's
library, which does not know the option.  Complex legs (--complex: configs[4]'s shape, N = 131072 with half bandwidth 50, made
non-Hermitian the same way, (hl, hu) = (50, 25)): option 1 (the complex loop on compressed columns) and option 2 (the complex
session).  Each leg runs in a process of its own, which imports the package (from DIR for the parent), builds the same operand once
and then runs one solve per line it is sent; it idles while another leg measures.  The block scheme of DESIGN.md section 6: one
untimed warm-up block, then --blocks timed blocks; a block = the solve once with each leg, in turn.  Every leg calls the solver
through the C ABI (PolarDecomposition_wrp).

The figure is a host clock around the whole solver call, which ends in a device synchronise, divided by the iteration count (set-up
and Hm = U^H A are inside, the same for every leg).  Per leg the MEDIAN block is reported, all blocks are listed, spread = (max -
min) / median.  --pass: one more process measures the transpose pass alone on the product X X of the real operand in slab form,
between two HIP events on the engine's stream (option time_kernels with NTPOLY_AMD_DEBUG_SPGEMM: the library prints the time and
the bytes it read and wrote), median of --blocks calls, and (bytes read + written) / time as a fraction of the 8 TB/s HBM peak -- a
number, no target.  The last line states the medians' ratios and whether the session is slower than a leg without it by more than
the largest block spread (the rule that decides the option's default).  Prints JSON lines and writes them to --out when given:

    timeout -k 10 1100 python tools/bench_polar_session.py --parent-root /path/to/parent --pass --out profiles/polar_session_bench.json
"""
import argparse
import ctypes as C
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


def load(root, unfused=False):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("spgemm_fma", 0 if unfused else 1)
    return nt


def triplets(n, hl, hu, cplx):
    import numpy as np
    from gen import banded_triplets
    col, row, val = banded_triplets(n, max(hl, hu), shift=2.5, complex_=cplx)
    d = row.astype(np.int64) - col
    keep = (d >= -hu) & (d <= hl)
    val = np.where(d < 0, 0.5 * val, val)
    return col[keep], row[keep], val[keep]


def solve(nt, args, A, opt):
    if opt is not None:
        nt.set_option("slab_transpose", opt)
    p = nt.SolverParameters()
    p.SetThreshold(args.threshold)
    p.SetConvergeDiff(args.converge)
    U, Hm = nt.Matrix_ps(args.n), nt.Matrix_ps(args.n)
    c0 = nt.slab_transpose_counts() if opt is not None else None
    s0 = nt.slab_algebra_counts()
    nt.synchronize()
    t0 = time.perf_counter()
    nt.lib.PolarDecomposition_wrp(A.ih, U.ih, Hm.ih, p.ih)
    nt.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    tr = nt.solver_trace()
    c1 = nt.slab_transpose_counts() if opt is not None else None
    s1 = nt.slab_algebra_counts()
    return dict(ms=ms, iters=int(tr["iterations"]), last_norm=float(tr["value"][-1]), nnz_end=int(tr["nnz"][-1]),
                counts={k: c1[k] - c0[k] for k in c1} if c1 else None, slab={k: int(s1[k] - s0[k]) for k in s1})


def serve(args):
    """one leg: one solve per line on stdin, one JSON line back; ends at end of input"""
    nt = load(args.root, args.unfused)
    A = nt.Matrix_ps.from_triplets(args.n, *triplets(args.n, args.hl, args.hu, args.complex))
    opt = None if args.serve_option < 0 else args.serve_option   # (the parent's library does not know the option)
    print(json.dumps(dict(ready=True)), flush=True)
    for line in sys.stdin:
        if not line.strip():
            break
        print(json.dumps(solve(nt, args, A, opt)), flush=True)


def serve_pass(args):
    """the transpose pass alone: X X left in slab form by the C ABI's product, then TransposeMatrix between two HIP events"""
    os.environ["NTPOLY_AMD_DEBUG_SPGEMM"] = "1"
    nt = load(args.root, args.unfused)
    nt.set_option("slab_transpose", 1)
    X = nt.Matrix_ps.from_triplets(args.n, *triplets(args.n, args.hl, args.hu, args.complex))
    P, T = nt.Matrix_ps(args.n), nt.Matrix_ps(args.n)
    P.Gemm(X, X, None, 1.0, 0.0, args.threshold)
    nt.set_option("time_kernels", 1)
    nt.synchronize()
    with tempfile.TemporaryFile(mode="w+") as f:   # (the library writes the figure to stderr)
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            c0 = nt.slab_transpose_counts()
            for _ in range(args.blocks + 1):
                T.Transpose(P)
            nt.synchronize()
            c1 = nt.slab_transpose_counts()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read()
    got = [(float(m.group(1)), float(m.group(2))) for m in re.finditer(r"\[slab transpose\] timed: .* bytes (\d+) ms ([0-9.]+)", text)]
    nt.set_option("time_kernels", 0)
    ms = [g[1] for g in got[1:]]   # (the first call is the warm-up)
    out = dict(transposes=c1["transposes"] - c0["transposes"], calls_timed=len(ms))
    if ms:
        med = statistics.median(ms)
        out.update(pass_ms=round(med, 4), pass_ms_all=[round(x, 4) for x in ms], bytes=int(got[-1][0]), nnz=int(P.GetSize()),
                   gbs=round(got[-1][0] / med / 1e6, 1), hbm_fraction=round(got[-1][0] / med / 1e6 / HBM_PEAK_GBS, 4))
    print(json.dumps(out), flush=True)


class Leg:
    """a child process that measures one leg; it idles while the others measure"""

    def __init__(self, args, name, root, option, mode="--serve"):
        self.name = name
        # (a time limit of its own: a child that hangs ends, and the blocking read below then sees the end of its output)
        self.p = subprocess.Popen(["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), mode,
                                   "--serve-option", str(option), "--root", os.path.abspath(root), "--n", str(args.n), "--hl", str(args.hl),
                                   "--hu", str(args.hu), "--threshold", repr(args.threshold), "--converge", repr(args.converge),
                                   "--blocks", str(args.blocks)] + (["--complex"] if args.complex else []) + (["--unfused"] if args.unfused else []),
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def line(self):
        while True:
            ln = self.p.stdout.readline()
            if not ln:
                raise RuntimeError("the process of leg %s ended early (exit code %s)" % (self.name, self.p.poll()))
            if ln.startswith("{"):
                return json.loads(ln)

    def run(self):
        self.p.stdin.write("solve\n")
        self.p.stdin.flush()
        return self.line()

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=120)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--complex", action="store_true", help="the complex legs (options 1 and 2) on configs[4]'s shape")
    ap.add_argument("--unfused", action="store_true", help="the real legs in unfused arithmetic (complex sessions need FMA arithmetic)")
    ap.add_argument("--n", type=int, default=0, help="default 262144, with --complex 131072")
    ap.add_argument("--hl", type=int, default=0, help="default 100, with --complex 50")
    ap.add_argument("--hu", type=int, default=0, help="default 50, with --complex 25")
    ap.add_argument("--threshold", type=float, default=1e-8)
    ap.add_argument("--converge", type=float, default=1e-8)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--options", type=int, nargs="+", default=None, choices=[0, 1, 2], help="the option's values measured, in block order")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit: measured as one more leg")
    ap.add_argument("--pass", dest="pass_", action="store_true", help="also the transpose pass alone, between HIP events")
    ap.add_argument("--child-timeout", type=int, default=800, help="seconds after which a leg's process is ended")
    ap.add_argument("--out", default="", help="file the JSON lines are written to (replaced)")
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--serve-pass", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--serve-option", type=int, default=-1, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.n = args.n or (131072 if args.complex else 262144)
    args.hl = args.hl or (50 if args.complex else 100)
    args.hu = args.hu or (25 if args.complex else 50)
    if args.serve:
        return serve(args)
    if args.serve_pass:
        return serve_pass(args)
    base, session = (1, 2) if args.complex else (0, 1)   # (the leg without the session, the leg with it)
    legs = list(dict.fromkeys(args.options or [session, base])) + (["parent"] if args.parent_root else [])
    what = "Polar: %s non-Hermitian band N=%d (hl, hu)=(%d, %d), threshold=%g, convergence=%g, %s arithmetic" % (
        "complex" if args.complex else "real", args.n, args.hl, args.hu, args.threshold, args.converge, "unfused" if args.unfused else "FMA")
    procs = {}
    lines, medians, spreads = [], {}, {}
    try:
        for v in legs:   # (one after the other: each builds its operand while nothing is being timed)
            procs[v] = Leg(args, str(v), args.parent_root if v == "parent" else ROOT, -1 if v == "parent" else v)
            procs[v].line()   # (ready)
        for v in legs:
            procs[v].run()   # (untimed: first launches, allocator pools)
        runs = {v: [] for v in legs}
        for _ in range(args.blocks):
            for v in legs:
                runs[v].append(procs[v].run())
        for v in legs:
            per = [r["ms"] / r["iters"] for r in runs[v]]
            med = statistics.median(per)
            last = runs[v][-1]
            medians[v], spreads[v] = med, (max(per) - min(per)) / med
            lines.append(json.dumps(dict(
                workload=what, slab_transpose=v, blocks=args.blocks, iterations=last["iters"], ms_per_iteration=round(med, 3),
                blocks_ms_per_iteration=[round(x, 3) for x in per], spread=round(spreads[v], 4),
                call_ms=round(statistics.median(r["ms"] for r in runs[v]), 2), last_norm=last["last_norm"], nnz_end=last["nnz_end"],
                slab_transpose_counts=last["counts"], slab_algebra_counts=last["slab"])))
    finally:
        for leg in procs.values():
            leg.close()
    if args.pass_:
        leg = Leg(args, "pass", ROOT, 1, mode="--serve-pass")
        try:
            lines.append(json.dumps(dict(workload="transpose pass on X X of: " + what, **leg.line())))
        finally:
            leg.close()
    spread = max(spreads[v] for v in legs)
    summary = dict(summary="medians compared", largest_spread=round(spread, 4), parent_measured="parent" in medians)
    if base in medians and "parent" in medians:
        summary["option_%d_over_parent" % base] = round(medians[base] / medians["parent"] - 1.0, 4)
    if session in medians:
        gains = {str(v): round((medians[v] - medians[session]) / medians[v], 4) for v in legs if v != session}
        summary["gain_of_%d_over" % session] = gains
        summary["option_%d_not_slower_than_any_by_more_than_the_spread" % session] = bool(gains and all(g >= -spread for g in gains.values()))
    lines.append(json.dumps(summary))
    for ln in lines:
        print(ln)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
