#!/usr/bin/env python3
"""Complex products of the grouped LDS-hash kernel on the matrix cores (option ghash_mfma_complex), measured: ONE product A * A of
configs[4]'s operand -- the complex Hermitian band, N = 131 072, h = 50, threshold 1e-8 -- under the seed-42 relabelling AS IT
STANDS: the block path off (block_path = 0) and the grouped kernel forced (spgemm_variant = 500), FMA arithmetic with complex_tile
(the library's defaults), option 0 (the reference's complex multiply-add on the vector units) against option 1 (table class 0 on
the FP64 matrix cores, two FMA chains per part of an entry).

The block and median scheme of DESIGN.md section 6: one untimed warm-up block, then --blocks timed blocks; a block = the product
once with each option, a host clock around a call that ends in a device synchronise (wall) and the engine's own event timers
around the numeric launches (option time_kernels: kernel).  The MEDIAN block is reported per option, all blocks are listed, the
spread is (max - min) / median of the wall times.  Prints one JSON line per option and appends them to --out when given:

    timeout -k 10 900 python tools/bench_complex_ghash.py --out profiles/complex_ghash_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--h", type=int, default=50)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--threshold", type=float, default=1e-8)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default="", help="file the JSON lines are written to (replaced)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ntpoly_amd as nt
    from gen import permuted_banded_triplets
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("spgemm_fma", 1)
    nt.set_option("complex_tile", 1)
    nt.set_option("block_path", 0)
    nt.set_option("spgemm_variant", 500)
    nt.set_option("time_kernels", 1)
    n = args.n
    A = nt.Matrix_ps.from_triplets(n, *permuted_banded_triplets(n, args.h, args.seed, complex_=True))

    def product(opt):
        nt.set_option("ghash_mfma_complex", opt)
        C = nt.Matrix_ps(n)
        nt.synchronize()
        c0 = nt.ghash_class_counts()
        t0 = time.perf_counter()
        C.Gemm(A, A, None, 1.0, 0.0, args.threshold)
        nt.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        st, gs, c1 = nt.last_spgemm_stats(), nt.last_grouped_stats(), nt.ghash_class_counts()
        assert gs["used"] == 1, gs
        return wall, st["ms_numeric"], st, gs, {k: c1[k] - c0[k] for k in c0}

    for opt in (0, 1):
        product(opt)   # (untimed: first launches, allocator pools, the kept column order)
    wall = {0: [], 1: []}
    kern = {0: [], 1: []}
    last = {}
    for _ in range(args.blocks):
        for opt in (0, 1):
            w, k, st, gs, groups = product(opt)
            wall[opt].append(w)
            kern[opt].append(k)
            last[opt] = (st, gs, groups)
    lines = []
    for opt in (0, 1):
        st, gs, groups = last[opt]
        med = statistics.median(wall[opt])
        lines.append(json.dumps(dict(
            workload="A*A, configs[4] operand under the seed-%d relabelling, grouped kernel forced" % args.seed, ghash_mfma_complex=opt,
            n=n, h=args.h, threshold=args.threshold, blocks=args.blocks,
            kernel_ms=round(statistics.median(kern[opt]), 3), kernel_blocks_ms=[round(x, 3) for x in kern[opt]],
            wall_ms=round(med, 3), wall_blocks_ms=[round(x, 3) for x in wall[opt]],
            wall_spread=round((max(wall[opt]) - min(wall[opt])) / med, 4),
            nnz_c=st["nnz_c"], products=st["products"], groups=gs["groups"], table_class=gs["level"], failed_cols=gs["failed_cols"],
            union_ratio=round(gs["union_ratio"], 3), groups_per_path=groups)))
    for ln in lines:
        print(ln)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
