#!/usr/bin/env python3
"""Headline benchmark: TRS2 density purification on a synthetic banded Hamiltonian
(BASELINE.json configs[2]: N = 262 144, ~200 nnz/row, threshold 1e-8, ISQ = I, trace = N/2).

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
    python bench.py --gpus N ...                 (no launcher: starts its own N rank processes)

A "step" is one TRS2 iteration, driven through the engine's C ABI exactly as
DensityMatrixSolversModule.F90:380-413 does it: trace(X) -> sigma, X2 = X*X (SpGEMM with threshold),
X <- 2X - X2 or X2, energy = dot(X, H).  All matrices stay in HBM; only scalars return to the host.
W warm-up iterations are followed by exactly K timed ones (barrier + device synchronise on both
sides, max over ranks); the region is repeated --blocks times from X0 and the MEDIAN block is reported.
The iterations are those of a solve: the solver stops once X has converged (iteration ~45 on the headline operand), and
iterating past that point only amplifies rounding noise until X fills in without bound.  So the iterate restarts from X0
after every TRS2_WINDOW iterations (warm-up included), outside the clock; W + K <= TRS2_WINDOW never restarts.
Rank 0 prints ONE JSON line.

A plain run does only what that line's headline needs: setup, warm-up, the timed blocks, --dump-outputs, the line.  --full
adds the measurements and checks that take runs of their own (cpu_baseline, trs2_wrp_check and, for a relabelled or 3-D
operand on several ranks, the solver path's rate); --no-cpu-baseline / --no-wrp-check leave one of them out of a --full run.

Extra objects in the line:
  roofline     -- the dominant kernel (SpGEMM numeric phase with the TRS2 update in its epilogue: k_spgemm_tile on the FP64
                  matrix cores in the default FMA arithmetic, k_spgemm_slab in unfused arithmetic, k_bs_numeric / k_spgemm_ghash
                  for operands without runs): algorithmic bytes 12*(nnzA+nnzB+nnzC)+4*(cols...) per launch / its HIP-event
                  time on the engine's stream, vs 8 TB/s HBM; traffic = the committed PMC passes of the same command
  roofline_compute -- the same launches against the FP64 peak of the arithmetic mode
  cpu_baseline -- (--full) the oracle (C restatement with OpenMP, kind "port") on all host cores at the FULL size: ONE
                  solve of warmup + 5 iterations, the last five timed one by one, median -- reported, not the target
  trs2_wrp_check -- (--full) the same rate measured through the reference's entry point TRS2_wrp ((t(25) - t(5)) / 20)

Other workloads: --permute SEED (the operand under the load balancer's random relabelling), --random SEED (the same
operand left AS IT STANDS -- no band recovery, no block order: the north star's LDS-hash SpGEMM, the shape of the
reference's own UnitTests/bench.f90:58-76), --lattice L (3-D Hamiltonian), --config 3 (BASELINE configs[3]: one A*A at
N = 1 048 576), --arithmetic fma|unfused, --set OPTION=VALUE.

--dump-outputs DIR writes what the timed path computed in its last timed step (the last block's) as DIR/<name>.npy,
float64: the scalars the step returned and DUMP_COLUMNS whole columns of the resulting matrix, dense, at column indices
drawn with a fixed seed -- the same columns for the same arguments, so that two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# RCCL between processes needs dmabuf IPC on this driver stack (already exported on the GPU boxes; kept for other launchers)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
TRS2_WINDOW = 40          # iterations from X0 before the iterate restarts (the headline converges at ~45, fills in from ~53)
DUMP_COLUMNS = 16         # --dump-outputs: dense columns of the result (16 x 8 B x N: 32 MB at N = 262 144)
DUMP_SEED = 20260101
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(directory, M, n, scalars):
    """--dump-outputs: `scalars` (name -> float) and DUMP_COLUMNS dense columns of the distributed matrix M at seeded
    column indices, as float64 .npy files under `directory` (one rank: every column is local)"""
    cols = np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=min(DUMP_COLUMNS, n), replace=False))
    while 8 * len(cols) * n > DUMP_LIMIT_BYTES - (1 << 20):
        cols = cols[::2]
    col, row, val = M.triplets()            # 1-based, sorted by column then row
    dense = np.zeros((len(cols), n), dtype=np.float64)
    lo = np.searchsorted(col, cols + 1, side="left")
    hi = np.searchsorted(col, cols + 1, side="right")
    for k in range(len(cols)):
        dense[k, row[lo[k]:hi[k]] - 1] = np.real(val[lo[k]:hi[k]])
    del col, row, val
    out = {"column_index": cols.astype(np.float64), "columns": dense}
    out.update((k, np.array([v], dtype=np.float64)) for k, v in scalars.items())
    os.makedirs(directory, exist_ok=True)
    for k, a in out.items():
        np.save(os.path.join(directory, k + ".npy"), a)


def trs2_step(nt, X, X2, WH, pool, trace_target, thr, trace_x=None):
    """one iteration of DensityMatrixSolversModule.F90:380-413, exactly the body TRS2_wrp loops over
    (ntpoly_amd_trs2_step = csrc/solvers.cpp trs2_step: trace -> sigma, X2 = X*X, fused update + energy + trace of the
    new iterate, which the solver loop hands to the next iteration); returns (sigma, energy, trace of the new X)"""
    return nt.trs2_step(X, X2, WH, trace_target, thr, trace_x)


def trs2_step_unfused(nt, X, X2, WH, pool, trace_target, thr):
    """the same iteration spelled with the reference's individual C-ABI calls (cross-check)"""
    tr = X.Trace()
    sigma = -1.0 if (trace_target - tr) < 0.0 else 1.0
    X2.Gemm(X, X, pool, 1.0, 0.0, thr)
    if sigma > 0.0:
        X.Scale(2.0)
        X.Increment(X2, -1.0, thr)
    else:
        nt.lib.CopyMatrix_ps_wrp(X2.ih, X.ih)
    return sigma, float(np.real(X.Dot(WH)))


def cpu_baseline(n, h, thr, warmup, steps, permute=None, fma=False, lattice=None):
    """the oracle (C restatement with OpenMP, kind "port") at the FULL configuration size on all host cores, in the
    arithmetic mode the GPU line ran in: one TRS2 solve of warmup + 3 iterations; the last three iterations, timed one by
    one, are three samples of the region the GPU line times (setup excluded, as BASELINE.md section 2 measures the
    reference); the value is their median."""
    from oracle import oracle_py as O
    from gen import banded_triplets, permuted_banded_triplets, lattice_triplets
    if lattice is not None:
        col, row, val = lattice_triplets(lattice)
    elif permute is None:
        col, row, val = banded_triplets(n, h)
    else:
        col, row, val = permuted_banded_triplets(n, h, permute)
    H = O.Mat.from_triplets(n, n, col, row, val)
    del col, row, val
    I = O.Mat.identity(n)
    O.set_fma(fma)

    # ONE run of warmup + 3 iterations; the oracle stamps the wall clock at the end of every iteration (otrace.stamp), so
    # the last three differences are three samples of one iteration of the region the GPU line times
    nsamp = 3 if lattice is not None else 5
    iters = min(max(1, warmup), TRS2_WINDOW - nsamp) + nsamp     # (inside the window the GPU line iterates in)
    try:
        p = O.params(converge_diff=1e-30, max_iterations=iters, threshold=thr, monitor_convergence=False)
        _, _, _, tro = O.density("trs2", H, I, n / 2.0, p)
    finally:
        O.set_fma(False)
    st = tro["stamp"]
    samples = sorted(max(1e-9, float(st[k] - st[k - 1])) for k in range(max(1, len(st) - nsamp), len(st)))
    per_iter = samples[len(samples) // 2]
    return {"value": 1.0 / per_iter, "unit": "iters/s", "cores": int(O.lib().oracle_num_threads()),
            "kind": "port",
            "sample": "oracle TRS2 (OpenMP, all host cores, %s arithmetic) at the full size N=%d (h=%d, thr=%g%s): iterations "
                      "%d..%d of one solve, single-iteration samples (wall clock stamped by the oracle after every iteration) = %s s, median %.3f s/iter; "
                      "no scaling" % ("fma" if fma else "unfused", n, h, thr,
                                      (", %d^3 lattice" % lattice) if lattice is not None else
                                      "" if permute is None else ", relabelled with seed %d" % permute, warmup + 1,
                                      warmup + nsamp, "/".join("%.3f" % x for x in samples), per_iter)}


def trs2_wrp_check(nt, H, n, thr, n1=5, n2=25):
    """cross-check of `value` through the reference's own entry point: TRS2_wrp (the whole solver: setup, loop, final
    transformation) with max_iterations n1 and n2, monitor off; (t(n2) - t(n1)) / (n2 - n1) is the time of one loop
    iteration as BASELINE.md section 2 measures it for the reference."""
    ISQ = nt.Matrix_ps(n)
    ISQ.FillIdentity()
    ts = {}
    for iters in (n1, n1, n2):      # the first call warms the allocator
        p = nt.SolverParameters()
        p.SetConvergeDiff(1e-30)
        p.SetThreshold(thr)
        p.SetMaxIterations(iters)
        p.SetMonitorConvergence(False)
        K = nt.Matrix_ps(n)
        nt.synchronize()
        t0 = time.perf_counter()
        nt.DensityMatrixSolvers.TRS2(H, ISQ, n / 2.0, K, p)
        nt.synchronize()
        ts[iters] = time.perf_counter() - t0
        tr = nt.solver_trace()
        del K
    per = (ts[n2] - ts[n1]) / (n2 - n1)
    out = {"iters_per_s": 1.0 / per, "ms_per_iter": 1e3 * per,
           "method": "TRS2_wrp with max_iterations %d and %d (monitor off): (t(%d) - t(%d)) / %d" % (n1, n2, n2, n1, n2 - n1)}
    # the solver's own clock around its loop (setup, redistribution of the operands and the final transformation outside):
    # what the differenced whole-solve times above also contain is whatever of a solve's fixed cost GROWS with the iterate --
    # on several ranks, the result of a solve in a recovered order carried back to the caller's labels
    if tr.get("iterations", 0) > 0 and tr.get("loop_ms", 0.0) > 0.0:
        out["loop_ms_per_iter"] = tr["loop_ms"] / tr["iterations"]
        out["loop_iters_per_s"] = 1e3 * tr["iterations"] / tr["loop_ms"]
        out["setup_ms"] = tr["setup_ms"]
    return out


def sources_sha16():
    """fingerprint of the kernel sources a committed PMC traffic figure belongs to"""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "ntpoly_amd", "csrc")
    # every device source and every header / generated loop they include: a figure belongs to ALL of them
    for f in sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".hpp", ".inc"))):
        h.update(f.encode())
        with open(os.path.join(csrc, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def run_config3(nt, args, rank, world):
    """BASELINE configs[3]: ONE distributed product C = A * A of the banded operand at N = 1 048 576, halfband 100 (201 per
    row; --permute SEED: the same operand under the seeded random relabelling the reference's load balancer applies,
    LoadBalancerModule.F90:14-52), through MatrixMultiply_ps_wrp exactly as distributed_algebra_includes/MatrixMultiply.f90
    :92-267 is entered by a caller.  A step = one multiply (exchange + local product + prune); value = output entries per
    second over all ranks; the roofline object is rank 0's numeric kernel."""
    from gen import banded_triplets, permuted_banded_triplets
    n = args.n if args.n is not None else 1048576
    h, thr = args.halfband, args.threshold
    nt.ConstructGlobalProcessGrid(1, world, 1)
    nt.set_option("time_kernels", 1)
    lib_default = "fma" if nt.get_option("spgemm_fma") == 1 else "unfused"
    arithmetic = args.arithmetic or lib_default
    nt.set_option("spgemm_fma", 1 if arithmetic == "fma" else 0)
    A = nt.Matrix_ps(n)
    c0, c1 = A.local_columns()
    col, row, val = banded_triplets(n, h, c0=c0, c1=c1) if args.permute is None else permuted_banded_triplets(n, h, args.permute, c0=c0, c1=c1)
    tl = nt.TripletList_r()
    tl.set_arrays(col, row, val)
    A.FillFromTripletList(tl, prepartitioned=True)
    del col, row, val, tl
    nnz_a = A.GetSize()
    Cm = nt.Matrix_ps(n)
    pool = nt.PMatrixMemoryPool(A)

    def fence():
        nt.synchronize()
        if world > 1:
            nt.barrier()
            nt.synchronize()

    # The timed region runs with the per-product statistics OFF (they cost a counting pass and a read-back of their own
    # inside MatrixMultiply); the roofline object comes from one more, untimed, block of the same K multiplies with the
    # HIP-event timers and the statistics on.
    blocks = []
    for blk in range(max(1, args.blocks) + 1):
        stats_block = blk == max(1, args.blocks)
        nt.set_option("time_kernels", 1 if stats_block else 0)
        for _ in range(max(1, args.warmup)):
            Cm.Gemm(A, A, pool, 1.0, 0.0, thr)
        nt.reset_spgemm_accum()
        m0 = nt.malloc_stats()
        h0 = nt.exchange_stats()[2]
        fence()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            Cm.Gemm(A, A, pool, 1.0, 0.0, thr)
        fence()
        elapsed = time.perf_counter() - t0
        if world > 1:
            elapsed = nt.allreduce_max(elapsed)
        rec = dict(elapsed=elapsed, acc=nt.spgemm_accum(), st=nt.last_spgemm_stats(), gs=nt.last_grouped_stats(), bs=nt.last_block_stats(),
                   m0=m0, m1=nt.malloc_stats(), syncs=nt.exchange_stats()[2] - h0)
        if stats_block:
            stats = rec
        else:
            blocks.append(rec)
            if args.dump_outputs is not None and blk + 1 == max(1, args.blocks):
                dump_outputs(args.dump_outputs, Cm, n, {})     # the last timed product (before the statistics block)
    nnz_c = Cm.GetSize()     # (collective; whole matrix)
    order = sorted(range(len(blocks)), key=lambda k: blocks[k]["elapsed"])
    med = blocks[order[len(order) // 2]]
    if rank != 0:
        return None
    elapsed, acc, st, gs, bs = med["elapsed"], stats["acc"], stats["st"], stats["gs"], stats["bs"]
    calls = max(1, acc["calls"])
    ms_numeric = max(acc["ms_numeric"], 1e-9)
    achieved = acc["alg_bytes"] / (ms_numeric * 1e-3) / 1e9
    tfl = 2.0 * acc["products"] / (ms_numeric * 1e-3) / 1e12
    kernel = ("k_spgemm_tile" if arithmetic == "fma" else "k_spgemm_slab") if st.get("slab") else \
        "k_bs_numeric (block path)" if bs.get("used") else "k_spgemm_ghash (grouped LDS hash)" if gs.get("used") else "k_spgemm_pair3 / k_spgemm_hash"
    line = {
        "metric": "SpGEMM nnz-out/s, BASELINE configs[3]: one A*A, N=%d ~%d nnz/row" % (n, 2 * h + 1),
        "value": nnz_c * args.steps / elapsed, "unit": "nnz-out/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": "one distributed product A*A (BASELINE configs[3]): banded A N=%d halfband=%d%s, threshold=%g, 1-D column panels on %d rank(s)" % (
                       n, h, "" if args.permute is None else " under a random symmetric relabelling (seed %d)%s" % (
                           args.permute, ", taken as it stands (no band recovery, no block order: the LDS-hash SpGEMM)" if args.random is not None else ""), thr, world),
                   "arithmetic": arithmetic, "arithmetic_default": lib_default, "blocks_ms": [1e3 * b["elapsed"] for b in blocks],
                   "n": n, "halfband": h, "threshold": thr, "permute_seed": args.permute, "nnz_A": int(nnz_a), "nnz_C": int(nnz_c),
                   "host_syncs_per_step": med["syncs"] / float(args.steps),
                   "ms_per_step_with_statistics_on": 1e3 * stats["elapsed"] / args.steps,
                   "hipMalloc_in_timed_region": {"calls": med["m1"][0] - med["m0"][0], "ms": med["m1"][1] - med["m0"][1]}},
        "spgemm_products_per_s": world * acc["products"] / (ms_numeric * 1e-3),
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                     "kernel": kernel + " (SpGEMM numeric phase, rank 0's panel)", "alg_bytes_per_launch": acc["alg_bytes"] / calls,
                     "ms_per_launch": ms_numeric / calls,
                     "note": "rank-0 panel; algorithmic bytes = 12*(nnzA+nnzB+nnzC)+4*(colsA+colsB+colsC+3) of the local product"},
        "roofline_compute": {"bound": "fp64 matrix cores" if arithmetic == "fma" else "fp64 vector ALU (unfused mul+add)", "achieved": tfl,
                             "peak": 78.6 if arithmetic == "fma" else 39.3, "unit": "TFLOP/s", "frac": tfl / (78.6 if arithmetic == "fma" else 39.3)},
    }
    if bs.get("used"):
        line["block_path"] = bs
    if gs.get("used"):
        line["grouped_hash"] = gs
    return line


def transport_note(world):
    """how the ranks of this run talk to each other (config.transport)"""
    if world <= 1:
        return "none (one rank)"
    ndev = int(os.environ.get("NTPOLY_AMD_BENCH_DEVICES", "0"))
    if os.environ.get("NTPOLY_AMD_COMM", "").startswith("shm:"):
        return ("shared-memory TEST transport through host memory, %d ranks sharing %s GPU(s): a functional run of the "
                "distributed path, NOT a scaling measurement" % (world, ndev if ndev else "the box's"))
    return "RCCL over xGMI, one rank per GPU"


def probe_device_count():
    """number of GPUs visible, asked of a CHILD process: the parent of a self-launched multi-rank run never touches the GPU
    (a process that has initialised HIP must neither fork workers that use the GPU nor be replaced by another program)"""
    import subprocess
    r = subprocess.run([sys.executable, "-c",
                        "import sys; sys.path.insert(0, %r); import ntpoly_amd; print(int(ntpoly_amd.lib.ntpoly_amd_device_count()))" % ROOT],
                       stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    try:
        return int(r.stdout.strip().splitlines()[-1])
    except (ValueError, IndexError):
        return 0


def launch_ranks(world):
    """`python bench.py --gpus N` without a launcher: start N fresh child processes of this very command, one rank each
    (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT as torch.distributed.run would set them), relay rank 0's
    JSON line and exit with the first non-zero status of a child.  With fewer GPUs than ranks (a one-GPU box) the ranks
    share the devices round-robin and talk over the engine's shared-memory TEST transport instead of RCCL
    (NTPOLY_AMD_COMM=shm:<name>, csrc/comm.cpp): every line of the distributed path runs, the number is a functional
    check and says so in `config.transport`."""
    import socket
    import subprocess
    forced = os.environ.get("NTPOLY_AMD_COMM", "")
    ndev = probe_device_count()
    if ndev < 1:
        raise SystemExit("bench.py: no GPU visible (the product has no CPU path)")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    name = None
    env0 = dict(os.environ, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                NTPOLY_AMD_BENCH_DEVICES=str(ndev))
    if forced.startswith("shm:") or ndev < world:
        name = forced[4:] if forced.startswith("shm:") and len(forced) > 4 else "bench_%d_%d" % (os.getpid(), port)
        env0["NTPOLY_AMD_COMM"] = "shm:" + name
    else:
        # RCCL: rank 0 hands the unique id over through a file named here (host.init_comm_from_env)
        env0["NTPOLY_AMD_RDV"] = "/tmp/ntpoly_amd_rdv_bench_%d_%d" % (os.getpid(), port)
        env0["NTPOLY_AMD_RDV_NONCE"] = "%d:%d" % (os.getpid(), port)
    procs = []
    try:
        for r in range(world):
            env = dict(env0, RANK=str(r), LOCAL_RANK=str(r % ndev))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=(None if r == 0 else subprocess.DEVNULL)))
        rc = 0
        pending = list(procs)
        while pending:
            for p in list(pending):
                st = p.poll()
                if st is None:
                    continue
                pending.remove(p)
                if st != 0 and rc == 0:
                    rc = st if st > 0 else 1
                    for q in pending:      # a rank died: its peers would wait for it for ever
                        q.terminate()
            time.sleep(0.05)
        return rc
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        if name is not None:
            try:
                os.unlink("/dev/shm/ntpoly_amd_" + name)
            except OSError:
                pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--halfband", type=int, default=100)
    ap.add_argument("--threshold", type=float, default=1e-8)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run what it does not need: the CPU baseline, the TRS2_wrp-differenced "
                         "cross-check of the value and, for a relabelled or 3-D operand on several ranks, the solver path's rate")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-label-order", action="store_true",
                    help="with --permute: do not look for a band hidden under the labels (option label_order = 0): the "
                         "relabelled operand runs on the grouped LDS-hash SpGEMM as it stands")
    ap.add_argument("--no-wrp-check", action="store_true",
                    help="with --full: skip the TRS2_wrp-differenced cross-check of the value (on one rank)")
    ap.add_argument("--permute", type=int, default=None, metavar="SEED",
                    help="run on P^T H P under a seeded random relabelling (SURVEY 8(d): the load-balanced / "
                         "unstructured operand; the SpGEMM leaves the run-based kernels for the LDS hash path)")
    ap.add_argument("--random", type=int, default=None, metavar="SEED",
                    help="the unstructured workload: P^T H P under a seeded random relabelling taken AS IT STANDS (options label_order = 0, "
                         "block_path = 0, band_scope = 0: no band recovery, no block order) -- the shape of the reference's own harness "
                         "(UnitTests/bench.f90:58-76: a decaying band, randomly permuted, multiplied) on the north star's named kernel, "
                         "the grouped LDS-hash SpGEMM k_spgemm_ghash; with --config 3 one product, otherwise TRS2 iterations")
    ap.add_argument("--lattice", type=int, default=None, metavar="L",
                    help="run on the Hamiltonian of an L x L x L lattice (tests/gen.py lattice_triplets: 203 entries per row, "
                         "no band any relabelling could recover; N = L^3, e.g. 64 -> 262 144): the operand the north star's "
                         "LDS-hash SpGEMM exists for")
    ap.add_argument("--arithmetic", choices=("fma", "unfused"), default=None,
                    help="fma: every product entry is the chain of fma() over ascending k (one rounding per product) that "
                         "the reference computes when built with FP contraction -- run on the FP64 matrix cores "
                         "(v_mfma_f64_16x16x4_f64, option spgemm_fma = 1); unfused: separate multiply and add, the "
                         "reference's default x86-64 build bit for bit (v_mul_f64 + v_add_f64 register-slab kernel)")
    ap.add_argument("--blocks", type=int, default=5,
                    help="the timed region (warm-up + K steps from X0) is repeated this many times; the MEDIAN block is reported")
    ap.add_argument("--tile-rows", type=int, default=None, help="experiments: option tile_rows (1, 2, 4)")
    ap.add_argument("--tile-waves", type=int, default=None, help="experiments: option tile_waves (4, 8)")
    ap.add_argument("--set", action="append", default=[], metavar="OPTION=VALUE", help="experiments: any engine option (ntpoly_amd_set_option), e.g. tile2=0")
    ap.add_argument("--config", type=int, default=2, choices=(2, 3),
                    help="2: the headline (TRS2 iterations at BASELINE configs[2]); 3: BASELINE configs[3], ONE distributed product "
                         "A*A at N = 1 048 576, halfband 100 (with --permute SEED: under the load balancer's random relabelling), a "
                         "step = one MatrixMultiply_ps_wrp, value = nnz-out/s over all ranks")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float64; one GPU)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    if args.dump_outputs is not None and args.gpus != 1:
        ap.error("--dump-outputs needs --gpus 1")

    launched = int(os.environ.get("WORLD_SIZE", "1")) > 1 and "RANK" in os.environ
    if args.gpus > 1 and not launched:
        # no launcher around us: be the launcher (before anything touches the GPU in this process)
        sys.exit(launch_ranks(args.gpus))

    import ntpoly_amd as nt
    from gen import banded_triplets, permuted_banded_triplets
    # one process per GPU (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_PORT from the launcher); the engine owns its RCCL
    # communicator and torch is not imported: its wheel bundles a second HIP runtime, and two runtimes in one process
    # corrupt the heap at exit
    rank, world = nt.init_comm_from_env()
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE is %d" % (args.gpus, world))

    # experiment switches first: they apply to every workload (--config 3 included)
    if args.random is not None:
        if args.permute is not None or args.lattice is not None:
            raise SystemExit("--random SEED is a workload of its own (not with --permute / --lattice)")
        args.permute = args.random
        for k in ("label_order", "block_path", "band_scope"):
            nt.set_option(k, 0)
    if args.tile_rows is not None:
        nt.set_option("tile_rows", args.tile_rows)
    if args.tile_waves is not None:
        nt.set_option("tile_waves", args.tile_waves)
    if args.no_label_order:
        nt.set_option("label_order", 0)
    for kv in args.set:
        k, v = kv.split("=")
        nt.set_option(k, int(v))

    if args.config == 3:
        line = run_config3(nt, args, rank, world)
        if rank == 0:
            line["config"]["transport"] = transport_note(world)
            print(json.dumps(line), flush=True)
        if world > 1:
            nt.barrier()
        return

    n, h, thr = (args.n if args.n is not None else 262144), args.halfband, args.threshold
    if args.lattice is not None:
        n = args.lattice ** 3
    nt.ConstructGlobalProcessGrid(1, world, 1)  # column panels: one per GPU
    nt.set_option("time_kernels", 1)
    # the arithmetic a drop-in caller gets without asking (the library's default, or NTPOLY_AMD_ARITHMETIC from the
    # environment) is what this line times unless --arithmetic says otherwise
    lib_default = "fma" if nt.get_option("spgemm_fma") == 1 else "unfused"
    if args.arithmetic is None:
        args.arithmetic = lib_default
    nt.set_option("spgemm_fma", 1 if args.arithmetic == "fma" else 0)
    # ---- setup (untimed): Hamiltonian panel, X0 = (e_max*I - H)/(e_max - e_min)  (:344-371)
    H = nt.Matrix_ps(n)
    c0, c1 = H.local_columns()
    if args.lattice is not None:
        from gen import lattice_triplets
        col, row, val = lattice_triplets(args.lattice, c0=c0, c1=c1)
    elif args.permute is None:
        col, row, val = banded_triplets(n, h, c0=c0, c1=c1)
    else:
        col, row, val = permuted_banded_triplets(n, h, args.permute, c0=c0, c1=c1)
    tl = nt.TripletList_r()
    tl.set_arrays(col, row, val)
    H.FillFromTripletList(tl, prepartitioned=True)
    del col, row, val, tl
    nnz_h = H.GetSize()
    e_min, e_max = nt.EigenBounds.GershgorinBounds(H)
    Ident = nt.Matrix_ps(n)
    Ident.FillIdentity()
    pool = nt.PMatrixMemoryPool(H)
    trace_target = n / 2.0

    def fence():
        # device synchronise (stream + hipDeviceSynchronize inside the engine's own HIP runtime: the same
        # thing torch.cuda.synchronize() does for torch's), then a barrier over all ranks
        nt.synchronize()
        if world > 1:
            nt.barrier()
            nt.synchronize()

    # The timed region is short (20 steps = 34 ms on the headline), so ONE block of it carries +-3 % of noise (VERDICT r3
    # weak 7).  The same region -- X0 from H, W untimed warm-up steps, barrier + device synchronise, exactly K timed
    # steps, barrier + device synchronise, max over ranks -- is therefore run `--blocks` times (default 5), each time
    # from scratch, and the line reports the MEDIAN block (its time, its kernel timers, its counters); `steps` stays K.
    def x0():
        X = nt.Matrix_ps(H)
        X.Scale(-1.0)
        X.Increment(Ident, e_max, 0.0)
        X.Scale(1.0 / (e_max - e_min))
        return X

    blocks = []
    for blk in range(max(1, args.blocks)):
        X = x0()
        X2 = nt.Matrix_ps(n)
        energy, tr_x = 0.0, None
        for g in range(args.warmup):
            if g and g % TRS2_WINDOW == 0:
                X, tr_x = x0(), None
            _, energy, tr_x = trs2_step(nt, X, X2, H, pool, trace_target, thr, tr_x)
        nt.reset_spgemm_accum()
        m0 = nt.malloc_stats()
        fz0 = nt.fusion_counts()
        m_restart = [0, 0.0]    # hipMalloc calls / ms of the restarts (outside the clock)
        elapsed = 0.0
        fence()
        t0 = time.perf_counter()
        for g in range(args.warmup, args.warmup + args.steps):
            if g and g % TRS2_WINDOW == 0:
                # restart from X0 (TRS2_WINDOW): the clock stops for it
                fence()
                elapsed += time.perf_counter() - t0
                r0 = nt.malloc_stats()
                X, tr_x = x0(), None
                r1 = nt.malloc_stats()
                m_restart = [m_restart[0] + r1[0] - r0[0], m_restart[1] + r1[1] - r0[1]]
                fence()
                t0 = time.perf_counter()
            sigma, energy, tr_x = trs2_step(nt, X, X2, H, pool, trace_target, thr, tr_x)
        fence()
        elapsed += time.perf_counter() - t0
        if world > 1:
            elapsed = nt.allreduce_max(elapsed)
        m1 = nt.malloc_stats()
        m1 = (m1[0] - m_restart[0], m1[1] - m_restart[1])
        fz1 = nt.fusion_counts()
        blocks.append(dict(elapsed=elapsed, energy=energy, m0=m0, m1=m1, fused={k: fz1[k] - fz0[k] for k in fz1}, acc=nt.spgemm_accum(),
                           st=nt.last_spgemm_stats(), gs=nt.last_grouped_stats(), bs=nt.last_block_stats(), nnz_x=X.GetSize()))
        if blk + 1 < max(1, args.blocks):
            del X, X2
    if args.dump_outputs is not None:
        # the last timed step of the last block: the new iterate X and the scalars the step returned (deterministic: the
        # same iteration of the same window for the same arguments)
        dump_outputs(args.dump_outputs, X, n, {"sigma": sigma, "energy": energy, "trace": tr_x})
    order = sorted(range(len(blocks)), key=lambda k: blocks[k]["elapsed"])
    med = blocks[order[len(order) // 2]]
    elapsed, energy, m0, m1, fused, acc, st, gs, bs, nnz_x = (med[k] for k in ("elapsed", "energy", "m0", "m1", "fused", "acc", "st", "gs", "bs", "nnz_x"))
    block_ms = [1e3 * b["elapsed"] for b in blocks]

    if rank == 0:
        # HBM traffic of the dominant kernel comes from PMC passes (FETCH_SIZE / WRITE_SIZE, separate rocprofv3 runs of
        # this same command; they cannot be collected from inside the process): profiles/<tag>_pmc_traffic*.json holds
        # the corrected bytes per launch together with a fingerprint of the kernel sources it was measured on -- a
        # figure measured on other sources is not reported (null)
        traffic, traffic_src = None, None
        tname = ("r06_pmc_traffic%s.json" if args.arithmetic == "fma" else "r06_pmc_traffic_unfused%s.json") % (
            "_lattice" if args.lattice is not None else "" if args.permute is None else "_random" if args.random is not None else "_permute")
        try:
            with open(os.path.join(ROOT, "profiles", tname)) as f:
                tj = json.load(f)
            if (n, thr, world) == (262144, 1e-8, 1) and (h == 100 or args.lattice is not None) and tj.get("sources_sha16") == sources_sha16() and \
                    args.tile_rows is None and args.tile_waves is None:
                traffic, traffic_src = float(tj["hbm_bytes_per_launch"]), "profiles/" + tname
        except Exception:
            traffic = None
        iters_per_s = args.steps / elapsed
        if args.warmup + args.steps > TRS2_WINDOW:
            timed_note = " (iterations counted from X0, restarted from X0 outside the clock every %d)" % TRS2_WINDOW
        else:
            timed_note = ""
        # nnz-out/s of the SpGEMM alone: local output entries / local numeric+symbolic time; whole job
        # = sum over ranks (ranks hold equal panels of a homogeneous band)
        ms_spgemm = max(acc["ms_total"], 1e-9)
        ms_numeric = max(acc["ms_numeric"], 1e-9)
        calls = max(1, acc["calls"])
        achieved = acc["alg_bytes"] / (ms_numeric * 1e-3) / 1e9  # GB/s, algorithmic bytes / kernel time
        line = {
            "metric": "TRS2 iters/s + SpGEMM nnz-out/s, N=262k ~200 nnz/row, 1/2/4/8 GPU",
            "value": iters_per_s,
            "unit": "iters/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": ("TRS2 purification on a 3-D lattice Hamiltonian (no band structure): %d^3 = %d sites, couplings within "
                                    "distance sqrt(13) (203 nnz/row), threshold=%g, ISQ=I, trace=N/2; timed iterations %d..%d%s" % (
                                        args.lattice, n, thr, args.warmup + 1, args.warmup + args.steps, timed_note))
                       if args.lattice is not None else
                       "TRS2 purification (BASELINE configs[2]): banded H N=%d halfband=%d (%d nnz/row)%s, "
                       "threshold=%g, ISQ=I, trace=N/2; timed iterations %d..%d%s" % (
                           n, h, 2 * h + 1,
                           "" if args.permute is None else " under a random symmetric relabelling (seed %d)%s" % (
                               args.permute, ", taken as it stands (no band recovery, no block order: the LDS-hash SpGEMM)" if args.random is not None else ""),
                           thr, args.warmup + 1, args.warmup + args.steps, timed_note),
                       "lattice": args.lattice, "trs2_window": TRS2_WINDOW,
                       "arithmetic": ("fma: every product entry is the chain of fma() over ascending k (one rounding per product), "
                                      "the reference's FP-contracted build bit for bit (tests/golden/ps_gemm_fma.npz); run-like "
                                      "operands on the FP64 matrix cores (v_mfma_f64_16x16x4_f64, spgemm_tile.hip), operands without runs "
                                      "as 16x16 tiles of a clustered index order on the same instruction (spgemm_block.hip)"
                                      if args.arithmetic == "fma" else
                                      "unfused: separate v_mul_f64 + v_add_f64, the reference's default x86-64 build bit for bit"),
                       "arithmetic_default": lib_default,   # what an unmodified caller of the C ABI runs with
                       "blocks_ms": block_ms,               # every repetition of the timed region; `value` is the median block
                       "n": n, "halfband": h, "threshold": thr, "nnz_H": int(nnz_h), "nnz_X_end": int(nnz_x),
                       "nnz_product_last": int(st.get("nnz_c", -1)), "energy_end": energy,
                       "permute_seed": args.permute, "random": args.random is not None,
                       "decomposition": "1-D column panels, %d rank(s)" % world,
                       "transport": transport_note(world),
                       "hipMalloc_in_timed_region": {"calls": m1[0] - m0[0], "ms": m1[1] - m0[1]}},
            "spgemm_nnz_out_per_s": world * acc["nnz_c"] / (ms_spgemm * 1e-3),
            "spgemm_products_per_s": world * acc["products"] / (ms_numeric * 1e-3),
            "spgemm_ms_per_call": ms_spgemm / calls,
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         "kernel": (("k_spgemm_tile" if args.arithmetic == "fma" else "k_spgemm_slab") if st.get("slab") else
                                    "k_bs_numeric (block path: 16x16 tiles of a clustered index order on v_mfma_f64_16x16x4_f64, spgemm_block.hip)" if bs.get("used") else
                                    "k_spgemm_ghash (grouped LDS hash)" if gs.get("used")
                                    else "k_spgemm_pair3 / k_spgemm_hash") +
                                   (" (SpGEMM numeric phase with the TRS2 update, energy and trace in its epilogue)"
                                    if fused["square"] + fused["update"] > 0 else " (SpGEMM numeric phase)"),
                         "alg_bytes_per_launch": acc["alg_bytes"] / calls, "ms_per_launch": ms_numeric / calls,
                         "traffic_source": traffic_src,
                         "note": "rank-0 panel; algorithmic bytes = 12*(nnzA+nnzB+nnzC)+4*(colsA+colsB+colsC+3); traffic = bytes "
                                 "per launch from the committed PMC passes of this command (null when the kernel sources "
                                 "have changed since)"},
        }
        # compute-side view: 2 flops per product against the FP64 peak of the arithmetic mode -- 78.6 TFLOP/s for fused
        # multiply-adds (vector FMA and the f64 matrix instruction have the same rate on gfx950), 39.3 for SEPARATE
        # multiply and add instructions
        tfl = 2.0 * acc["products"] / (ms_numeric * 1e-3) / 1e12
        if args.arithmetic == "fma":
            line["roofline_compute"] = {"bound": "fp64 matrix cores (v_mfma_f64_16x16x4_f64, one FMA per product)", "achieved": tfl,
                                        "peak": 78.6, "unit": "TFLOP/s", "frac": tfl / 78.6}
        else:
            line["roofline_compute"] = {"bound": "fp64 vector ALU (unfused mul+add)", "achieved": tfl, "peak": 39.3,
                                        "unit": "TFLOP/s", "frac": tfl / 39.3}
        # timed steps computed inside the SpGEMM kernel (X*X; 2X - X*X) and fused steps that had to be repeated unfused
        line["fused_steps"] = fused
        if gs.get("used"):
            line["grouped_hash"] = gs
        if bs.get("used"):
            # block path: of the 16 x 16 x 16 tile products issued (4 matrix instructions each) only the products of two
            # stored entries are the reference's multiply-adds -- the rest multiplies zeros of the tiles
            issued = 4096.0 * bs["tile_products"]
            line["block_path"] = dict(bs, useful_fraction_last_product=(st["products"] / issued if issued else None),
                                      issued_tflops_last_product=(2.0 * issued / (st["ms_numeric"] * 1e-3) / 1e12 if st.get("ms_numeric") else None))
    check = None
    reordered = args.permute is not None or args.lattice is not None   # (operands the solver redistributes on several ranks)
    if args.full and (not args.no_wrp_check or (world > 1 and reordered)):
        del X, X2
        check = trs2_wrp_check(nt, H, n, thr)       # (collective: every rank takes part)
    if rank == 0 and world > 1 and reordered and check:
        # A relabelled or 3-D operand on several ranks: the SOLVER recovers the band (or takes the pattern's block order) once per
        # solve and redistributes the operands (csrc/band_scope.cpp); the step API above works on the caller's distribution and
        # cannot.  `value` stays what it is on every other line -- the rate of the step API -- and the rate of the reference's
        # own entry point, TRS2_wrp differenced over two iteration counts, is reported beside it.
        # (... and, beside that, the solver's own clock around its loop: the differenced whole-solve times contain the growth of
        # the per-solve redistribution with the iterate's entry count -- through the host-memory test transport that dominates)
        line["solver_path_iters_per_s"] = check["iters_per_s"]
        line["config"]["solver_path_measured_through"] = check["method"]
        if "loop_iters_per_s" in check:
            line["solver_loop_iters_per_s"] = check["loop_iters_per_s"]
    if rank == 0:
        if check:
            line["trs2_wrp_check"] = check
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(n, h, thr, args.warmup, args.steps, args.permute, fma=args.arithmetic == "fma",
                                                lattice=args.lattice)
        print(json.dumps(line), flush=True)
    if world > 1:
        nt.barrier()


if __name__ == "__main__":
    main()
