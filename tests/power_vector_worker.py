#!/usr/bin/env python3
"""Child process of tests/test_gpu_power_vector.py (option power_vector).

    python tests/power_vector_worker.py memory
        a fresh process: after a warm-up PowerBounds on a 64 x 64 identity, in-use + cached device bytes before and after
        PowerBounds with 60 fixed steps on a band of N = 65 536, h = 16; one JSON line.

    python tests/power_vector_worker.py ranks <out-prefix>
        one rank of the several-ranks test: RANK / WORLD_SIZE / NTPOLY_AMD_COMM come from the environment, the ranks share ONE GPU
        and exchange through the shared-memory test transport.  PowerBounds with ten fixed steps on the solver test's operands
        and on n = 5, in both arithmetic modes; the bound (as hex, for a bitwise comparison) and the counters per case, as JSON.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fixed_steps(nt, steps, thr):
    p = nt.SolverParameters()
    p.SetThreshold(thr)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(steps)
    p.SetMonitorConvergence(False)
    return p


def counted(nt, A, p):
    before = nt.power_vector_counts()
    bound = nt.EigenBounds.PowerBounds(A, p)
    after = nt.power_vector_counts()
    return bound, [after[k] - before[k] for k in ("solves", "steps", "refused")]


def memory():
    import ntpoly_amd as nt
    from gen import banded_triplets
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    nt.set_option("power_vector", 1)
    I = nt.Matrix_ps(64)
    I.FillIdentity()
    nt.EigenBounds.PowerBounds(I, fixed_steps(nt, 3, 0.0))
    n, h = 65536, 16
    col, row, val = banded_triplets(n, h)
    A = nt.Matrix_ps.from_triplets(n, col, row, val)
    before = sum(nt.memory())
    bound, counts = counted(nt, A, fixed_steps(nt, 60, 1e-8))
    after = sum(nt.memory())
    print(json.dumps(dict(n=n, nnz=int(len(val)), before=before, after=after, bound=bound, counts=counts)))


def panel(nt, n, triplets_of):
    """the matrix from this rank's own columns"""
    A = nt.Matrix_ps(n)
    c0, c1 = A.local_columns()
    col, row, val = triplets_of(c0, c1)
    t = nt.TripletList_c() if np.iscomplexobj(val) else nt.TripletList_r()
    t.set_arrays(col, row, val)
    A.FillFromTripletList(t, prepartitioned=True)
    return A, c1 - c0


def ranks(out):
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    import ntpoly_amd as nt
    from gen import banded_triplets
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    nt.set_option("power_vector", 1)

    def nonsym(n, hl, hu):
        def f(c0, c1):
            col, row, val = banded_triplets(n, max(hl, hu), shift=2.5, c0=c0, c1=c1)
            d = row.astype(np.int64) - col
            keep = (d >= -hu) & (d <= hl)
            return col[keep], row[keep], np.where(d < 0, 0.5 * val, val)[keep]
        return f

    cases = {
        "sym1037": (1037, lambda c0, c1: banded_triplets(1037, 24, c0=c0, c1=c1)),
        "nonsym257": (257, nonsym(257, 24, 9)),
        "hermitian1037": (1037, lambda c0, c1: banded_triplets(1037, 24, complex_=True, c0=c0, c1=c1)),
        "n5": (5, nonsym(5, 2, 1)),
    }
    res = {}
    for name, (n, f) in cases.items():
        A, width = panel(nt, n, f)
        if name == "n5":
            res["n5_width"] = int(width)
        for arith, mode in (("fma", 1), ("unfused", 0)):
            nt.set_option("spgemm_fma", mode)
            bound, counts = counted(nt, A, fixed_steps(nt, 10, 1e-8))
            res["%s_%s" % (name, arith)] = dict(bound_hex=float(bound).hex(), counts=counts)
    with open(out + ".%d.json" % rank, "w") as f:
        json.dump(res, f)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    if sys.argv[1] == "memory":
        memory()
    else:
        ranks(sys.argv[2])
