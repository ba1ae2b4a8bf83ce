#!/usr/bin/env python3
"""One rank of the scalar-reduction test across ranks (tests/test_gpu_scalar_forms.py): RANK / WORLD_SIZE / NTPOLY_AMD_COMM come
from the environment as for tests/multirank_vocab_worker.py, the ranks are processes sharing ONE GPU and exchange through the
shared-memory test transport, the grid is 1 x world x 1.  The mixed case of tests/scalar_reference.py in both families, real and
complex, as compressed column panels: Dot of every pair, Trace, Norm and GershgorinBounds of every operand; the same three of
the banded panel operands, whose extreme column and missing diagonal lie in a panel with col_offset != 0.  Then the slab-form
panels of a solver session (option panel_sessions, FMA arithmetic -- the one-call sessions of the C ABI do not open across ranks,
so the vocabulary calls above always see compressed columns there): the first step of the order-2 inverse square root takes the
Gershgorin bounds of its slab-form panel of A I, with col_offset != 0 on every rank but the first, and records
1 / max(|lo|, |hi|).  Results, keys "<case>.<scalar>.<operands>", go to <out>.<rank>.npz.

    python tests/scalar_forms_worker.py <out-prefix>
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out = sys.argv[1]
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    import ntpoly_amd as nt
    import scalar_reference as R
    nt.init_comm(nt.get_unique_id(), rank, world)
    nt.ConstructGlobalProcessGrid(1, world, 1)
    res = {}

    def fill(n, t):
        """this rank's own columns of the operand, prepartitioned"""
        M = nt.Matrix_ps(n)
        c0, c1 = M.local_columns()
        tl = nt.TripletList_c() if np.iscomplexobj(t[2]) else nt.TripletList_r()
        tl.set_arrays(*R.split_for_rank(t, c0, c1))
        M.FillFromTripletList(tl, prepartitioned=True)
        return M

    for family in ("int", "real"):
        for cplx in (False, True):
            c = R.case("mixed", family, cplx)
            n, cid = c["n"], c["id"]
            M = {name: fill(n, t) for name, t in c["ops"].items()}
            for a, b in c["dots"]:
                re, im = C.c_double(), C.c_double()
                nt.lib.DotMatrix_psc_wrp(M[a].ih, M[b].ih, C.byref(re), C.byref(im))
                res["%s.dot.%s.%s" % (cid, a, b)] = np.array([re.value, im.value])
            for name in c["singles"]:
                res["%s.trace.%s" % (cid, name)] = np.array([M[name].Trace()])
                res["%s.norm.%s" % (cid, name)] = np.array([M[name].Norm()])
                res["%s.gershgorin.%s" % (cid, name)] = np.array(nt.EigenBounds.GershgorinBounds(M[name]))

    n = R.N_MIXED
    p = nt.SolverParameters()
    p.SetThreshold(0.0)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(1)
    for name, (t, ext, gone) in R.panel_operands(world).items():
        H = fill(n, t)
        res["panel.%s.compressed" % name] = np.array([H.Trace(), H.Norm()] + list(nt.EigenBounds.GershgorinBounds(H)))
        Out = nt.Matrix_ps(n)
        s0, p0 = nt.slab_algebra_counts(), nt.panel_product_counts()
        nt.SquareRootSolvers.with_order(H, Out, p, True, 2)
        s1, p1 = nt.slab_algebra_counts(), nt.panel_product_counts()
        res["panel.%s.lambda" % name] = np.array([nt.solver_trace()["sigma"][0]])
        res["panel.%s.counts" % name] = np.array([s1["products"] - s0["products"], s1["others"] - s0["others"], s1["refusals"] - s0["refusals"],
                                                  p1["slab"] - p0["slab"]])

    nt.barrier()
    np.savez(out + ".%d.npz" % rank, **res)
    nt.DestructGlobalProcessGrid()


if __name__ == "__main__":
    main()
