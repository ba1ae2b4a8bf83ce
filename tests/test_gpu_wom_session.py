"""GPU: WOM_GC / WOM_C in a slab session (option wom_session; solvers_extra.cpp solver_wom, csrc/wom_heun.hip).  1: the loop's
matrices stay in slab form between the products and the same vocabulary calls run in the same order; 2: the tail of a Heun trial
(RK2, err, err2) is one pass over the runs and the canonical step's two dots are one kernel, bit for bit what 1 computes.  Against
option 0 -- the loop on compressed columns, the code as it stood -- the session's norm and dots sum in another order, and they set
the step sizes: the comparison is held to what the solver's own threshold moves the result by, measured here on option 0.

A dense numpy simulation of the loop on this Hamiltonian (n = 512 and n = 2048; banded_triplets(n, 20), ISQ = I, threshold 1e-8,
step_thresh 1e-2, inv_temp 2) gives 10 trials, 8 accepted and 2 rejected, for both solvers, a half bandwidth of W of about 66, and
the err closest to 1.1 step_thresh 2.3 % away from it for WOM_GC and 1.7 % for WOM_C: rounding cannot flip a decision.  The
option-0 run is held to these counts, as a condition on the inputs."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from gen import banded_triplets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HALF, THR, INV_TEMP, STEP_THRESH = 2048, 20, 1e-8, 2.0, 1e-2
TRIALS, ACCEPTED = 10, 8
KEYS = ("solves", "heun_passes", "c_dot_passes", "refused")
NONE = dict.fromkeys(KEYS, 0)


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture(params=[1, 0], ids=["fma", "unfused"])
def fma(nt, request):
    nt.set_option("spgemm_fma", request.param)
    yield request.param
    nt.set_option("spgemm_fma", 0)
    nt.set_option("slab_algebra", 1)
    nt.set_option("wom_session", 0)


def srt(t):
    c, r, v = t
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def dense(t, n):
    c, r, v = t
    D = np.zeros((n, n), dtype=v.dtype)
    D[r - 1, c - 1] = v
    return D


def wom_solve(nt, H, n, kind, option, thr=THR):
    nt.set_option("wom_session", option)
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    p = nt.SolverParameters()
    p.SetThreshold(thr)
    K = nt.Matrix_ps(n)
    c0, s0 = nt.wom_session_counts(), nt.slab_algebra_counts()
    if kind == "gc":
        e = nt.FermiOperator.WOM_GC(H, I, K, 0.0, INV_TEMP, p)
    else:
        e = nt.FermiOperator.WOM_C(H, I, K, n / 2.0, INV_TEMP, p)
    c1, s1 = nt.wom_session_counts(), nt.slab_algebra_counts()
    tr = nt.solver_trace()
    nt.set_option("wom_session", 0)
    value = np.asarray(tr["value"]).copy()
    return dict(out=srt(K.triplets()), e=e, trials=tr["iterations"], accepted=int((value <= 1.1 * STEP_THRESH).sum()), value=value,
                sigma=np.asarray(tr["sigma"]).copy(), energy=np.asarray(tr["energy"]).copy(), nnz=np.asarray(tr["nnz"]).copy(),
                counts={k: c1[k] - c0[k] for k in c1}, refusals=s1["refusals"] - s0["refusals"])


def equal(x, y):
    return (x["trials"] == y["trials"] and same(x["out"], y["out"]) and x["e"] == y["e"] and
            all(np.array_equal(x[k], y[k]) for k in ("value", "sigma", "energy", "nnz")))


@pytest.fixture(scope="module")
def hamiltonian(nt):
    return nt.Matrix_ps.from_triplets(N, *banded_triplets(N, HALF))


@pytest.mark.parametrize("kind", ["gc", "c"])
def test_the_three_options(nt, fma, hamiltonian, kind):
    H = hamiltonian
    off = wom_solve(nt, H, N, kind, 0)
    fine = wom_solve(nt, H, N, kind, 0, THR / 10)
    one = wom_solve(nt, H, N, kind, 1)
    two = wom_solve(nt, H, N, kind, 2)
    print(kind, "option 0: trials", off["trials"], "accepted", off["accepted"], "err", off["value"].tolist(), "steps", off["sigma"].tolist())
    print(kind, "counts", off["counts"], one["counts"], two["counts"], "session refusals", off["refusals"], one["refusals"], two["refusals"])
    # a condition on the inputs: the counts of the dense simulation, and no err near the acceptance bound
    assert off["trials"] == TRIALS and off["accepted"] == ACCEPTED
    assert np.min(np.abs(off["value"] / (1.1 * STEP_THRESH) - 1.0)) > 0.01
    assert off["counts"] == NONE and fine["counts"] == NONE
    assert len(off["sigma"]) == TRIALS and np.all(off["nnz"] > N) and len(set(off["energy"].tolist())) == ACCEPTED
    # option 2 against option 1: bit for bit
    assert two["trials"] == one["trials"]
    for k in ("value", "sigma", "energy", "nnz"):
        assert np.array_equal(two[k], one[k]), k
    assert same(two["out"], one["out"]), "density triplets, bit for bit"
    assert two["e"] == one["e"]
    gradients = two["trials"] + two["accepted"]
    assert one["counts"] == dict(NONE, solves=1)
    assert two["counts"] == dict(solves=1, heun_passes=two["trials"], c_dot_passes=gradients if kind == "c" else 0, refused=0)
    assert two["refusals"] <= one["refusals"]
    # options 1 and 2 against option 0: what a rounding-level change of a step size moves, against what the threshold moves
    D0, Df = dense(off["out"], N), dense(fine["out"], N)
    bound_k, bound_e = float(np.max(np.abs(D0 - Df))), abs(off["e"] - fine["e"])
    for name, run in (("1", one), ("2", two)):
        dk, de = float(np.max(np.abs(dense(run["out"], N) - D0))), abs(run["e"] - off["e"])
        print(kind, "option", name, "max |K - K0|", dk, "bound", bound_k, "|E - E0|", de, "bound", bound_e)
        assert run["trials"] == off["trials"] and run["accepted"] == off["accepted"]
        assert dk <= bound_k
        assert de <= bound_e


def test_gates(nt, fma, hamiltonian):
    """the option at 0, slab_algebra = 0 and a complex Hamiltonian count nothing: the results of option 0"""
    H = hamiltonian
    want = wom_solve(nt, H, N, "gc", 0)
    again = wom_solve(nt, H, N, "gc", 0)
    assert want["counts"] == NONE == again["counts"] and equal(want, again)
    nt.set_option("slab_algebra", 0)
    a = wom_solve(nt, H, N, "gc", 2)
    b = wom_solve(nt, H, N, "c", 2)
    b0 = wom_solve(nt, H, N, "c", 0)
    nt.set_option("slab_algebra", 1)
    assert a["counts"] == NONE and equal(a, want)
    assert b["counts"] == NONE == b0["counts"] and equal(b, b0)
    nc, hc = 1024, 12
    Hc = nt.Matrix_ps.from_triplets(nc, *banded_triplets(nc, hc, complex_=True))
    c = wom_solve(nt, Hc, nc, "gc", 2)
    d = wom_solve(nt, Hc, nc, "gc", 0)
    assert c["counts"] == NONE == d["counts"] and equal(c, d)


def test_the_trace_is_the_solvers_own(nt, fma, hamiltonian):
    """solver_wom resets the record: after a WOM call it is not the previous solver's"""
    p = nt.SolverParameters()
    p.SetThreshold(THR)
    p.SetMaxIterations(3)
    I, K = nt.Matrix_ps(N), nt.Matrix_ps(N)
    I.FillIdentity()
    nt.DensityMatrixSolvers.TRS2(hamiltonian, I, N / 2.0, K, p)
    before = nt.solver_trace()
    assert 0 < before["iterations"] <= 3
    r = wom_solve(nt, hamiltonian, N, "gc", 0)
    assert r["trials"] == TRIALS and np.all(r["sigma"] > 0.0) and np.all(r["sigma"] <= 1.0)


# ------------------------------------------------------------------ two ranks
def run_world(world, tmp_path):
    out = str(tmp_path / ("wom%d" % world))
    name = "w%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name, NTPOLY_AMD_SHM_MB="64",
                   NTPOLY_AMD_SPGEMM_FMA="1")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "wom_session_worker.py"), out],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=300)
            logs.append(o)
            if p.returncode != 0:   # (the first failure ends the world: the other rank would wait for it in a collective)
                break
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        try:
            os.unlink("/dev/shm/ntpoly_amd_" + name)
        except OSError:
            pass
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d of %d failed:\n%s" % (r, world, logs[r][-3000:] if r < len(logs) else "(ended with the first failure)")
    return [dict(np.load(out + ".%d.npz" % r)) for r in range(world)]


def test_two_ranks_option_2_against_option_1(tmp_path):
    """WOM_GC and WOM_C of a real band, n = 2048, as column panels on two ranks sharing one GPU (shared-memory transport, FMA
    arithmetic), option 2 against option 1 in the same processes: the traces and the gathered density bit for bit (one reduction
    carries both norms, element by element what two carry), fused passes on both ranks"""
    two = run_world(2, tmp_path)
    for kind in ("gc", "c"):
        a, b = kind + "_1", kind + "_2"
        for r, p in enumerate(two):
            print("rank", r, kind, "trials", int(p["iters_" + b][0]), "counts", p["counts_" + a].tolist(), p["counts_" + b].tolist())
            trials = int(p["iters_" + b][0])
            assert trials == int(p["iters_" + a][0]) == TRIALS
            for k in ("value", "sigma", "energy", "nnz"):
                assert np.array_equal(p["%s_%s" % (k, a)], p["%s_%s" % (k, b)]), (kind, k)
            assert p["e_" + a][0] == p["e_" + b][0]
            assert p["counts_" + a].tolist() == [1, 0, 0, 0]
            accepted = int((p["value_" + b] <= 1.1 * STEP_THRESH).sum())
            assert p["counts_" + b].tolist() == [1, trials, trials + accepted if kind == "c" else 0, 0], (r, p["counts_" + b])
        for k in ("col", "row", "val"):
            assert np.array_equal(np.concatenate([p["%s_%s" % (k, a)] for p in two]), np.concatenate([p["%s_%s" % (k, b)] for p in two])), (kind, k)
        assert len(np.concatenate([p["val_" + b] for p in two])) > N
        assert np.array_equal(two[0]["value_" + b], two[1]["value_" + b])
