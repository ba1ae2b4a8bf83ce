"""GPU: the traces of CGSolver from column dot passes (option cg_dots; csrc/cg_dots.hip k_cg_dots / k_cg_trace, solvers_extra.cpp
solver_cg).

The premise: entry (j, j) of MatrixMultiply(U^H, V, threshold) is the chain over ascending k of conj(U(k, j)) V(k, j) in the
product's arithmetic, pruned as the product prunes, and MatrixTrace sums the real parts in a fixed order.  So (1) the diagonal and
the trace that cg_dots returns equal the diagonal of the product formed through the public calls (TransposeMatrix, MatrixMultiply)
and its MatrixTrace bit for bit -- real operands, both arithmetic modes; (2) complex operands with the option at 2 in FMA mode run
beside the complex tile kernel's tolerance mode and are compared by the rule of close() in tests/test_gpu_complex_tile.py (1e-13 of
the largest entry); in unfused mode and with the option at 1 the entry point declines them.  (3) CGSolver with the option at 1 is
CGSolver with the option at 0: X in pattern and bits, the logged iteration count, the counters; the `cg` and `pade` cases of
tests/golden/extras.npz through the new path; ComputeExponentialPade bit for bit.  (4) The complex solve with the option at 2
against a dense numpy restatement of the loop, no further from it than ten times the solve with the option at 0.  (5) Two and three
ranks over the shared-memory transport.

Thresholded case of (1) and (2): the threshold is the midpoint between two neighbouring moduli of the dense numpy diagonal, chosen
so that it drops three tenths of its non-zero entries (pick_threshold of tests/test_gpu_power_vector.py); the test asserts that
between a tenth and a half are dropped in the engine's result.  A diagonal with fewer than four non-zero entries (n = 1) has no
such threshold and runs at threshold 0 only.

(5), unfused arithmetic: a slab session across ranks exists in FMA arithmetic only (option panel_sessions), so with several ranks in
unfused mode the solve is kept out by the gate "no session for the operands' kind" and counts nowhere -- option 1 is then option 0
by construction, which the digests confirm; the counters are asserted to show the path on every rank in FMA mode and on one rank
in both modes.

Measured on an MI355X (test 4, n = 65, six iterations): see profiles/README.md."""
import json
import os
import re
import subprocess
import sys
import uuid

import numpy as np
import pytest

from gen import banded_triplets
from golden_util import Golden, to_dense
from test_gpu_power_vector import band, bits, full_row_and_column, pick_threshold, with_empties

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION = "cg_dots"
REL = 1e-13
SLOTS = ("solves", "passes", "refused", "not_formed")


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture(params=[1, 0], ids=["fma", "unfused"])
def arith(nt, request):
    before = {k: nt.get_option(k) for k in ("spgemm_fma", OPTION)}
    nt.set_option("spgemm_fma", request.param)
    yield request.param
    for k, v in before.items():
        nt.set_option(k, v)


# ------------------------------------------------------------------ operands
def one(v):
    return (np.array([1], dtype=np.int32), np.array([1], dtype=np.int32), np.array([v]))


# name: (n, U, V) -- two different non-symmetric bands; V None: the case U = V
PAIRS = {
    "band257": lambda: (257, band(257, 24, 9), band(257, 9, 24, shift=0.5)),
    "n63": lambda: (63, band(63, 24, 9), band(63, 9, 24, shift=0.5)),
    "n65": lambda: (65, band(65, 24, 9), band(65, 9, 24, shift=0.5)),
    "n1": lambda: (1, one(2.5), one(-1.5)),
    "empties150": lambda: (150, with_empties(150), band(150, 9, 24, shift=0.5)),
    "rowcol130": lambda: (130, full_row_and_column(130), band(130, 9, 24, shift=0.5)),
    "same257": lambda: (257, band(257, 24, 9), None),
}


def make(name, cplx):
    n, U, V = PAIRS[name]()
    out = []
    for seed, t in ((7, U), (8, V)):
        if t is None:
            out.append(None)
            continue
        col, row, val = t
        if cplx:
            val = val + 1j * 0.3 * np.random.default_rng(seed).standard_normal(len(val))
        out.append((col, row, val))
    return n, out[0], out[1]


def dense(n, t):
    A = np.zeros((n, n), dtype=t[2].dtype)
    A[t[1] - 1, t[0] - 1] = t[2]
    return A


def reference(nt, n, U, V, thr):
    """(diagonal, MatrixTrace) of MatrixMultiply(U^H, V, thr) through the public calls; 0.0 stands for an absent entry"""
    UT = nt.Matrix_ps(n)
    UT.Transpose(U)
    if U.IsComplex():
        UT.Conjugate()
    Cm = nt.Matrix_ps(n)
    Cm.Gemm(UT, V, threshold=thr)
    col, row, val = Cm.triplets()
    d = np.zeros(n, dtype=val.dtype)
    on = col == row
    d[col[on] - 1] = val[on]
    return d, Cm.Trace()


def thresholds_for(n, Ud, Vd):
    dd = np.einsum("kj,kj->j", np.conj(Ud), Vd)
    t = pick_threshold(dd)
    if t is None:
        assert n == 1, "every operand but n = 1 has a pruning threshold"
        return [0.0]
    return [0.0, t]


# ------------------------------------------------------------------ 1. the pass is the product's diagonal
@pytest.mark.parametrize("name", list(PAIRS))
def test_pass_is_the_diagonal_of_the_product(nt, arith, name):
    nt.set_option(OPTION, 1)
    n, tu, tv = make(name, False)
    U = nt.Matrix_ps.from_triplets(n, *tu)
    V = U if tv is None else nt.Matrix_ps.from_triplets(n, *tv)
    Ud = dense(n, tu)
    Vd = Ud if tv is None else dense(n, tv)
    kept = {}
    for thr in thresholds_for(n, Ud, Vd):
        tag = (name, thr)
        want_d, want_t = reference(nt, n, U, V, thr)
        before = nt.cg_dots_counts()
        got = nt.cg_dots(U, V, thr)
        assert got is not None, tag
        assert nt.cg_dots_counts() == before, tag   # (the diagnostic entry point counts nothing)
        d, t = got
        print(name, thr, np.count_nonzero(d), t, want_t)
        assert np.array_equal(bits(d), bits(want_d)), tag + (np.abs(d - want_d).max(),)
        assert bits(np.array([t]))[0] == bits(np.array([want_t]))[0], tag + (t, want_t)
        kept[thr] = np.count_nonzero(d)
        # the same bits again, and the operands are whole afterwards
        again = nt.cg_dots(U, V, thr)
        assert np.array_equal(bits(again[0]), bits(d)) and again[1] == t, tag
    for thr, k in kept.items():
        if thr > 0:
            share = (kept[0.0] - k) / kept[0.0]
            assert 0.1 <= share <= 0.5, (name, thr, share)
    cu, ru, vu = U.triplets()
    assert np.array_equal(cu, tu[0]) and np.array_equal(ru, tu[1]) and np.array_equal(bits(vu), bits(tu[2])), name


# ------------------------------------------------------------------ 2. complex
@pytest.mark.parametrize("name", list(PAIRS))
def test_complex_pass_in_the_tile_kernels_tolerance_mode(nt, name):
    before = {k: nt.get_option(k) for k in ("spgemm_fma", OPTION)}
    try:
        nt.set_option("spgemm_fma", 1)
        nt.set_option(OPTION, 2)
        n, tu, tv = make(name, True)
        U = nt.Matrix_ps.from_triplets(n, *tu)
        V = U if tv is None else nt.Matrix_ps.from_triplets(n, *tv)
        Ud = dense(n, tu)
        Vd = Ud if tv is None else dense(n, tv)
        kept = {}
        for thr in thresholds_for(n, Ud, Vd):
            tag = (name, thr)
            want_d, want_t = reference(nt, n, U, V, thr)
            got = nt.cg_dots(U, V, thr)
            assert got is not None, tag
            d, t = got
            # (the rule of close() in tests/test_gpu_complex_tile.py on the diagonal: entries on one side only sit at the threshold)
            scale = max(1.0, np.abs(want_d).max())
            diff = np.abs(d - want_d.real)
            print(name, thr, np.count_nonzero(d), diff.max(), t, want_t)
            bad = diff > REL * scale
            assert np.all(diff[bad] <= thr * (1 + 1e-9) + REL * scale), tag + (diff.max(),)
            assert abs(np.count_nonzero(d) - np.count_nonzero(want_d.real)) <= 8, tag
            assert abs(t - want_t) <= REL * scale * n + 8 * thr, tag + (t, want_t)
            kept[thr] = np.count_nonzero(d)
        for thr, k in kept.items():
            if thr > 0:
                share = (kept[0.0] - k) / kept[0.0]
                assert 0.1 <= share <= 0.5, (name, thr, share)
        # option 1 is for real operands; unfused arithmetic has no complex session
        nt.set_option(OPTION, 1)
        assert nt.cg_dots(U, V, 0.0) is None, name
        nt.set_option(OPTION, 2)
        nt.set_option("spgemm_fma", 0)
        assert nt.cg_dots(U, V, 0.0) is None, name
    finally:
        for k, v in before.items():
            nt.set_option(k, v)


# ------------------------------------------------------------------ 3. the solve equals option 0
def params(nt, thr, conv, maxit, verbose=True):
    p = nt.SolverParameters()
    p.SetThreshold(thr)
    p.SetConvergeDiff(conv)
    p.SetMaxIterations(maxit)
    p.SetMonitorConvergence(False)
    p.SetVerbosity(verbose)
    return p


def logged(nt, path, call):
    """runs call() with the logger writing to `path`; (the last "Total Iterations" of the log, the iterations it lists).  The loop
    logs one "Convergence" element per iteration it ran and, as the reference does, II - 1 as the total: one less than it ran
    when the monitor ended it."""
    nt.ActivateLogger(True, str(path))
    try:
        call()
    finally:
        nt.DeactivateLogger()
    text = open(str(path)).read()
    found = re.findall(r"Total Iterations:\s*(\d+)", text)
    assert found, "the solver logs its iteration count"
    return int(found[-1]), len(re.findall(r"^\s*- Convergence:", text, re.M))


def grown(nt, before):
    after = nt.cg_dots_counts()
    return tuple(after[k] - before[k] for k in SLOTS)


def same_matrix(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))


@pytest.mark.parametrize("n,h,thr,conv,maxit,ran", [(257, 24, 1e-5, 1e-30, 8, 8), (130, 8, 1e-6, 1e-5, 100, 13)])
def test_solve_with_the_passes_is_the_solve_on_compressed_columns(nt, arith, tmp_path, n, h, thr, conv, maxit, ran):
    """`ran`: the iterations a dense numpy restatement of the loop runs (8: the last one drops the whole diagonal of R^H R, the
    step is 0 and the monitor ends the loop; 13)."""
    A = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, h, shift=2.5))
    B = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, max(2, h // 3), shift=0.5))
    p = params(nt, thr, conv, maxit)
    res, its, counts = {}, {}, {}
    for opt in (0, 1):
        nt.set_option(OPTION, opt)
        X = nt.Matrix_ps(n)
        before = nt.cg_dots_counts()
        its[opt] = logged(nt, tmp_path / ("cg%d.log" % opt), lambda: nt.LinearSolvers.CGSolver(A, X, B, p))
        counts[opt] = grown(nt, before)
        res[opt] = X.triplets()
    print(n, h, its, counts, len(res[0][2]))
    assert np.isfinite(res[0][2]).all(), "precondition: the solve on compressed columns is finite"
    assert its[0][1] == ran, "precondition: the solve on compressed columns runs the restatement's iterations"
    assert its[1] == its[0]   # (the logged total and the iterations listed)
    assert same_matrix(res[1], res[0]), np.abs(to_dense((n, n) + tuple(res[1])) - to_dense((n, n) + tuple(res[0]))).max()
    assert counts[0] == (0, 0, 0, 0)
    assert counts[1][:3] == (1, 2 * ran, 0), counts[1]
    # per iteration three products and three transposes are not formed
    assert counts[1][3] == 6 * ran, counts[1]


def test_cg_and_pade_goldens_through_the_passes(nt, arith):
    g = Golden("extras")
    mats = {}
    seen = {"cg": 0, "pade": 0}
    nt.set_option(OPTION, 1)
    for i, c in enumerate(g.cases):
        kind = c["kind"]
        if kind not in seen:
            continue
        for k in (c["A"], c["B"]):
            if k is not None and k not in mats and k != "none_identity":
                t = g.tri(None, "M_" + k)
                mats[k] = nt.Matrix_ps.from_triplets(t[0], t[2], t[3], t[4])
        A, B = mats[c["A"]], mats.get(c["B"])
        n = A.GetActualDimension()
        p = nt.SolverParameters()
        p.SetThreshold(c["thr"])
        p.SetConvergeDiff(c["conv"])
        Out = nt.Matrix_ps(n)
        before = nt.cg_dots_counts()
        if kind == "cg":
            nt.LinearSolvers.CGSolver(A, Out, B, p)
        else:
            nt.ExponentialSolvers.ComputeExponentialPade(A, Out, p)
        grew = grown(nt, before)
        want = g.tri(i, "K")
        wd = to_dense(want)
        gd = to_dense((want[0], want[1]) + tuple(Out.triplets()))
        scale = max(1.0, np.abs(wd).max())
        err = np.abs(gd - wd).max()
        print(i, kind, c["A"], c["B"], A.IsComplex(), grew, err)
        if not A.IsComplex() and (B is None or not B.IsComplex()):
            # (an operand that is not run-like stays in compressed columns: its passes run there and count as refused)
            assert grew[0] == 1 and grew[1] + grew[2] >= 2, (i, grew)
        # (the tolerances of test_remaining_solver_families_golden)
        assert err <= {"pade": 1e-7, "cg": 1e-8}[kind] * scale, (i, kind, err)
        seen[kind] += 1
    assert seen["cg"] >= 1 and seen["pade"] >= 1, seen


def test_pade_exponential_takes_the_path_bit_for_bit(nt, arith):
    n = 130
    A = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, 8))
    p = nt.SolverParameters()
    p.SetThreshold(1e-7)
    p.SetConvergeDiff(1e-6)
    res = {}
    for opt in (0, 1):
        nt.set_option(OPTION, opt)
        Out = nt.Matrix_ps(n)
        before = nt.cg_dots_counts()
        nt.ExponentialSolvers.ComputeExponentialPade(A, Out, p)
        g = grown(nt, before)
        assert (g[0], g[2]) == ((1, 0) if opt else (0, 0)) and (g[1] >= 2) == bool(opt), (opt, g)
        res[opt] = Out.triplets()
    assert np.isfinite(res[0][2]).all()
    assert same_matrix(res[1], res[0])


# ------------------------------------------------------------------ 4. the complex solve
def dense_cg(A, B, steps):
    """the loop of solver_cg on dense numpy matrices at threshold 0"""
    n = A.shape[0]
    X = np.eye(n, dtype=A.dtype)
    R = B - A @ X
    P = R.copy()
    for _ in range(steps):
        Q = A @ P
        top = np.trace(R.conj().T @ R).real
        bottom = np.trace(P.conj().T @ Q).real
        step = top / bottom
        X = X + step * P
        R = R - step * Q
        new_top = np.trace(R.conj().T @ R).real
        P = (new_top / top) * P + R
    return X


def test_complex_solve_in_a_complex_session(nt):
    """n = 65, six fixed iterations, threshold 0, FMA arithmetic.  e0 = max |X(option 0) - X_np|, e2 = max |X(option 2) - X_np| for
    the dense numpy restatement X_np; asserted: e2 <= 10 e0.  Measured on an MI355X: profiles/README.md 138."""
    before = {k: nt.get_option(k) for k in ("spgemm_fma", OPTION)}
    try:
        nt.set_option("spgemm_fma", 1)
        n = 65
        ta = banded_triplets(n, 24, complex_=True, shift=2.5)
        tb = banded_triplets(n, 8, complex_=True, shift=0.5)
        A = nt.Matrix_ps.from_triplets(n, *ta)
        B = nt.Matrix_ps.from_triplets(n, *tb)
        Xnp = dense_cg(dense(n, ta), dense(n, tb), 6)
        p = params(nt, 0.0, 1e-30, 6, verbose=False)
        err = {}
        for opt in (0, 2):
            nt.set_option(OPTION, opt)
            X = nt.Matrix_ps(n)
            grew_before = nt.cg_dots_counts()
            nt.LinearSolvers.CGSolver(A, X, B, p)
            grew = grown(nt, grew_before)
            assert grew[:3] == ((1, 12, 0) if opt else (0, 0, 0)), (opt, grew)
            err[opt] = np.abs(to_dense((n, n) + tuple(X.triplets())) - Xnp).max()
        print("complex solve: e0 = %.3e, e2 = %.3e" % (err[0], err[2]))
        assert np.isfinite(err[0]) and err[2] <= 10 * err[0], err
    finally:
        for k, v in before.items():
            nt.set_option(k, v)


# ------------------------------------------------------------------ 5. several ranks
def run_world(world, tmp_path):
    out = str(tmp_path / ("cg%d" % world))
    name = "c%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name, NTPOLY_AMD_SHM_MB="8")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "cg_dots_worker.py"),
                                       "ranks", out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=300)
            logs.append(o)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        try:
            os.unlink("/dev/shm/ntpoly_amd_" + name)
        except OSError:
            pass
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d of %d failed:\n%s" % (r, world, logs[r][-3000:])
    return [(json.load(open(out + ".%d.json" % r)), np.load(out + ".%d.npz" % r)) for r in range(world)]


def assembled(parts, key, n):
    X = np.zeros((n, n))
    for _, arrays in parts:
        X[arrays[key + "_row"] - 1, arrays[key + "_col"] - 1] = arrays[key + "_val"]
    return X


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    return run_world(1, tmp_path_factory.mktemp("cg_ref"))


CASES = {"solve257": (257, 8), "n5": (5, 3)}   # name: (n, iterations)


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_equal_option_0_bit_for_bit_and_one_rank_to_rounding(world, one_rank, tmp_path):
    parts = run_world(world, tmp_path)
    for arith in ("fma", "unfused"):
        for name, (n, its) in CASES.items():
            k0, k1 = "%s_%s_0" % (name, arith), "%s_%s_1" % (name, arith)
            for rank, (rep, _) in enumerate(parts):
                print(world, rank, k1, rep[k0], rep[k1])
                assert rep[k1]["digest"] == rep[k0]["digest"] and rep[k1]["entries"] == rep[k0]["entries"], (k1, rank)
                assert rep[k0]["counts"] == [0, 0, 0, 0], (k0, rank)
                solves, passes, refused, _ = rep[k1]["counts"]
                if arith == "fma":   # (a panel session: the path ran on every rank)
                    assert solves == 1 and passes + refused == 2 * its and passes >= 1, (k1, rank, rep[k1]["counts"])
                else:                # (no session across ranks in unfused arithmetic: gated, counted nowhere)
                    assert rep[k1]["counts"] == [0, 0, 0, 0], (k1, rank)
            # one rank and `world` ranks: the reduction over ranks is another summation order
            X1, Xw = assembled(one_rank, k1, n), assembled(parts, k1, n)
            assert np.isfinite(X1).all(), k1
            assert np.abs(Xw - X1).max() <= 1e-9 * max(1.0, np.abs(X1).max()), (k1, np.abs(Xw - X1).max())
    # one rank: the path runs in both arithmetic modes
    for arith in ("fma", "unfused"):
        for name, (n, its) in CASES.items():
            rep = one_rank[0][0]
            assert rep["%s_%s_1" % (name, arith)]["counts"][:3] == [1, 2 * its, 0], (name, arith)
            assert rep["%s_%s_1" % (name, arith)]["digest"] == rep["%s_%s_0" % (name, arith)]["digest"], (name, arith)
    if world == 3:
        # n = 5 on three ranks: an uneven split of the columns
        assert sorted(rep["n5_width"] for rep, _ in parts) == [1, 2, 2]
