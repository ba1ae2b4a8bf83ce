"""GPU: ScaleAndFold with the fold update, the energy and the next step's trace in one pass (option scale_fold_step; csrc/slab_extra.hip
k_saf_update / k_saf_dot_trace, engine.hpp ps_saf_update / ps_saf_dot_trace).  Behind its one product X X -> X2 an iteration of the
fold branch calls, with the vocabulary at threshold 0, X *= 2 alpha; X += (-alpha^2) X2; energy = 2 dot(X, WH), and the next
iteration begins with trace(X).  The fused update reads the runs of X, X2 and WH once, writes the new X and returns both sums; in
the scale branch, whose product's result is the new X, one pass over X and WH returns them.

The kernels are reached with crafted operands through nt.scale_fold_update_step / nt.scale_fold_dot_trace and compared with (i) the
same vocabulary calls on compressed columns (slab_algebra = 0) and (ii) a numpy restatement of AddSparseVectors.f90 at threshold 0
written here -- never with the fused code itself.  numpy's float64 products and sums are the correctly rounded ones the kernel
spells as __dmul_rn / __dadd_rn, so patterns are compared for equality and values with np.array_equal.  The trace is held to the
bits of MatrixTrace on the new X in slab form: it decides the next branch."""
import ctypes as C
import math
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from gen import banded_triplets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 259   # (not a multiple of the 4 waves of a workgroup)
ALPHAS = (0.75, 1.25)   # 2 alpha and alpha^2 are short binary fractions, which the planted cancellations need
NONE = dict(updates=0, dot_traces=0, refused=0)


def factors(alpha):
    """(a, b) as solvers.cpp rounds them"""
    return -1.0 * alpha * alpha, 2 * alpha


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture(params=[1, 0], ids=["fma", "unfused"])
def fma(nt, request):
    """both arithmetic modes: slots padded to the tile kernel's row alignment, and runs packed back to back"""
    nt.set_option("spgemm_fma", request.param)
    yield request.param
    nt.set_option("spgemm_fma", 0)
    nt.set_option("slab_algebra", 1)
    nt.set_option("scale_fold_step", 1)


def srt(t):
    c, r, v = t
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def same(a, b):
    """sorted triplets: equal patterns, equal values"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------ operands
# a column is (rows, values)
EMPTY = {"X": {7, 40}, "X2": {8, 40}, "WH": {11}}   # empty in each operand in turn, column 40 in X and X2
DIAG_ONLY = {13}
BELOW, ABOVE = 60, 150    # columns whose runs lie beyond / before the diagonal row in every operand
NO_DIAG = 110             # a column whose X and X2 have a hole on the diagonal inside their runs
CANCEL, ONE_SIDED = 30, 31   # row 33: (2 alpha) x + (-alpha^2) x2 == 0 exactly; the same x with no X2 entry there
ROW = 33


def _runs(rng, n, empty):
    """{column: (rows, values)}: a run around the diagonal with half-widths 6..90 drawn per side, ~12 % holes inside, values
    log-uniform in [1e-6, 1] with a random sign"""
    cols = {}
    for j in range(n):
        if j in empty:
            continue
        if j in DIAG_ONLY:
            rows = np.array([j])
        else:
            if j == BELOW:
                f, l = j + 3, j + int(rng.integers(30, 60))
            elif j == ABOVE:
                f, l = j - int(rng.integers(30, 60)), j - 3
            else:
                f, l = max(0, j - int(rng.integers(6, 91))), min(n - 1, j + int(rng.integers(6, 91)))
            rows = np.arange(f, l + 1)
            keep = rng.random(len(rows)) > 0.12
            keep[0] = keep[-1] = True
            rows = rows[keep]
        cols[j] = (rows, 10.0 ** rng.uniform(-6.0, 0.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows)))
    return cols


def _set(cols, j, r, v):
    rows, vals = cols[j]
    if r in rows:
        vals[rows == r] = v
    else:
        k = int(np.searchsorted(rows, r))
        cols[j] = (np.insert(rows, k, r), np.insert(vals, k, v))


def _unset(cols, j, r):
    rows, vals = cols[j]
    cols[j] = (rows[rows != r], vals[rows != r])


def _plant(X, X2, alpha):
    """a cancellation, exact by construction and checked here in numpy"""
    a, b = factors(alpha)
    x2 = 0.75
    x = alpha * x2 / 2.0
    assert b * x + a * x2 == 0.0 and b * x != 0.0
    _set(X, CANCEL, ROW, x)
    _set(X2, CANCEL, ROW, x2)
    # ... and with no X2 entry there: the row keeps the one-sided (2 alpha) x
    _set(X, ONE_SIDED, ROW, x)
    _unset(X2, ONE_SIDED, ROW)
    for M in (X, X2):
        _unset(M, NO_DIAG, NO_DIAG)


@pytest.fixture(scope="module")
def operands():
    out = {}
    for alpha in ALPHAS:
        rng = np.random.default_rng(20261019)
        X, X2, WH = (_runs(rng, N, EMPTY[k]) for k in ("X", "X2", "WH"))
        _plant(X, X2, alpha)
        if alpha > 1.0:
            _set(WH, ONE_SIDED, ROW, 0.0)   # (a stored zero: this WH enters slab form as a read-only view)
        out[alpha] = (X, X2, WH)
    return out


def _triplets(cols):
    c, r, v = [], [], []
    for j in sorted(cols):
        rows, vals = cols[j]
        c.append(np.full(len(rows), j + 1))
        r.append(rows + 1)
        v.append(vals)
    if not c:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)
    return np.concatenate(c).astype(np.int32), np.concatenate(r).astype(np.int32), np.concatenate(v)


def _matrix(nt, cols, n=N):
    c, r, v = _triplets(cols)
    M = nt.Matrix_ps.from_triplets(n, c, r, v)
    assert len(M.triplets()[2]) == len(v)
    return M


# ------------------------------------------------------------------ AddSparseVectors.f90 at threshold 0, restated
def add_sparse(a, alpha, b, beta, stats, tag):
    """alpha a + beta b on sorted sparse vectors (rows, values), the scaled values rounded, then added: inside the overlap of the
    two lists an entry is kept iff its value is not zero, beyond the end of one list the tail of the other is copied unfiltered"""
    (ra, va), (rb, vb) = a, b
    if len(ra) == 0 and len(rb) == 0:
        return ra, va
    rows = np.union1d(ra, rb)
    ia, ib = np.isin(rows, ra), np.isin(rows, rb)
    wa, wb = np.zeros(len(rows)), np.zeros(len(rows))
    wa[ia] = alpha * va
    wb[ib] = beta * vb
    s = np.where(ia & ib, wa + wb, np.where(ia, wa, wb))
    lim = min(ra[-1] if len(ra) else -1, rb[-1] if len(rb) else -1)
    nz = s != 0.0
    keep = (rows > lim) | nz
    stats[tag + "_both_kept"] = stats.get(tag + "_both_kept", 0) + int((ia & ib & nz).sum())
    stats[tag + "_cancelled"] = stats.get(tag + "_cancelled", 0) + int((ia & ib & ~nz).sum())
    stats[tag + "_only_a"] = stats.get(tag + "_only_a", 0) + int((ia & ~ib).sum())
    stats[tag + "_only_b"] = stats.get(tag + "_only_b", 0) + int((~ia & ib).sum())
    stats["underflow"] = stats.get("underflow", 0) + int((~nz & ~(ia & ib)).sum())
    return rows[keep], s[keep]


def restated(X, X2, WH, alpha):
    """the new X, the terms of dot(X, WH) and the new diagonal, column by column, and branch statistics"""
    a, b = factors(alpha)
    empty = (np.zeros(0, dtype=np.int64), np.zeros(0))
    st, new, terms, diag = {}, {}, [], []
    for j in range(N):
        x, x2, w = X.get(j, empty), X2.get(j, empty), WH.get(j, empty)
        s = (x[0], b * x[1])                                        # ScaleMatrix(X, 2 alpha)
        st["underflow"] = st.get("underflow", 0) + int((s[1] == 0.0).sum())
        o = add_sparse(s, 1.0, x2, a, st, "o")                      # IncrementMatrix(X2, X, -alpha^2)
        st["empty_result"] = st.get("empty_result", 0) + int(len(o[0]) == 0)
        st["diagonal_absent"] = st.get("diagonal_absent", 0) + int(j not in o[0])
        if len(o[0]):
            new[j] = o
        both = np.intersect1d(o[0], w[0])
        terms.append(o[1][np.isin(o[0], both)] * w[1][np.isin(w[0], both)])
        diag.append(o[1][o[0] == j][0] if j in o[0] else 0.0)
    return new, np.concatenate(terms), np.array(diag), st


@pytest.fixture(scope="module")
def references(operands):
    return {alpha: restated(*operands[alpha], alpha) for alpha in ALPHAS}


def test_the_inputs_reach_every_branch(operands, references):
    """from the operands and the numpy restatement alone: columns empty in X, in X2, in both and in WH, a diagonal-only column, runs
    wholly beyond and before the diagonal row, a hole on the diagonal, columns 0 and N - 1, and in the merge both-present sums
    that are kept, one that cancels, one-sided entries from either side; no scaled entry underflows (the restatement would hold
    a stored zero the runs cannot); one WH stores a zero"""
    for alpha in ALPHAS:
        X, X2, WH = operands[alpha]
        assert 7 not in X and 7 in X2 and 8 not in X2 and 8 in X and 40 not in X and 40 not in X2 and 40 in WH and 11 not in WH
        for M in (X, X2):
            assert 0 in M and N - 1 in M and M[BELOW][0][0] > BELOW and M[ABOVE][0][-1] < ABOVE and list(M[13][0]) == [13]
            assert NO_DIAG not in M[NO_DIAG][0] and M[NO_DIAG][0][0] < NO_DIAG < M[NO_DIAG][0][-1]
        assert ROW in X[CANCEL][0] and ROW in X2[CANCEL][0] and ROW in X[ONE_SIDED][0] and ROW not in X2[ONE_SIDED][0]
        new, terms, diag, st = references[alpha]
        print(alpha, st, "terms", len(terms))
        assert st["underflow"] == 0
        assert st["o_cancelled"] == 1 and st["o_both_kept"] > 1000 and st["o_only_a"] > 0 and st["o_only_b"] > 0, st
        assert st["empty_result"] == 1 and 40 not in new
        assert st["diagonal_absent"] >= 4 and all(diag[j] == 0.0 for j in (40, BELOW, ABOVE, NO_DIAG)) and diag[13] != 0.0 and diag[N - 1] != 0.0
        a, b = factors(alpha)
        assert ROW not in new[CANCEL][0] and new[ONE_SIDED][1][new[ONE_SIDED][0] == ROW][0] == b * (alpha * 0.75 / 2.0)
        assert new[N - 1][0][-1] == N - 1
        assert len(terms) > 1000
    assert np.any(operands[ALPHAS[1]][2][ONE_SIDED][1] == 0.0) and not any(np.any(v == 0.0) for _, v in operands[ALPHAS[0]][2].values())


def _vocabulary(nt, MX, MX2, MW, alpha):
    """the calls of solvers.cpp solver_scale_and_fold behind its product, through the C ABI"""
    a, b = factors(alpha)
    V = nt.Matrix_ps(MX)
    V.Scale(b)
    V.Increment(MX2, a, 0.0)
    return V, V.Dot(MW)


def _dot_in_session(nt, A, B):
    """DotMatrix through the C ABI alone (host.py's Dot first asks whether the matrices are complex, an entry point that packs
    them): inside a session it leaves both operands in slab form"""
    v = C.c_double()
    nt.lib.DotMatrix_psr_wrp(A.ih, B.ih, C.byref(v))
    return v.value


def _sum_bound(terms):
    """any summation order of m numbers is within (m - 1) u sum |t| (1 + O(m u)) of their exact sum, u = 2^-53; the terms here are
    the rounded products themselves, so m 2^-52 sum |t| holds with room for the second-order part"""
    return math.fsum(terms), len(terms) * 2.0 ** -52 * math.fsum(np.abs(terms))


@pytest.mark.parametrize("alpha", ALPHAS)
def test_update_bit_for_bit(nt, fma, operands, references, alpha):
    X, X2, WH = operands[alpha]
    new, terms, diag, _ = references[alpha]
    a, b = factors(alpha)
    want = _triplets(new)
    Ms = [_matrix(nt, c) for c in (X, X2, WH)]
    before = [srt(m.triplets()) for m in Ms]
    # (i) the vocabulary on compressed columns against (ii) the restatement
    nt.set_option("slab_algebra", 0)
    V, ev = _vocabulary(nt, *Ms, alpha)
    nt.set_option("slab_algebra", 1)
    assert same(srt(V.triplets()), want), "compressed columns against the restatement"
    # the fused update; then, in the same session, MatrixTrace of the restated new X in slab form (a dot with X2, which the update
    # has left in slab form, brings it there)
    O, Mn = nt.Matrix_ps(N), _matrix(nt, new)
    c0, s0 = nt.scale_fold_step_counts(), nt.slab_algebra_counts()
    with nt.solver_session(False):
        got = nt.scale_fold_update_step(Ms[0], Ms[1], a, b, Ms[2], O)
        c1, s1 = nt.scale_fold_step_counts(), nt.slab_algebra_counts()
        _dot_in_session(nt, Mn, Ms[1])
        s2 = nt.slab_algebra_counts()
        ts = Mn.Trace()
        s3 = nt.slab_algebra_counts()
    print(alpha, "counts", c0, c1, "slab algebra", s0, s1, s2, s3)
    assert got is not None
    e, t = got
    assert {k: c1[k] - c0[k] for k in c1} == dict(updates=1, dot_traces=0, refused=0)
    assert s1["merges"] - s0["merges"] == 1 and s1["others"] - s0["others"] == 2 and s1["refusals"] == s0["refusals"]
    assert s2["others"] - s1["others"] == 1 and s3["others"] - s2["others"] == 1 and s3["refusals"] == s0["refusals"], "the trace was taken in slab form"
    for m, bf in zip(Ms, before):
        assert same(srt(m.triplets()), bf), "the operands are as they were"
    g = srt(O.triplets())
    print(alpha, "entries", len(want[2]))
    assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]), "pattern"
    assert same(g, want), "values against the restatement"
    assert same(g, srt(V.triplets())), "values against compressed columns"
    # the trace: the bits of MatrixTrace on the new X in slab form; and within the bound of any summation order of the diagonal
    exact_t, bound_t = _sum_bound(diag)
    print(alpha, "trace", t, "MatrixTrace in slab form", ts, "exact", exact_t, "bound", bound_t)
    assert t == ts
    assert abs(t - exact_t) <= bound_t
    # the energy's dot
    exact, bound = _sum_bound(terms)
    print(alpha, "dot", e, "exact", exact, "|difference|", abs(e - exact), "bound", bound, "compressed columns", ev)
    assert abs(e - exact) <= bound
    assert abs(ev - exact) <= bound


@pytest.mark.parametrize("alpha", ALPHAS)
def test_dot_and_trace_pass(nt, fma, operands, references, alpha):
    """the pass behind the scale branch's product, on the new X of the update test: nothing written, both sums returned"""
    new, terms, diag, _ = references[alpha]
    MX, MW = _matrix(nt, new), _matrix(nt, operands[alpha][2])
    before = [srt(m.triplets()) for m in (MX, MW)]
    c0, s0 = nt.scale_fold_step_counts(), nt.slab_algebra_counts()
    with nt.solver_session(False):
        got = nt.scale_fold_dot_trace(MX, MW)
        c1, s1 = nt.scale_fold_step_counts(), nt.slab_algebra_counts()
        ts = MX.Trace()
        s2 = nt.slab_algebra_counts()
    print(alpha, "counts", c0, c1, "slab algebra", s0, s1, s2)
    assert got is not None
    e, t = got
    assert {k: c1[k] - c0[k] for k in c1} == dict(updates=0, dot_traces=1, refused=0)
    assert s1["merges"] == s0["merges"] and s1["others"] - s0["others"] == 2 and s1["refusals"] == s0["refusals"]
    assert s2["others"] - s1["others"] == 1 and s2["refusals"] == s0["refusals"], "the trace was taken in slab form"
    for m, bf in zip((MX, MW), before):
        assert same(srt(m.triplets()), bf), "the operands are as they were"
    exact_t, bound_t = _sum_bound(diag)
    exact, bound = _sum_bound(terms)
    print(alpha, "trace", t, ts, "dot", e, "exact", exact, "|difference|", abs(e - exact), "bound", bound)
    assert t == ts and abs(t - exact_t) <= bound_t
    assert abs(e - exact) <= bound


# ------------------------------------------------------------------ refusals
def test_refusals_leave_everything_as_it_was(nt, fma):
    n, j = 4099, 5
    col = lambda f, l, v=None: {j: (np.arange(f, l + 1), np.linspace(0.1, 0.9, l - f + 1) if v is None else v)}

    def refused(MX, MX2, MW, a, b):
        O = nt.Matrix_ps(n)
        before = [srt(m.triplets()) for m in (MX, MX2, MW)]
        c0, s0 = nt.scale_fold_step_counts(), nt.slab_algebra_counts()
        with nt.solver_session(False):
            got = nt.scale_fold_update_step(MX, MX2, a, b, MW, O)
        c1, s1 = nt.scale_fold_step_counts(), nt.slab_algebra_counts()
        assert got is None
        assert c1 == dict(c0, refused=c0["refused"] + 1), (c0, c1)
        assert s1 == s0, (s0, s1)   # (a refused update is no operation and no refusal of the session)
        for m, bf in zip((MX, MX2, MW), before):
            assert same(srt(m.triplets()), bf)
        assert len(O.triplets()[2]) == 0

    MX, near, MW = _matrix(nt, col(0, 9), n=n), _matrix(nt, col(4, 20), n=n), _matrix(nt, col(0, 30), n=n)
    far = _matrix(nt, col(n // 2 + 1, n // 2 + 11), n=n)
    a, b = factors(0.75)
    # two runs n / 2 rows apart in one column, either way round: the hull is beyond what the column's slots bound
    refused(MX, far, MW, a, b)
    refused(far, MX, MW, a, b)
    # 1e-300 x 1e-30 rounds to zero: an underflow
    tiny = _matrix(nt, col(0, 9, np.full(10, 1e-30)), n=n)
    refused(tiny, near, MW, a, 1e-300)
    # a factor that is not finite: refused before anything is launched
    refused(MX, near, MW, float("nan"), b)
    refused(MX, near, MW, a, float("inf"))
    # the same column with the runs side by side is taken
    O = nt.Matrix_ps(n)
    with nt.solver_session(False):
        got = nt.scale_fold_update_step(MX, near, a, b, MW, O)
    assert got is not None
    x, x2, w = np.zeros(31), np.zeros(31), np.linspace(0.1, 0.9, 31)   # (adding an absent entry as +0.0 gives the merge's values)
    x[0:10], x2[4:21] = np.linspace(0.1, 0.9, 10), np.linspace(0.1, 0.9, 17)
    o = b * x + a * x2
    assert np.all(o[:21] != 0.0) and np.all(o[21:] == 0.0)
    cc, rr, vv = srt(O.triplets())
    assert np.all(cc == j + 1) and np.array_equal(rr, np.arange(1, 22)) and np.array_equal(vv, o[:21])
    exact, bound = _sum_bound(o * w)
    assert abs(got[0] - exact) <= bound and got[1] == o[j]


# ------------------------------------------------------------------ the solver
SOLVE = (4096, 20, 1e-8, 12)   # the configuration of test_gpu_slab_algebra.py test_other_purification_loops_in_slab_form
HOMO_LUMO = (-0.05, 0.05)


def saf_solve(nt, H, n, iters=SOLVE[3], thr=SOLVE[2], homo_lumo=HOMO_LUMO):
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    p = nt.SolverParameters()
    p.SetThreshold(thr)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(iters)
    p.SetMonitorConvergence(False)
    K = nt.Matrix_ps(n)
    c0, s0 = nt.scale_fold_step_counts(), nt.slab_algebra_counts()
    e = nt.DensityMatrixSolvers.ScaleAndFold(H, I, n / 2.0, K, homo_lumo[0], homo_lumo[1], p)
    c1, s1 = nt.scale_fold_step_counts(), nt.slab_algebra_counts()
    tr = nt.solver_trace()
    return dict(out=srt(K.triplets()), e=e, iters=tr["iterations"], sigma=np.asarray(tr["sigma"]).copy(), nnz=np.asarray(tr["nnz"]).copy(),
                energy=np.asarray(tr["energy"]).copy(), step={k: c1[k] - c0[k] for k in c1}, refusals=s1["refusals"] - s0["refusals"])


@pytest.fixture(scope="module")
def hamiltonian(nt):
    n, h = SOLVE[0], SOLVE[1]
    return nt.Matrix_ps.from_triplets(n, *banded_triplets(n, h)), n


def test_solver_option_1_against_option_0(nt, fma, hamiltonian):
    """the trace keeps its bits, the update its values and pattern, and the energy never enters the iterate: the branch sequence,
    the entry counts and the density are those of option 0 bit for bit; the energies, summed in another order, to 1e-10 relative.
    The option-0 run takes both branches within its 12 iterations (a condition on the inputs, checked on the reference run), so
    both kernels are reached"""
    H, n = hamiltonian
    nt.set_option("scale_fold_step", 0)
    off = saf_solve(nt, H, n)
    nt.set_option("scale_fold_step", 1)
    on = saf_solve(nt, H, n)
    print("iterations", on["iters"], "step", on["step"], "refusals", on["refusals"], off["refusals"], "branches of option 0", off["sigma"].tolist())
    print("max relative energy difference", float(np.max(np.abs(on["energy"] - off["energy"]) / np.abs(off["energy"]))))
    assert set(off["sigma"].tolist()) == {-1.0, 1.0}, "the reference run takes both branches"
    assert off["step"] == NONE
    assert on["iters"] == off["iters"] == SOLVE[3]
    assert np.array_equal(on["sigma"], off["sigma"]), "branch sequence, bit for bit"
    assert np.array_equal(on["nnz"], off["nnz"])
    assert same(on["out"], off["out"]), "density triplets, bit for bit"
    assert np.all(np.abs(on["energy"] - off["energy"]) <= 1e-10 * np.abs(off["energy"]))
    assert abs(on["e"] - off["e"]) <= 1e-10 * abs(off["e"])
    assert on["step"]["updates"] >= 1 and on["step"]["dot_traces"] >= 1 and on["step"]["refused"] == 0, on["step"]
    assert on["step"]["updates"] + on["step"]["dot_traces"] >= on["iters"] - 1, on["step"]
    assert on["refusals"] <= off["refusals"]


def test_gates(nt, fma, hamiltonian):
    """the option at 0, slab_algebra = 0 and a complex Hamiltonian fuse nothing and refuse nothing: the results of option 0"""
    H, n = hamiltonian
    iters = 4

    def equal(x, y):
        return (x["iters"] == y["iters"] and same(x["out"], y["out"]) and np.array_equal(x["sigma"], y["sigma"]) and
                np.array_equal(x["energy"], y["energy"]) and np.array_equal(x["nnz"], y["nnz"]) and x["e"] == y["e"])

    nt.set_option("scale_fold_step", 0)
    want = saf_solve(nt, H, n, iters)
    again = saf_solve(nt, H, n, iters)
    assert want["step"] == NONE == again["step"] and equal(want, again)
    nt.set_option("scale_fold_step", 1)
    nt.set_option("slab_algebra", 0)
    a = saf_solve(nt, H, n, iters)
    nt.set_option("scale_fold_step", 0)
    want_a = saf_solve(nt, H, n, iters)
    nt.set_option("slab_algebra", 1)
    nt.set_option("scale_fold_step", 1)
    assert a["step"] == NONE == want_a["step"] and equal(a, want_a)
    nc, hc = 1024, 12
    Hc = nt.Matrix_ps.from_triplets(nc, *banded_triplets(nc, hc, complex_=True))
    c = saf_solve(nt, Hc, nc, iters)
    nt.set_option("scale_fold_step", 0)
    d = saf_solve(nt, Hc, nc, iters)
    nt.set_option("scale_fold_step", 1)
    assert c["step"] == NONE == d["step"] and equal(c, d)


# ------------------------------------------------------------------ two ranks
def run_world(world, tmp_path):
    out = str(tmp_path / ("saf%d" % world))
    name = "s%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name, NTPOLY_AMD_SHM_MB="64",
                   NTPOLY_AMD_SPGEMM_FMA="1")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "scale_fold_step_worker.py"), out],
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


def test_two_ranks_option_1_against_option_0(tmp_path):
    """ScaleAndFold of a real band, n = 4096, as column panels on two ranks sharing one GPU (shared-memory transport, FMA arithmetic),
    option 1 against option 0 in the same processes: the same iteration count, the branch sequence bit for bit (one reduction
    carries dot and trace, element by element what two carry), the gathered density bit for bit, fused steps on both ranks"""
    two = run_world(2, tmp_path)
    for r, p in enumerate(two):
        print("rank", r, "iterations", int(p["iters_on"][0]), "counts (updates, dot_traces, refused)", p["counts_on"].tolist(), p["counts_off"].tolist(),
              "branches", p["sigma_off"].tolist())
        assert int(p["iters_on"][0]) == int(p["iters_off"][0]) == 12
        assert np.array_equal(p["sigma_on"], p["sigma_off"]), "branch sequence, bit for bit"
        assert np.array_equal(p["nnz_on"], p["nnz_off"])
        assert np.all(np.abs(p["energy_on"] - p["energy_off"]) <= 1e-10 * np.abs(p["energy_off"]))
        assert p["counts_off"].tolist() == [0, 0, 0]
        assert p["counts_on"][0] + p["counts_on"][1] >= 11 and p["counts_on"][2] == 0, (r, p["counts_on"])
    for k in ("col", "row", "val"):
        assert np.array_equal(np.concatenate([p[k + "_on"] for p in two]), np.concatenate([p[k + "_off"] for p in two])), k
    assert len(np.concatenate([p["val_on"] for p in two])) > 4096
    assert np.array_equal(two[0]["sigma_on"], two[1]["sigma_on"])
