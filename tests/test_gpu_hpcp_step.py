"""GPU: HPCP purification with its two traces and its update in one pass each (option hpcp_step; csrc/slab_extra.hip k_hpcp_traces /
k_hpcp_update, engine.hpp ps_hpcp_traces / ps_hpcp_update).  Around its two products D1 (I - D1) -> DDH and D1 DDH -> D2DH an
iteration calls, with the vocabulary at threshold 0, D1 += 2 D2DH; D1 += (-2 sigma) DDH; energy = dot(D1, WH), and at the top of
the next iteration DH = D1; DH += (-1) I; DH *= -1.  The fused update reads the three runs and WH once and writes the new D1 and DH.

The kernel is reached with crafted operands through nt.hpcp_update_step and compared with (i) the same vocabulary calls on
compressed columns (slab_algebra = 0) and (ii) a numpy restatement of AddSparseVectors.f90 at threshold 0 written here -- never
with the fused code itself.  numpy's float64 products and sums are the correctly rounded ones the kernel spells as __dmul_rn /
__dadd_rn, so patterns are compared for equality and values with np.array_equal.  The traces are held to their bits through the
solver: sigma is their quotient."""
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
SIGMAS = (0.375, -0.75)   # one positive, one negative; -2 sigma is then a short binary fraction, which the planted sums need
NAMES = ("D1", "DDH", "D2DH")


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
    nt.set_option("hpcp_step", 1)


def srt(t):
    c, r, v = t
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def same(a, b):
    """sorted triplets: equal patterns, equal values"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------ operands
# a column is (rows, values)
EMPTY = {"D1": {7, 40}, "DDH": {8, 40}, "D2DH": {9, 40}, "WH": {11}}   # empty in each operand in turn, column 40 in all three
DIAG_ONLY = {13}
BELOW, ABOVE = 60, 150   # columns whose runs lie beyond / before the diagonal row in every operand
NO_DIAG = 110            # a column whose D1, DDH and D2DH have a hole on the diagonal inside their runs
ONE_INSIDE, ONE_AT_END = 50, N - 1   # columns whose new D1 has exactly 1.0 on the diagonal: inside its run, and as its last row


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


def _plant(D1, DDH, D2DH, sigma):
    """cancellations, exact by construction and checked here in numpy"""
    s2 = -1.0 * 2.0 * sigma
    # t = d1 + 2 d2dh = 0 (the entry of the new D1 is then the one-sided (-2 sigma) ddh)
    x = 0.731
    _set(D2DH, 20, 25, x)
    _set(D1, 20, 25, -(2.0 * x))
    _set(DDH, 20, 25, 0.0417)
    assert -(2.0 * x) + 2.0 * x == 0.0
    # ... and with no DDH entry there: nothing is left of the row
    _set(D2DH, 21, 25, x)
    _set(D1, 21, 25, -(2.0 * x))
    _unset(DDH, 21, 25)
    # o = t + (-2 sigma) ddh = 0: w = fl(s2 y), d2dh = -w, d1 = w, so t = w + (-2 w) = -w exactly
    y = 0.0917
    w = s2 * y
    _set(DDH, 30, 33, y)
    _set(D2DH, 30, 33, -w)
    _set(D1, 30, 33, w)
    assert (w + 2.0 * (-w)) + s2 * y == 0.0
    # o = 1.0 on a diagonal: inside the runs, and as the last row of every run (the last column)
    for j in (ONE_INSIDE, ONE_AT_END):
        for c, yd in ((0.125, 0.5), (0.25, 0.25), (0.0625, 1.0)):
            wd = s2 * yd
            xd = (1.0 - wd) - 2.0 * c
            if xd != 0.0 and (xd + 2.0 * c) + wd == 1.0:
                break
        else:
            raise AssertionError("no exact 1.0 among the candidates")
        _set(D1, j, j, xd)
        _set(D2DH, j, j, c)
        _set(DDH, j, j, yd)
    # a column whose D1 lacks the diagonal (and so do DDH and D2DH: the new D1 lacks it too, DH holds +1 there)
    for M in (D1, DDH, D2DH):
        _unset(M, NO_DIAG, NO_DIAG)


@pytest.fixture(scope="module")
def operands():
    out = {}
    for sigma in SIGMAS:
        rng = np.random.default_rng(20261019)
        D1, DDH, D2DH = (_runs(rng, N, EMPTY[k]) for k in NAMES)
        WH = _runs(rng, N, EMPTY["WH"])
        _plant(D1, DDH, D2DH, sigma)
        if sigma < 0:
            _set(WH, 31, 33, 0.0)   # (a stored zero: this WH enters slab form as a read-only view)
        out[sigma] = (D1, DDH, D2DH, WH)
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
    stats[tag + "_cancelled"] = stats.get(tag + "_cancelled", 0) + int((ia & ib & ~nz).sum())
    stats[tag + "_only_a"] = stats.get(tag + "_only_a", 0) + int((ia & ~ib).sum())
    stats[tag + "_only_b"] = stats.get(tag + "_only_b", 0) + int((~ia & ib).sum())
    stats["underflow"] = stats.get("underflow", 0) + int((~nz & ~(ia & ib)).sum())
    return rows[keep], s[keep]


def restated(D1, DDH, D2DH, WH, sigma):
    """the new D1, the DH made from it and the terms of dot(D1, WH), column by column, and branch statistics"""
    empty = (np.zeros(0, dtype=np.int64), np.zeros(0))
    st, new, dh, terms = {}, {}, {}, []
    for j in range(N):
        a, b, c, w, d = D1.get(j, empty), DDH.get(j, empty), D2DH.get(j, empty), WH.get(j, empty), (np.array([j]), np.array([1.0]))
        t = add_sparse(a, 1.0, c, 2.0, st, "t")                     # IncrementMatrix(D2DH, D1, 2)
        o = add_sparse(t, 1.0, b, -1.0 * 2.0 * sigma, st, "o")      # IncrementMatrix(DDH, D1, -2 sigma)
        u = add_sparse(o, 1.0, d, -1.0, st, "u")                    # CopyMatrix(D1, DH); IncrementMatrix(Identity, DH, -1)
        st["d1_lacks_diagonal"] = st.get("d1_lacks_diagonal", 0) + int(j not in a[0])
        st["o_is_one"] = st.get("o_is_one", 0) + int(j in o[0] and o[1][o[0] == j][0] == 1.0)
        if len(o[0]):
            new[j] = o
        if len(u[0]):
            dh[j] = (u[0], -1.0 * u[1])                             # ScaleMatrix(DH, -1)
        both = np.intersect1d(o[0], w[0])
        terms.append(o[1][np.isin(o[0], both)] * w[1][np.isin(w[0], both)])
    return new, dh, np.concatenate(terms), st


@pytest.fixture(scope="module")
def references(operands):
    return {sigma: restated(*operands[sigma], sigma) for sigma in SIGMAS}


def test_the_inputs_reach_every_branch(operands, references):
    """from the operands and the numpy restatement alone: columns empty in each operand in turn and in all three, a diagonal-only
    column, runs wholly beyond and before the diagonal, columns 0 and N - 1, in every merge both-present sums that cancel and
    one-sided entries from either side, 1.0 on a diagonal inside a run and at its end, a D1 without its diagonal; no scaled
    entry underflows (the restatement would hold a stored zero the runs cannot)"""
    for sigma in SIGMAS:
        D1, DDH, D2DH, WH = operands[sigma]
        assert 7 not in D1 and 7 in DDH and 7 in D2DH and 8 not in DDH and 8 in D1 and 9 not in D2DH and 9 in D1
        assert all(40 not in M for M in (D1, DDH, D2DH)) and 11 not in WH
        for M in (D1, DDH, D2DH):
            assert 0 in M and N - 1 in M and M[BELOW][0][0] > BELOW and M[ABOVE][0][-1] < ABOVE and list(M[13][0]) == [13]
            assert M[ONE_AT_END][0][-1] == ONE_AT_END and NO_DIAG not in M[NO_DIAG][0] and M[NO_DIAG][0][0] < NO_DIAG < M[NO_DIAG][0][-1]
            assert ONE_INSIDE in M[ONE_INSIDE][0] and M[ONE_INSIDE][0][0] < ONE_INSIDE < M[ONE_INSIDE][0][-1]
        new, dh, terms, st = references[sigma]
        print(sigma, st, "terms", len(terms))
        assert st["underflow"] == 0
        assert st["t_cancelled"] >= 2 and st["o_cancelled"] >= 1 and st["u_cancelled"] == 2 == st["o_is_one"], st
        for m in "tou":
            assert st[m + "_only_a"] > 0 and st[m + "_only_b"] > 0, (m, st)
        assert st["d1_lacks_diagonal"] >= 4
        for j in (ONE_INSIDE, ONE_AT_END):
            assert new[j][1][new[j][0] == j][0] == 1.0 and j not in dh[j][0]
        assert dh[ONE_AT_END][0][-1] < ONE_AT_END == new[ONE_AT_END][0][-1]
        for j in (NO_DIAG, BELOW, ABOVE, 40):
            assert (j not in new or j not in new[j][0]) and dh[j][1][dh[j][0] == j][0] == 1.0
        assert 25 not in new[21][0] and new[20][1][new[20][0] == 25][0] == -1.0 * 2.0 * sigma * 0.0417 and 33 not in new[30][0]
        assert len(terms) > 1000
    assert np.any(operands[SIGMAS[1]][3][31][1] == 0.0) and not any(np.any(v == 0.0) for _, v in operands[SIGMAS[0]][3].values())


def _vocabulary(nt, M1, MB, MC, MW, sigma):
    """the calls of solvers.cpp solver_hpcp around its products, through the C ABI on compressed columns"""
    I = nt.Matrix_ps(N)
    I.FillIdentity()
    D = nt.Matrix_ps(M1)
    D.Increment(MC, 2.0, 0.0)
    D.Increment(MB, -1.0 * 2.0 * sigma, 0.0)
    e = D.Dot(MW)
    DH = nt.Matrix_ps(D)
    nt.increment_identity(I, DH, -1.0)
    DH.Scale(-1.0)
    return D, DH, e


@pytest.mark.parametrize("sigma", SIGMAS)
def test_update_bit_for_bit(nt, fma, operands, references, sigma):
    D1, DDH, D2DH, WH = operands[sigma]
    w1, w2, terms, _ = references[sigma]
    want = [_triplets(w1), _triplets(w2)]
    Ms = [_matrix(nt, c) for c in (D1, DDH, D2DH, WH)]
    before = [srt(m.triplets()) for m in Ms]
    # (i) the vocabulary on compressed columns against (ii) the restatement
    nt.set_option("slab_algebra", 0)
    V1, V2, ev = _vocabulary(nt, *Ms, sigma)
    nt.set_option("slab_algebra", 1)
    for V, w in zip((V1, V2), want):
        assert same(srt(V.triplets()), w), "compressed columns against the restatement"
    # the fused update
    O1, O2 = nt.Matrix_ps(N), nt.Matrix_ps(N)
    c0, s0 = nt.hpcp_step_counts(), nt.slab_algebra_counts()
    with nt.solver_session(False):
        e = nt.hpcp_update_step(Ms[0], Ms[1], Ms[2], sigma, Ms[3], O1, O2)
    c1, s1 = nt.hpcp_step_counts(), nt.slab_algebra_counts()
    assert e is not None
    assert {k: c1[k] - c0[k] for k in c1} == dict(traces=0, updates=1, refused=0)
    assert s1["merges"] - s0["merges"] == 4 and s1["others"] - s0["others"] == 2 and s1["refusals"] == s0["refusals"]
    for m, b in zip(Ms, before):
        assert same(srt(m.triplets()), b), "the operands are as they were"
    for g, w, V, name in zip((srt(O1.triplets()), srt(O2.triplets())), want, (V1, V2), ("the new D1", "DH")):
        print(sigma, name, "entries", len(w[2]))
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), name + ": pattern"
        assert same(g, w), name + ": values against the restatement"
        assert same(g, srt(V.triplets())), name + ": values against compressed columns"
    # the energy: any summation order of the m rounded products is within m u sum |o wh| of their exact sum
    exact, bound = math.fsum(terms), len(terms) * 2.0 ** -53 * math.fsum(np.abs(terms))
    print(sigma, "energy", e, "exact", exact, "|difference|", abs(e - exact), "bound", bound, "compressed columns", ev)
    assert abs(e - exact) <= bound
    assert abs(ev - exact) <= bound


# ------------------------------------------------------------------ refusals
def test_refusals_leave_everything_as_it_was(nt, fma):
    n, j = 4099, 5
    col = lambda f, l, v=None: {j: (np.arange(f, l + 1), np.linspace(0.1, 0.9, l - f + 1) if v is None else v)}

    def refused(M1, MB, MC, MW, sigma):
        O1, O2 = nt.Matrix_ps(n), nt.Matrix_ps(n)
        before = [srt(m.triplets()) for m in (M1, MB, MC, MW)]
        c0, s0 = nt.hpcp_step_counts(), nt.slab_algebra_counts()
        with nt.solver_session(False):
            e = nt.hpcp_update_step(M1, MB, MC, sigma, MW, O1, O2)
        c1, s1 = nt.hpcp_step_counts(), nt.slab_algebra_counts()
        assert e is None
        assert c1 == dict(c0, refused=c0["refused"] + 1), (c0, c1)
        assert s1 == s0, (s0, s1)   # (a refused update is no operation and no refusal of the session)
        for m, b in zip((M1, MB, MC, MW), before):
            assert same(srt(m.triplets()), b)
        assert len(O1.triplets()[2]) == 0 and len(O2.triplets()[2]) == 0

    M1, near, mid, MW = (_matrix(nt, col(0, 9), n=n), _matrix(nt, col(4, 20), n=n), _matrix(nt, col(2, 12), n=n), _matrix(nt, col(0, 30), n=n))
    far = _matrix(nt, col(n // 2 + 1, n // 2 + 11), n=n)
    # two runs n / 2 rows apart in one column, in either product: the hull is beyond what the column's slots bound
    refused(M1, far, mid, MW, 0.375)
    refused(M1, mid, far, MW, 0.375)
    # sigma zero or not finite: refused before anything is launched
    refused(M1, near, mid, MW, 0.0)
    refused(M1, near, mid, MW, float("nan"))
    refused(M1, near, mid, MW, float("inf"))
    # (-2 x 1e-300) x 1e-30 rounds to zero: an underflow
    tiny = _matrix(nt, col(4, 20, np.full(17, 1e-30)), n=n)
    refused(M1, tiny, mid, MW, 1e-300)
    # the same column with the runs side by side is taken
    O1, O2 = nt.Matrix_ps(n), nt.Matrix_ps(n)
    with nt.solver_session(False):
        e = nt.hpcp_update_step(M1, near, mid, 0.375, MW, O1, O2)
    assert e is not None
    a, b, c = np.zeros(21), np.zeros(21), np.zeros(21)   # (adding an absent entry as +0.0 gives the merges' values)
    a[0:10], b[4:21], c[2:13] = np.linspace(0.1, 0.9, 10), np.linspace(0.1, 0.9, 17), np.linspace(0.1, 0.9, 11)
    o = (a + 2.0 * c) + (-1.0 * 2.0 * 0.375) * b
    assert np.all(o != 0.0) and o[j] != 1.0
    cc, rr, vv = srt(O1.triplets())
    assert np.all(cc == j + 1) and np.array_equal(rr, np.arange(1, 22)) and np.array_equal(vv, o)
    cc, rr, vv = srt(O2.triplets())
    col_j = cc == j + 1
    d = np.zeros(21)
    d[j] = 1.0
    assert np.array_equal(rr[col_j], np.arange(1, 22)) and np.array_equal(vv[col_j], -1.0 * (o + -1.0 * d))
    assert (~col_j).sum() == n - 1 and np.array_equal(cc[~col_j], rr[~col_j]) and np.all(vv[~col_j] == 1.0)   # (+1 on every other diagonal)


# ------------------------------------------------------------------ the solver
SOLVE = (4096, 20, 1e-8, 12)   # the configuration of test_gpu_slab_algebra.py test_other_purification_loops_in_slab_form


def hpcp_solve(nt, H, n, iters=SOLVE[3], thr=SOLVE[2]):
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    p = nt.SolverParameters()
    p.SetThreshold(thr)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(iters)
    p.SetMonitorConvergence(False)
    K = nt.Matrix_ps(n)
    c0, s0 = nt.hpcp_step_counts(), nt.slab_algebra_counts()
    e, mu = nt.DensityMatrixSolvers.HPCP(H, I, n / 2.0, K, p)
    c1, s1 = nt.hpcp_step_counts(), nt.slab_algebra_counts()
    tr = nt.solver_trace()
    return dict(out=srt(K.triplets()), e=e, mu=mu, iters=tr["iterations"], sigma=np.asarray(tr["sigma"]).copy(), nnz=np.asarray(tr["nnz"]).copy(),
                energy=np.asarray(tr["energy"]).copy(), step={k: c1[k] - c0[k] for k in c1}, refusals=s1["refusals"] - s0["refusals"])


@pytest.fixture(scope="module")
def hamiltonian(nt):
    n, h = SOLVE[0], SOLVE[1]
    return nt.Matrix_ps.from_triplets(n, *banded_triplets(n, h)), n


def test_solver_option_1_against_option_0(nt, fma, hamiltonian):
    """the traces keep their bits, the update its values and patterns, and the energy never enters the iterate: sigma, the entry
    counts and the density are those of option 0 bit for bit; the energies, summed in another order, to 1e-10 relative"""
    H, n = hamiltonian
    nt.set_option("hpcp_step", 0)
    off = hpcp_solve(nt, H, n)
    nt.set_option("hpcp_step", 1)
    on = hpcp_solve(nt, H, n)
    print("iterations", on["iters"], "step", on["step"], "refusals", on["refusals"], off["refusals"])
    print("max relative energy difference", float(np.max(np.abs(on["energy"] - off["energy"]) / np.abs(off["energy"]))))
    assert off["step"] == dict(traces=0, updates=0, refused=0)
    assert on["iters"] == off["iters"] == SOLVE[3]
    assert np.array_equal(on["sigma"], off["sigma"]), "sigma, bit for bit"
    assert np.array_equal(on["nnz"], off["nnz"])
    assert same(on["out"], off["out"]), "density triplets, bit for bit"
    assert np.all(np.abs(on["energy"] - off["energy"]) <= 1e-10 * np.abs(off["energy"]))
    assert abs(on["e"] - off["e"]) <= 1e-10 * abs(off["e"]) and on["mu"] == off["mu"]
    assert on["step"]["updates"] >= on["iters"] - 1 and on["step"]["refused"] == 0, on["step"]
    assert on["step"]["traces"] >= on["iters"] - 1, on["step"]
    assert on["refusals"] <= off["refusals"]


def test_gates(nt, fma, hamiltonian):
    """the option at 0, slab_algebra = 0 and a complex Hamiltonian fuse nothing and refuse nothing: the results of option 0"""
    none = dict(traces=0, updates=0, refused=0)
    H, n = hamiltonian
    iters = 4
    nt.set_option("hpcp_step", 0)
    want = hpcp_solve(nt, H, n, iters)
    assert want["step"] == none
    nt.set_option("hpcp_step", 1)
    nt.set_option("slab_algebra", 0)
    a = hpcp_solve(nt, H, n, iters)
    nt.set_option("hpcp_step", 0)
    want_a = hpcp_solve(nt, H, n, iters)
    nt.set_option("slab_algebra", 1)
    nt.set_option("hpcp_step", 1)
    assert a["step"] == none == want_a["step"]
    assert a["iters"] == want_a["iters"] and same(a["out"], want_a["out"]) and np.array_equal(a["sigma"], want_a["sigma"])
    assert np.array_equal(a["energy"], want_a["energy"])
    nc, hc = 1024, 12
    Hc = nt.Matrix_ps.from_triplets(nc, *banded_triplets(nc, hc, complex_=True))
    c = hpcp_solve(nt, Hc, nc, iters)
    nt.set_option("hpcp_step", 0)
    d = hpcp_solve(nt, Hc, nc, iters)
    nt.set_option("hpcp_step", 1)
    assert c["step"] == none == d["step"]
    assert c["iters"] == d["iters"] and same(c["out"], d["out"]) and np.array_equal(c["sigma"], d["sigma"]) and np.array_equal(c["energy"], d["energy"])


# ------------------------------------------------------------------ two ranks
def run_world(world, tmp_path):
    out = str(tmp_path / ("hpcp%d" % world))
    name = "h%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name, NTPOLY_AMD_SHM_MB="64",
                   NTPOLY_AMD_SPGEMM_FMA="1")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "hpcp_step_worker.py"), out],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
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
    return [dict(np.load(out + ".%d.npz" % r)) for r in range(world)]


def test_two_ranks_option_1_against_option_0(tmp_path):
    """HPCP of a real band, n = 4096, as column panels on two ranks sharing one GPU (shared-memory transport, FMA arithmetic), option
    1 against option 0 in the same processes: the same iteration count, sigma bit for bit (one reduction carries both traces,
    element by element what two carry), the gathered density bit for bit, fused updates on both ranks"""
    two = run_world(2, tmp_path)
    for r, p in enumerate(two):
        print("rank", r, "iterations", int(p["iters_on"][0]), "counts (traces, updates, refused)", p["counts_on"].tolist(), p["counts_off"].tolist())
        assert int(p["iters_on"][0]) == int(p["iters_off"][0]) == 12
        assert np.array_equal(p["sigma_on"], p["sigma_off"]), "sigma, bit for bit"
        assert p["counts_off"].tolist() == [0, 0, 0]
        assert p["counts_on"][1] >= 11 and p["counts_on"][0] >= 11 and p["counts_on"][2] == 0, (r, p["counts_on"])
    for k in ("col", "row", "val"):
        assert np.array_equal(np.concatenate([p[k + "_on"] for p in two]), np.concatenate([p[k + "_off"] for p in two])), k
    assert len(np.concatenate([p["val_on"] for p in two])) > 4096
    assert np.array_equal(two[0]["sigma_on"], two[1]["sigma_on"])
