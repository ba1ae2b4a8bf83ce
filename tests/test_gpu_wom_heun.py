"""GPU: the tail of a Heun trial of the WOM solvers in one pass, and the canonical step's two dots in one kernel (option wom_session
= 2; csrc/wom_heun.hip k_wom_heun / k_wom_c_dots, engine.hpp ps_wom_heun / ps_wom_c_dots).  Between its products a trial builds, with
the vocabulary at the solver's threshold, RK2 = W; RK2 += c K0; RK2 += c K1 (c = h * 0.5), err = MatrixNorm(RK1 - RK2) and, once
accepted, err2 = MatrixNorm(RK2 - W).  The fused pass reads the four runs once, writes RK2 and returns both norms.

The kernel is reached with crafted operands through nt.wom_heun_step / nt.wom_c_dots and compared with (i) the same vocabulary calls
on compressed columns (slab_algebra = 0) and (ii) a numpy restatement of AddSparseVectors.f90 WITH its threshold written here --
never with the fused code itself.  numpy's float64 products and sums are the correctly rounded ones the kernel spells as __dmul_rn
/ __dadd_rn, so patterns are compared for equality and values with np.array_equal.  The norms are held to the bits of MatrixNorm on
the restated differences in slab form: they set the next step size."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 1100   # (not a multiple of the 4 waves of a workgroup)
STEPS = (0.5, 0.3125)   # c = 0.25 and 0.15625: short binary fractions, which the planted cancellations need
THR = 1e-8
NONE = dict(solves=0, heun_passes=0, c_dot_passes=0, refused=0)
OPS = ("W", "K0", "K1", "RK1")


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
    nt.set_option("wom_session", 2)
    yield request.param
    nt.set_option("spgemm_fma", 0)
    nt.set_option("slab_algebra", 1)
    nt.set_option("wom_session", 0)


def srt(t):
    c, r, v = t
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def same(a, b):
    """sorted triplets: equal patterns, equal values"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------ operands
# a column is (rows, values), rows 0-based
EMPTY = {"W": {7, 40}, "K0": {8, 40}, "K1": {9, 40}}   # empty in each operand in turn, column 40 in all of them
SUM_DROPPED = 30     # row ROW: w + c k0 is 2^-30 <= thr, dropped (both present, under both extents)
ONE_UNDER = 31       # row ROW: K1 alone holds 1e-12 under M1's extent: dropped
ONE_BEYOND = 32      # K1 alone holds 1e-12 one row beyond M1's last row: kept unfiltered
CHAIN = 33           # W and K0 both end at row l with w + c k0 == 0, K1 holds 1e-12 at l: exh(M1) < l, so RK2 keeps it
EQUAL = 34           # W, K0, K1 are such that RK1 == RK2 everywhere: D1's column is empty
LONG = 600           # the hull of the column spans more than 1024 rows
ROW = 36
SPECIAL = (SUM_DROPPED, ONE_UNDER, ONE_BEYOND, CHAIN, EQUAL, LONG)


def _runs(rng, n, empty):
    """{column: (rows, values)}: a run around the diagonal with half-widths 6..90 drawn per side, ~12 % holes inside, values
    log-uniform in [1e-6, 1] with a random sign"""
    cols = {}
    for j in range(n):
        if j in empty:
            continue
        f, l = max(0, j - int(rng.integers(6, 91))), min(n - 1, j + int(rng.integers(6, 91)))
        rows = np.arange(f, l + 1)
        keep = rng.random(len(rows)) > 0.12
        keep[0] = keep[-1] = True
        rows = rows[keep]
        cols[j] = (rows, 10.0 ** rng.uniform(-6.0, 0.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows)))
    return cols


def _col(f, l, v):
    return np.arange(f, l + 1), np.full(l - f + 1, v, dtype=np.float64)


def _set(cols, j, r, v):
    rows, vals = cols[j]
    if r in rows:
        vals[rows == r] = v
    else:
        k = int(np.searchsorted(rows, r))
        cols[j] = (np.insert(rows, k, r), np.insert(vals, k, v))


def _plant(W, K0, K1, h):
    """the special columns: dense short runs of round numbers, every cancellation exact by construction and checked in numpy"""
    c = h * 0.5
    # both present, the sum 2^-30 <= thr
    W[SUM_DROPPED], K0[SUM_DROPPED], K1[SUM_DROPPED] = _col(20, 50, 0.5), _col(20, 50, 0.25), _col(20, 50, 0.125)
    w = 2.0 ** -30 - c * 0.25
    assert w + c * 0.25 == 2.0 ** -30 and 2.0 ** -30 <= THR
    _set(W, SUM_DROPPED, ROW, w)
    # one-sided under the other operand's extent: W and K0 have a hole at ROW, K1 holds 1e-12 there
    for M in (W, K0):
        rows = np.array([r for r in range(20, 51) if r != ROW])
        M[ONE_UNDER] = (rows, np.full(len(rows), 0.5))
    K1[ONE_UNDER] = _col(20, 50, 0.125)
    _set(K1, ONE_UNDER, ROW, 1e-12)
    # one-sided beyond: W and K0 end at 50, K1 goes on to 51 with 1e-12
    W[ONE_BEYOND], K0[ONE_BEYOND], K1[ONE_BEYOND] = _col(20, 50, 0.5), _col(20, 50, 0.25), _col(20, 51, 0.125)
    _set(K1, ONE_BEYOND, 51, 1e-12)
    # the chain case: w + c k0 == 0 at the last row l = 50 of both, K1 holds 1e-12 there and ends there
    W[CHAIN], K0[CHAIN], K1[CHAIN] = _col(20, 50, 0.5), _col(20, 50, 0.25), _col(20, 50, 0.125)
    # (0.5 and -2.0 at c = 0.25; spelled from c so that the second step size cancels as exactly)
    w, k0 = 0.5, -0.5 / c if c == 0.25 else None
    if k0 is None:
        w, k0 = -(c * 0.25), 0.25
    assert w + c * k0 == 0.0 and c * k0 != 0.0
    _set(W, CHAIN, 50, w)
    _set(K0, CHAIN, 50, k0)
    _set(K1, CHAIN, 50, 1e-12)
    # RK1 == RK2: K1 == K0, so W + h K0 == (W + c K0) + c K0 where these round numbers add exactly
    W[EQUAL], K0[EQUAL], K1[EQUAL] = _col(20, 50, 0.5), _col(20, 50, 0.25), _col(20, 50, 0.25)
    assert 0.5 + h * 0.25 == (0.5 + c * 0.25) + c * 0.25
    # a hull of more than 1024 rows: three runs of 400 rows side by side.  At the first step size small round values, so that the
    # largest column sums of D1 and D2 -- the norms -- come from an ordinary column, held in registers; at the second values in
    # [0.5, 1) with random signs, so that they come from this column, which is swept from memory, and depend on the order of its sum
    if h == STEPS[0]:
        W[LONG], K0[LONG], K1[LONG] = _col(0, 399, 2.0 ** -7), _col(350, 749, 2.0 ** -8), _col(700, 1099, 2.0 ** -9)
    else:
        rng = np.random.default_rng(600)
        for M, f in ((W, 0), (K0, 350), (K1, 700)):
            M[LONG] = (np.arange(f, f + 400), rng.uniform(0.5, 1.0, 400) * rng.choice([-1.0, 1.0], 400))


@pytest.fixture(scope="module")
def operands():
    out = {}
    for h in STEPS:
        rng = np.random.default_rng(20261020)
        W, K0, K1 = (_runs(rng, N, EMPTY[k]) for k in ("W", "K0", "K1"))
        _plant(W, K0, K1, h)
        out[h] = (W, K0, K1)
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


# ------------------------------------------------------------------ AddSparseVectors.f90 with its threshold, restated
EMPTY_COL = (np.zeros(0, dtype=np.int64), np.zeros(0))


def add_sparse(a, alpha, b, thr, stats, tag):
    """alpha a + b on sorted sparse vectors (rows, values), the scaled value rounded, then added: inside the overlap of the two
    lists an entry is kept iff |value| > thr, beyond the end of one list the tail of the other is copied unfiltered"""
    (ra, va), (rb, vb) = a, b
    if len(ra) == 0 and len(rb) == 0:
        return EMPTY_COL
    rows = np.union1d(ra, rb)
    ia, ib = np.isin(rows, ra), np.isin(rows, rb)
    wa, wb = np.zeros(len(rows)), np.zeros(len(rows))
    wa[ia] = alpha * va
    wb[ib] = vb
    s = np.where(ia & ib, wa + wb, np.where(ia, wa, wb))
    lim = min(ra[-1] if len(ra) else -1, rb[-1] if len(rb) else -1)
    big = np.abs(s) > thr
    keep = (rows > lim) | big
    for name, mask in (("both_kept", ia & ib & big), ("both_dropped", ia & ib & ~big), ("one_under_dropped", (ia ^ ib) & (rows <= lim) & ~big),
                       ("one_beyond_small_kept", (ia ^ ib) & (rows > lim) & ~big), ("one_kept", (ia ^ ib) & keep)):
        stats[tag + "_" + name] = stats.get(tag + "_" + name, 0) + int(mask.sum())
    stats["kept_zero"] = stats.get("kept_zero", 0) + int((keep & (s == 0.0)).sum())
    return rows[keep], s[keep]


def heun_tail(W, K0, K1, RK1, h, thr, n=N):
    """RK2, D1, D2 column by column as solver_wom's vocabulary calls build them, and branch statistics"""
    c = h * 0.5
    st, rk2, d1, d2 = {}, {}, {}, {}
    for j in range(n):
        w, k0, k1, r1 = (M.get(j, EMPTY_COL) for M in (W, K0, K1, RK1))
        m1 = add_sparse(k0, c, w, thr, st, "m1")        # CopyMatrix(W, RK2); IncrementMatrix(K0, RK2, c, thr)
        o = add_sparse(k1, c, m1, thr, st, "rk2")       # IncrementMatrix(K1, RK2, c, thr)
        e1 = add_sparse(o, -1.0, r1, thr, st, "d1")     # CopyMatrix(RK1, Temp); IncrementMatrix(RK2, Temp, -1, thr)
        e2 = add_sparse(w, -1.0, o, thr, st, "d2")      # CopyMatrix(RK2, Temp); IncrementMatrix(W, Temp, -1, thr)
        for dst, v in ((rk2, o), (d1, e1), (d2, e2)):
            if len(v[0]):
                dst[j] = v
        st.setdefault("exh_m1", {})[j] = int(m1[0][-1]) if len(m1[0]) else -1
    return rk2, d1, d2, st


def rk1_of(W, K0, h, thr, n=N):
    """CopyMatrix(K0, RK1); ScaleMatrix(RK1, h); IncrementMatrix(W, RK1, 1, thr), restated (the tests build RK1 with the vocabulary
    itself and hold it to this)"""
    out, st = {}, {}
    for j in range(n):
        k0 = K0.get(j, EMPTY_COL)
        o = add_sparse(W.get(j, EMPTY_COL), 1.0, (k0[0], h * k0[1]), thr, st, "rk1")
        if len(o[0]):
            out[j] = o
    return out


@pytest.fixture(scope="module")
def references(operands):
    out = {}
    for h in STEPS:
        W, K0, K1 = operands[h]
        RK1 = rk1_of(W, K0, h, THR)
        out[h] = (RK1,) + heun_tail(W, K0, K1, RK1, h, THR)
    return out


def test_the_inputs_reach_every_branch(operands, references):
    """from the operands and the numpy restatement alone"""
    import ntpoly_amd as nt
    bound = nt.wom_heun_register_rows()
    for h in STEPS:
        W, K0, K1 = operands[h]
        RK1, rk2, d1, d2, st = references[h]
        print(h, {k: v for k, v in st.items() if k != "exh_m1"})
        assert 7 not in W and 7 in K0 and 7 in K1 and 8 not in K0 and 8 in W and 9 not in K1 and 9 in W
        assert all(40 not in M for M in (W, K0, K1)) and 40 not in rk2 and 40 not in RK1
        assert all(0 in M and N - 1 in M for M in (W, K0, K1)) and 0 in rk2 and N - 1 in rk2
        assert st["kept_zero"] == 0, "no kept value is exactly zero (the runs could not hold it)"
        for tag in ("m1", "rk2", "d1", "d2"):
            assert st[tag + "_both_kept"] > 1000 and st[tag + "_one_kept"] > 0, (tag, st)
        # a both-present sum <= thr, dropped: row ROW of M1 in column SUM_DROPPED (RK2 then takes c k1 alone there, under M1's extent)
        assert st["m1_both_dropped"] >= 1 and st["rk2_both_dropped"] + st["m1_both_dropped"] >= 1
        assert ROW in rk2[SUM_DROPPED][0] and rk2[SUM_DROPPED][1][rk2[SUM_DROPPED][0] == ROW][0] == (h * 0.5) * 0.125
        # a one-sided entry <= thr under the other operand's extent, dropped; one beyond it, kept
        assert st["rk2_one_under_dropped"] >= 1 and ROW not in rk2[ONE_UNDER][0] and rk2[ONE_UNDER][0][-1] == 50
        assert st["rk2_one_beyond_small_kept"] >= 2
        assert rk2[ONE_BEYOND][0][-1] == 51 and rk2[ONE_BEYOND][1][-1] == (h * 0.5) * 1e-12
        # THE CHAIN CASE: both inputs of M1 end at row 50, M1 ends below it, and RK2 keeps K1's 1e-12 at row 50
        assert W[CHAIN][0][-1] == K0[CHAIN][0][-1] == K1[CHAIN][0][-1] == 50 and st["exh_m1"][CHAIN] == 49
        assert rk2[CHAIN][0][-1] == 50 and rk2[CHAIN][1][-1] == (h * 0.5) * 1e-12 and abs(rk2[CHAIN][1][-1]) <= THR
        # RK1 == RK2 in a whole column: D1's column is empty, D2's is not
        assert EQUAL in rk2 and EQUAL not in d1 and EQUAL in d2
        assert np.array_equal(RK1[EQUAL][0], rk2[EQUAL][0]) and np.array_equal(RK1[EQUAL][1], rk2[EQUAL][1])
        # a hull beyond the kernel's register bound, and every other column within it: both of its paths run
        hull = lambda j: max(M[j][0][-1] for M in (W, K0, K1, RK1) if j in M) - min(M[j][0][0] for M in (W, K0, K1, RK1) if j in M) + 1
        assert hull(LONG) > 1024 >= bound, (hull(LONG), bound)
        assert max(hull(j) for j in range(N) if j != LONG and j != 40) + 64 <= bound
        assert len(d1) > 1000 and len(d2) > 1000
        # the norms: from an ordinary column (registers) at the first step size, from the long one (memory) at the second, and in
        # both a sum of many different magnitudes, which depends on its order
        for D in (d1, d2):
            top = max(D, key=lambda j: math.fsum(np.abs(D[j][1])))
            print(h, "the largest column sum is column", top, "with", len(D[top][0]), "entries")
            assert (top == LONG) == (h == STEPS[1]) and (top not in SPECIAL or top == LONG) and len(D[top][0]) > 64
            assert len(np.unique(np.abs(D[top][1]))) > 64


def _vocabulary(nt, MW, MK0, MK1, MRK1, h, thr):
    """the calls of solvers_extra.cpp solver_wom behind the trial's products, through the C ABI"""
    RK2 = nt.Matrix_ps(MW)
    RK2.Increment(MK0, h * 0.5, thr)
    RK2.Increment(MK1, h * 0.5, thr)
    T1 = nt.Matrix_ps(MRK1)
    T1.Increment(RK2, -1.0, thr)
    T2 = nt.Matrix_ps(RK2)
    T2.Increment(MW, -1.0, thr)
    return RK2, T1, T2


def _rk1_vocabulary(nt, MW, MK0, h, thr):
    R = nt.Matrix_ps(MK0)
    R.Scale(h)
    R.Increment(MW, 1.0, thr)
    return R


def _dot_in_session(nt, A, B):
    """DotMatrix through the C ABI alone (host.py's Dot first asks whether the matrices are complex, an entry point that packs
    them): inside a session it leaves both operands in slab form"""
    v = C.c_double()
    nt.lib.DotMatrix_psr_wrp(A.ih, B.ih, C.byref(v))
    return v.value


def _norm_in_session(nt, A):
    nt.lib.MatrixNorm_ps_wrp.restype = C.c_double
    return float(nt.lib.MatrixNorm_ps_wrp(A.ih))


def _column_sums(cols):
    """per column (the exact sum of moduli, the any-order bound m 2^-52 sum |t|)"""
    return [(math.fsum(np.abs(v)), len(v) * 2.0 ** -52 * math.fsum(np.abs(v))) for _, v in cols.values()]


def _norm_within_bound(got, cols):
    """got lies within the any-order bound of the exact maximum column sum: max is monotone, so |max_j s_j - max_j e_j| <= max_j b_j"""
    sums = _column_sums(cols)
    if not sums:
        return got == 0.0
    return abs(got - max(s for s, _ in sums)) <= max(b for _, b in sums)


@pytest.mark.parametrize("h", STEPS)
def test_heun_tail_bit_for_bit(nt, fma, operands, references, h):
    W, K0, K1 = operands[h]
    RK1, rk2, d1, d2, _ = references[h]
    want = _triplets(rk2)
    MW, MK0, MK1 = (_matrix(nt, c) for c in (W, K0, K1))
    # RK1 by the vocabulary on compressed columns, held to its restatement; (i) the vocabulary against (ii) the restatement
    nt.set_option("slab_algebra", 0)
    MRK1 = _rk1_vocabulary(nt, MW, MK0, h, THR)
    V, VT1, VT2 = _vocabulary(nt, MW, MK0, MK1, MRK1, h, THR)
    ev, ev2 = VT1.Norm(), VT2.Norm()
    nt.set_option("slab_algebra", 1)
    assert same(srt(MRK1.triplets()), _triplets(RK1)), "RK1: compressed columns against the restatement"
    assert same(srt(V.triplets()), want), "RK2: compressed columns against the restatement"
    assert same(srt(VT1.triplets()), _triplets(d1)) and same(srt(VT2.triplets()), _triplets(d2)), "the differences likewise"
    Ms = [MW, MK0, MK1, MRK1]
    before = [srt(m.triplets()) for m in Ms]
    # the fused pass; then, in the same session, MatrixNorm of the restated differences in slab form (a dot with W, which the pass
    # has left in slab form, brings them there)
    O, MD1, MD2 = nt.Matrix_ps(N), _matrix(nt, d1), _matrix(nt, d2)
    c0, s0 = nt.wom_session_counts(), nt.slab_algebra_counts()
    with nt.solver_session(False):
        got = nt.wom_heun_step(MW, MK0, MK1, MRK1, h, THR, O)
        c1, s1 = nt.wom_session_counts(), nt.slab_algebra_counts()
        _dot_in_session(nt, MD1, MW)
        _dot_in_session(nt, MD2, MW)
        s2 = nt.slab_algebra_counts()
        n1, n2 = _norm_in_session(nt, MD1), _norm_in_session(nt, MD2)
        s3 = nt.slab_algebra_counts()
    print(h, "counts", c0, c1, "slab algebra", s0, s1, s2, s3)
    assert got is not None
    err, err2 = got
    assert {k: c1[k] - c0[k] for k in c1} == dict(solves=0, heun_passes=1, c_dot_passes=0, refused=0)
    assert s1["merges"] - s0["merges"] == 7 and s1["others"] - s0["others"] == 2 and s1["refusals"] == s0["refusals"]
    assert s2["others"] - s1["others"] == 2 and s3["others"] - s2["others"] == 2 and s3["refusals"] == s0["refusals"], "the norms were taken in slab form"
    for m, bf in zip(Ms, before):
        assert same(srt(m.triplets()), bf), "the operands are as they were"
    g = srt(O.triplets())
    print(h, "entries", len(want[2]))
    assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]), "pattern"
    assert same(g, want), "values against the restatement"
    assert same(g, srt(V.triplets())), "values against compressed columns"
    print(h, "err", err, "MatrixNorm in slab form", n1, "compressed columns", ev, "err2", err2, "MatrixNorm in slab form", n2, "compressed columns", ev2)
    assert err == n1 and err2 == n2, "the bits of MatrixNorm on the differences in slab form"
    assert _norm_within_bound(err, d1) and _norm_within_bound(err2, d2)
    assert _norm_within_bound(ev, d1) and _norm_within_bound(ev2, d2)


@pytest.mark.parametrize("h", STEPS)
def test_c_dots_bit_for_bit(nt, fma, operands, h):
    """dot(X, W) and dot(W, XA) from one kernel: the bits of two DotMatrix calls on the same pairs in the same session"""
    X, Wm, XA = operands[h]   # (three matrices with empty columns in turn: any three serve)
    MX, MW, MXA = (_matrix(nt, c) for c in (X, Wm, XA))
    before = [srt(m.triplets()) for m in (MX, MW, MXA)]
    c0, s0 = nt.wom_session_counts(), nt.slab_algebra_counts()
    with nt.solver_session(False):
        got = nt.wom_c_dots(MX, MW, MXA)
        c1, s1 = nt.wom_session_counts(), nt.slab_algebra_counts()
        want = (_dot_in_session(nt, MX, MW), _dot_in_session(nt, MW, MXA))
        s2 = nt.slab_algebra_counts()
    assert got is not None
    print(h, "dots", got, "DotMatrix in the session", want)
    assert {k: c1[k] - c0[k] for k in c1} == dict(solves=0, heun_passes=0, c_dot_passes=1, refused=0)
    assert s1["others"] - s0["others"] == 2 and s1["merges"] == s0["merges"] and s1["refusals"] == s0["refusals"]
    assert s2["others"] - s1["others"] == 2 and s2["refusals"] == s0["refusals"], "the dots were taken in slab form"
    assert got[0] == want[0] and got[1] == want[1]
    for m, bf in zip((MX, MW, MXA), before):
        assert same(srt(m.triplets()), bf), "the operands are as they were"
    for value, (A, B) in zip(got, ((X, Wm), (Wm, XA))):
        terms = []
        for j in range(N):
            a, b = A.get(j, EMPTY_COL), B.get(j, EMPTY_COL)
            both = np.intersect1d(a[0], b[0])
            terms.append(a[1][np.isin(a[0], both)] * b[1][np.isin(b[0], both)])
        terms = np.concatenate(terms)
        exact, bound = math.fsum(terms), len(terms) * 2.0 ** -52 * math.fsum(np.abs(terms))
        print(h, "dot", value, "exact", exact, "|difference|", abs(value - exact), "bound", bound)
        assert len(terms) > 1000 and abs(value - exact) <= bound


# ------------------------------------------------------------------ refusals
def test_refusals_leave_everything_as_it_was(nt, fma):
    n, j = 4099, 5
    col = lambda f, l, v=None: {j: (np.arange(f, l + 1), np.linspace(0.1, 0.9, l - f + 1) if v is None else v)}
    h = 0.5

    def refused(MW, MK0, MK1, MRK1, step):
        O = nt.Matrix_ps(n)
        Ms = (MW, MK0, MK1, MRK1)
        before = [srt(m.triplets()) for m in Ms]
        c0, s0 = nt.wom_session_counts(), nt.slab_algebra_counts()
        with nt.solver_session(False):
            got = nt.wom_heun_step(MW, MK0, MK1, MRK1, step, THR, O)
        c1, s1 = nt.wom_session_counts(), nt.slab_algebra_counts()
        assert got is None
        assert c1 == dict(c0, refused=c0["refused"] + 1), (c0, c1)
        assert s1 == s0, (s0, s1)   # (a refused pass is no operation and no refusal of the session)
        for m, bf in zip(Ms, before):
            assert same(srt(m.triplets()), bf)
        assert len(O.triplets()[2]) == 0

    MW, near, near1 = _matrix(nt, col(0, 9), n=n), _matrix(nt, col(4, 20), n=n), _matrix(nt, col(2, 25), n=n)
    MRK1 = _matrix(nt, col(0, 20, np.linspace(2.1, 2.9, 21)), n=n)
    far = _matrix(nt, col(n // 2 + 1, n // 2 + 11), n=n)
    # two runs n / 2 rows apart in one column, either way round: the hull is beyond what the column's slots bound
    refused(MW, far, near1, MRK1, h)
    refused(far, MW, near1, MRK1, h)
    # 1e-300 / 2 x 1e-30 rounds to zero beyond W's last row: an underflowed tail
    tiny = _matrix(nt, col(4, 20, np.full(17, 1e-30)), n=n)
    refused(MW, tiny, near1, MRK1, 1e-300)
    # a step that is not finite: refused before anything is launched
    refused(MW, near, near1, MRK1, float("nan"))
    refused(MW, near, near1, MRK1, float("inf"))
    # the same column with the runs side by side is taken
    O = nt.Matrix_ps(n)
    with nt.solver_session(False):
        got = nt.wom_heun_step(MW, near, near1, MRK1, h, THR, O)
    assert got is not None
    c = h * 0.5
    w, k0, k1, r1 = np.zeros(26), np.zeros(26), np.zeros(26), np.zeros(26)   # (adding an absent entry as +0.0 gives the merge's values)
    w[0:10], k0[4:21], k1[2:26], r1[0:21] = np.linspace(0.1, 0.9, 10), np.linspace(0.1, 0.9, 17), np.linspace(0.1, 0.9, 24), np.linspace(2.1, 2.9, 21)
    o = (w + c * k0) + c * k1
    assert np.all(np.abs(o) > THR) and np.all(np.abs(w + c * k0)[:21] > THR)
    cc, rr, vv = srt(O.triplets())
    assert np.all(cc == j + 1) and np.array_equal(rr, np.arange(1, 27)) and np.array_equal(vv, o)
    e1, e2 = r1 - o, o - w
    assert np.all(np.abs(e1) > THR) and np.all(np.abs(e2)[2:] > THR) and np.all(e2[:2] == 0.0)
    for value, terms in zip(got, (e1, e2)):
        exact, bound = math.fsum(np.abs(terms)), len(terms) * 2.0 ** -52 * math.fsum(np.abs(terms))
        assert abs(value - exact) <= bound
