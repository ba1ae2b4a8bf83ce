"""GPU: PurificationExtrapolate in a slab session (option purify_session; csrc/purify_tail.hip k_purify_tail, engine.hpp
ps_purify_tail).  Behind its two products T = D S and N = T D an iteration calls, with the vocabulary at threshold 0,
    trace_value = dot(D, S);  if trace > trace_value: N *= -1; N += 2 D          (the fold: N' = 2 D - D S D; otherwise N' = D S D)
    D += -N';  norm = ||D||;  D = N'
With the option at 2 everything behind the products is one pass over the runs of D, N and S: it writes N' in the fold branch
(nothing in the plain one) and returns the norm and the NEXT iteration's trace dot(N', S).

The kernel is reached with crafted operands through nt.purify_tail_step and compared with (i) the same vocabulary calls on
compressed columns (slab_algebra = 0) and (ii) a numpy restatement of AddSparseVectors.f90 at threshold 0 written here -- never
with the fused code itself.  numpy's float64 products and sums are the correctly rounded ones the kernel spells as __dmul_rn /
__dadd_rn, so patterns are compared for equality and values with np.array_equal.  The norm ends the loop and the dot decides the
next branch: both are held to the bits of MatrixNorm / DotMatrix on the restated matrices in slab form in the same session."""
import ctypes as C
import math
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from gen import banded_triplets
from golden_util import Golden, to_dense

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 259   # (not a multiple of the 4 waves of a workgroup)
KEYS = ("solves", "fold_passes", "plain_passes", "refused")


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture(params=[1, 0], ids=["fma", "unfused"])
def fma(nt, request):
    """both arithmetic modes: slots padded to the tile kernel's row alignment, and runs packed back to back"""
    default = nt.get_option("purify_session")
    nt.set_option("spgemm_fma", request.param)
    nt.set_option("purify_session", 2)
    yield request.param
    nt.set_option("spgemm_fma", 0)
    nt.set_option("slab_algebra", 1)
    nt.set_option("purify_session", default)


def srt(t):
    c, r, v = t
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def same(a, b):
    """sorted triplets: equal patterns, equal values"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def delta(c0, c1):
    return {k: c1[k] - c0[k] for k in c1}


# ------------------------------------------------------------------ operands
# a column is (rows, values)
EMPTY = {"D": {7, 40}, "N": {8, 40}, "S": {11}}   # empty in each operand in turn, column 40 in D and N
DIAG_ONLY = {13}
BELOW, ABOVE = 60, 150      # columns whose runs lie beyond / before the diagonal row in every operand
CANCEL, ONE_SIDED = 30, 31  # row 33: 2 d - n == 0 exactly; the same d with no N entry there
ROW = 33
ZERO_FIRST = 90             # D and N begin at the same row with the same value: D - N' is exactly zero at the hull's first row


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


def _plant(D, Nm):
    """a cancellation and a zero of the difference, exact by construction and checked here in numpy"""
    d, n = 0.375, 0.75
    assert 2.0 * d + (-n) == 0.0 and 2.0 * d != 0.0
    _set(D, CANCEL, ROW, d)
    _set(Nm, CANCEL, ROW, n)
    # ... and with no N entry there: the row keeps the one-sided 2 d
    _set(D, ONE_SIDED, ROW, d)
    _unset(Nm, ONE_SIDED, ROW)
    # both runs begin at one row with one value x: the fold gives 2 x - x = x there and D - N' = 0 in either branch
    f = int(min(D[ZERO_FIRST][0][0], Nm[ZERO_FIRST][0][0]))
    for M in (D, Nm):
        rows, vals = M[ZERO_FIRST]
        M[ZERO_FIRST] = (rows[rows >= f], vals[rows >= f])
        _set(M, ZERO_FIRST, f, 0.5)
    assert 2.0 * 0.5 + (-0.5) == 0.5 and -1.0 * 0.5 + 0.5 == 0.0
    # ... and this column sets the norm (a maximum over columns): D's other entries there are scaled by 32, an exact factor, so
    # the assertion on the norm's bits sees the one column whose lane rotation is not that of the hull's first row
    rows, vals = D[ZERO_FIRST]
    D[ZERO_FIRST] = (rows, np.where(rows == f, vals, 32.0 * vals))


def _crafted(stored_zero):
    rng = np.random.default_rng(20261021)
    D, Nm, S = (_runs(rng, N, EMPTY[k]) for k in ("D", "N", "S"))
    _plant(D, Nm)
    if stored_zero:
        _set(S, ONE_SIDED, ROW, 0.0)   # (a stored zero: this S enters slab form as a read-only view)
    return D, Nm, S


def _long():
    """columns longer than one trip of the kernel's row loop (256 rows): 5 columns of an n = 700 matrix whose runs span 300 to 640
    rows, offset against each other so that both tails and both heads are one-sided, with holes"""
    n = 700
    rng = np.random.default_rng(20261022)
    out = []
    for shift in (0, 17, 5):
        cols = {}
        for j, (f, l) in {3: (0, 640), 4: (20, 330), 350: (40, 699), 351: (100, 420), 699: (380, 699)}.items():
            f, l = max(0, f + shift), min(n - 1, l - 2 * shift)
            rows = np.arange(f, l + 1)
            keep = rng.random(len(rows)) > 0.12
            keep[0] = keep[-1] = True
            rows = rows[keep]
            cols[j] = (rows, 10.0 ** rng.uniform(-6.0, 0.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows)))
        out.append(cols)
    return tuple(out), n


SETS = ("crafted", "crafted_view", "long")


@pytest.fixture(scope="module")
def operands():
    """{name: ((D, N, S), n)}"""
    long_ops, long_n = _long()
    return {"crafted": (_crafted(False), N), "crafted_view": (_crafted(True), N), "long": (long_ops, long_n)}


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
    stats[tag + "_tail_a"] = stats.get(tag + "_tail_a", 0) + int((ia & (rows > (rb[-1] if len(rb) else -1))).sum())
    stats[tag + "_tail_b"] = stats.get(tag + "_tail_b", 0) + int((ib & (rows > (ra[-1] if len(ra) else -1))).sum())
    stats["underflow"] = stats.get("underflow", 0) + int((~nz & ~(ia & ib)).sum())
    return rows[keep], s[keep]


def restated(D, Nm, S, n, fold):
    """N', the difference D - N', the terms of dot(N', S), the terms of each column's sum of |D - N'|, and branch statistics"""
    empty = (np.zeros(0, dtype=np.int64), np.zeros(0))
    st, new, diff, terms, colterms = {}, {}, {}, [], []
    st["zero_first"] = st["rotated"] = st["dot_rotated"] = 0
    for j in range(n):
        d, m, s = D.get(j, empty), Nm.get(j, empty), S.get(j, empty)
        if fold:
            o = add_sparse(d, 2.0, (m[0], -1.0 * m[1]), 1.0, st, "o")      # ScaleMatrix(N, -1); IncrementMatrix(D, N, 2)
        else:
            o = m
        st["empty_result"] = st.get("empty_result", 0) + int(len(o[0]) == 0)
        if len(o[0]):
            new[j] = o
        e = add_sparse(o, -1.0, d, 1.0, st, "e")                           # IncrementMatrix(N', D, -1)
        if len(e[0]):
            diff[j] = e
        colterms.append(np.abs(e[1]))
        hull = [x[0][0] for x in (d, m) if len(x[0])]
        if hull and (len(e[0]) == 0 or e[0][0] != min(hull)):
            st["zero_first"] += int(len(e[0]) > 0)
        if hull and len(e[0]) and (e[0][0] - min(hull)) % 64:
            st["rotated"] += 1
        both = np.intersect1d(o[0], s[0])
        if hull and len(both) and (max(o[0][0], s[0][0]) - min(hull)) % 64:
            st["dot_rotated"] += 1
        terms.append(o[1][np.isin(o[0], both)] * s[1][np.isin(s[0], both)])
    return new, diff, np.concatenate(terms), colterms, st


def _lane_sum(col, start):
    """the sum of |v| over a column (rows, values) as a wave of 64 lanes forms it: lane t adds the rows start + t + 64 m in ascending
    order, then the butterfly v += v[lane ^ o] for o = 32 .. 1 (the summation order of MatrixNorm on a slab-form column when
    `start` is its first row)"""
    rows, vals = col
    lanes = np.zeros(64)
    for r, v in zip(rows, np.abs(vals)):
        lanes[(r - start) % 64] += v
    o = 32
    while o:
        lanes = lanes + lanes[np.arange(64) ^ o]
        o >>= 1
    return float(lanes[0])


@pytest.fixture(scope="module")
def references(operands):
    return {(name, fold): restated(*operands[name][0], operands[name][1], fold) for name in SETS for fold in (1, 0)}


def test_the_inputs_reach_every_branch(operands, references):
    """from the operands and the numpy restatement alone: columns empty in D, in N, in both and in S, a diagonal-only column, runs
    wholly beyond and before the diagonal row, columns 0 and N - 1, holes inside runs, in the fold both-present sums that are
    kept, one that cancels, one-sided entries from either side and tails beyond the other operand's last row from either side; a
    column whose difference is exactly zero at the hull's first row (the norm's lane rotation is not the trivial one there); no
    kept value is zero; one S stores a zero; the long set has columns of more than 256 rows (more than one trip of the row loop)"""
    for name in ("crafted", "crafted_view"):
        (D, Nm, S), n = operands[name]
        assert n == N and N % 4 != 0
        assert 7 not in D and 7 in Nm and 8 not in Nm and 8 in D and 40 not in D and 40 not in Nm and 40 in S and 11 not in S
        for M in (D, Nm):
            assert 0 in M and N - 1 in M and M[BELOW][0][0] > BELOW and M[ABOVE][0][-1] < ABOVE and list(M[13][0]) == [13]
            holes = sum(int(r[-1] - r[0] + 1 - len(r)) for r, _ in M.values())
            span = sum(int(r[-1] - r[0] + 1) for r, _ in M.values())
            assert 0.08 < holes / span < 0.16, holes / span
        assert ROW in D[CANCEL][0] and ROW in Nm[CANCEL][0] and ROW in D[ONE_SIDED][0] and ROW not in Nm[ONE_SIDED][0]
        assert D[ZERO_FIRST][0][0] == Nm[ZERO_FIRST][0][0] and D[ZERO_FIRST][1][0] == Nm[ZERO_FIRST][1][0] == 0.5
        for fold in (1, 0):
            new, diff, terms, colterms, st = references[(name, fold)]
            print(name, fold, st, "terms", len(terms))
            assert st["underflow"] == 0
            assert st["empty_result"] == (1 if fold else 2) and 40 not in new
            assert diff[ZERO_FIRST][0][0] > D[ZERO_FIRST][0][0] and st["zero_first"] >= 1, "the difference is zero at the hull's first row"
            # the norm is a maximum over columns: THIS column sets it, and by a margin no rounding closes, so the asserted bits are
            # those of the column whose first kept row is not the hull's first row; its rotation (first kept row - the hull's first
            # row aligned down) mod 64 is neither 0 nor what the hull's first row or N''s first row would give, for every alignment
            # of the slots (1 in unfused arithmetic, 16 x the tile rows in FMA arithmetic)
            sums = np.array([math.fsum(t) for t in colterms])
            assert int(np.argmax(sums)) == ZERO_FIRST and sums[ZERO_FIRST] > 1.5 * np.delete(sums, ZERO_FIRST).max(), (int(np.argmax(sums)), sums[ZERO_FIRST])
            f0, df = int(D[ZERO_FIRST][0][0]), int(diff[ZERO_FIRST][0][0])
            assert new[ZERO_FIRST][0][0] == f0 and df > f0
            for al in (1, 2, 4, 8, 16, 32, 64):
                assert (df - f0 // al * al) % 64 != 0 and (df - f0) % 64 != 0, (al, f0, df)
            # (what the lane order can and cannot change: a lane's partial sum is the sum over one residue of the rows mod 64 whatever
            # row the lanes are counted from, and the butterfly joins lanes t and t ^ o, that is the residues mod 2 o, so a cyclic
            # shift of the lanes permutes only the operands of commutative additions -- the same bits from any first row.  The GPU
            # test holds the norm to this restated sum; the kernel's rotation follows MatrixNorm's lane order to the letter)
            assert _lane_sum(diff[ZERO_FIRST], df) == _lane_sum(diff[ZERO_FIRST], f0) == _lane_sum(diff[ZERO_FIRST], 0)
            assert st["rotated"] >= 1 and st["dot_rotated"] > 10
            assert st["e_both_kept"] > 1000 and st["e_cancelled"] == 1 and st["e_only_a"] > 0 and st["e_only_b"] > 0 and st["e_tail_a"] > 0, st
            assert fold or st["e_tail_b"] > 0, st   # (the fold's N' spans both runs: D has no tail beyond it)
            assert len(terms) > 1000
            if fold:
                assert st["o_cancelled"] == 1 and st["o_both_kept"] > 1000 and st["o_only_a"] > 0 and st["o_only_b"] > 0, st
                assert st["o_tail_a"] > 0 and st["o_tail_b"] > 0, st
                assert ROW not in new[CANCEL][0] and new[ONE_SIDED][1][new[ONE_SIDED][0] == ROW][0] == 0.75
                assert new[N - 1][0][-1] == N - 1 and 0 in new
    assert np.any(operands["crafted_view"][0][2][ONE_SIDED][1] == 0.0)
    assert not any(np.any(v == 0.0) for M in operands["crafted"][0] for _, v in M.values())
    (D, Nm, S), n = operands["long"]
    assert max(int(max(D[j][0][-1], Nm[j][0][-1]) - min(D[j][0][0], Nm[j][0][0])) for j in D) > 2 * 256
    assert any(256 < int(max(D[j][0][-1], Nm[j][0][-1]) - min(D[j][0][0], Nm[j][0][0])) < 2 * 256 for j in D)


def _vocabulary(nt, MD, MN, MS, fold):
    """the calls of solvers_extra.cpp purification_extrapolate behind its products, through the C ABI: N', ||D - N'||, dot(N', S)"""
    V = nt.Matrix_ps(MN)
    if fold:
        V.Scale(-1.0)
        V.Increment(MD, 2.0, 0.0)
    T = nt.Matrix_ps(MD)
    T.Increment(V, -1.0, 0.0)
    return V, T.Norm(), V.Dot(MS)


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


@pytest.mark.parametrize("fold", (1, 0), ids=["fold", "plain"])
@pytest.mark.parametrize("name", SETS)
def test_pass_bit_for_bit(nt, fma, operands, references, name, fold):
    (D, Nm, S), n = operands[name]
    new, diff, terms, colterms, _ = references[(name, fold)]
    want = _triplets(new)
    Ms = [_matrix(nt, c, n) for c in (D, Nm, S)]
    before = [srt(m.triplets()) for m in Ms]
    # (i) the vocabulary on compressed columns against (ii) the restatement
    nt.set_option("slab_algebra", 0)
    V, nv, ev = _vocabulary(nt, *Ms, fold)
    nt.set_option("slab_algebra", 1)
    assert same(srt(V.triplets()), want), "compressed columns against the restatement"
    # the fused pass; then, in the same session, DotMatrix of the restated N' with S and MatrixNorm of the restated difference, both
    # in slab form (a dot with S, which the pass has left in slab form, brings a matrix there)
    O, Mn, Md = nt.Matrix_ps(n), _matrix(nt, new, n), _matrix(nt, diff, n)
    c0, s0 = nt.purify_session_counts(), nt.slab_algebra_counts()
    with nt.solver_session(False):
        got = nt.purify_tail_step(Ms[0], Ms[1], Ms[2], fold, O)
        c1, s1 = nt.purify_session_counts(), nt.slab_algebra_counts()
        ds = _dot_in_session(nt, Mn, Ms[2])
        s2 = nt.slab_algebra_counts()
        _dot_in_session(nt, Md, Ms[2])
        s3 = nt.slab_algebra_counts()
        ns = Md.Norm()
        s4 = nt.slab_algebra_counts()
    print(name, fold, "counts", c0, c1, "slab algebra", s0, s1, s2, s3, s4)
    assert got is not None
    norm, nxt = got
    assert delta(c0, c1) == dict(solves=0, fold_passes=1 if fold else 0, plain_passes=0 if fold else 1, refused=0)
    assert s1["refusals"] == s0["refusals"]
    assert s2["others"] - s1["others"] == 1 and s3["others"] - s2["others"] == 1 and s4["others"] - s3["others"] == 1, "dot and norm were taken in slab form"
    assert s4["refusals"] == s0["refusals"]
    for m, bf in zip(Ms, before):
        assert same(srt(m.triplets()), bf), "the operands are as they were"
    g = srt(O.triplets())
    print(name, fold, "entries", len(want[2]))
    assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]), "pattern"
    assert same(g, want), "values against the restatement"
    assert same(g, srt(V.triplets())), "values against compressed columns"
    # the norm: the bits of MatrixNorm on the restated difference in slab form; and within the any-order bound of each column's sum
    exact = [_sum_bound(t) for t in colterms]
    exact_n, bound_n = max(e for e, _ in exact), max(b for _, b in exact)
    print(name, fold, "norm", norm, "MatrixNorm in slab form", ns, "exact", exact_n, "bound", bound_n, "compressed columns", nv)
    assert norm == ns
    if name != "long":   # (the planted column sets the norm: its sum in MatrixNorm's lane order, restated in numpy)
        assert norm == _lane_sum(diff[ZERO_FIRST], int(diff[ZERO_FIRST][0][0]))
    assert abs(norm - exact_n) <= bound_n and abs(nv - exact_n) <= bound_n
    # the next trace: the bits of DotMatrix(N', S) in slab form
    exact_d, bound_d = _sum_bound(terms)
    print(name, fold, "next trace", nxt, "DotMatrix in slab form", ds, "exact", exact_d, "|difference|", abs(nxt - exact_d), "bound", bound_d,
          "compressed columns", ev)
    assert nxt == ds
    assert abs(nxt - exact_d) <= bound_d and abs(ev - exact_d) <= bound_d


# ------------------------------------------------------------------ refusals
def test_refusals_leave_everything_as_it_was(nt, fma):
    n, j = 4099, 5
    col = lambda f, l, v=None: {j: (np.arange(f, l + 1), np.linspace(0.1, 0.9, l - f + 1) if v is None else v)}

    def attempt(MD, MN, MS, fold, counted):
        O = nt.Matrix_ps(n)
        before = [srt(m.triplets()) for m in (MD, MN, MS)]
        c0, s0 = nt.purify_session_counts(), nt.slab_algebra_counts()
        with nt.solver_session(False):
            got = nt.purify_tail_step(MD, MN, MS, fold, O)
        c1, s1 = nt.purify_session_counts(), nt.slab_algebra_counts()
        assert got is None
        assert c1 == dict(c0, refused=c0["refused"] + counted), (c0, c1)
        assert s1 == s0, (s0, s1)   # (a refused pass is no operation and no refusal of the session)
        for m, bf in zip((MD, MN, MS), before):
            assert same(srt(m.triplets()), bf)
        assert len(O.triplets()[2]) == 0

    MD, near, MS = _matrix(nt, col(0, 9), n=n), _matrix(nt, col(4, 20), n=n), _matrix(nt, col(0, 30), n=n)
    far = _matrix(nt, col(n // 2 + 1, n // 2 + 11), n=n)
    for fold in (1, 0):
        # two runs n / 2 rows apart in one column, either way round: the hull is beyond what the column's slots bound
        attempt(MD, far, MS, fold, 1)
        attempt(far, MD, MS, fold, 1)
        # a D that stores a zero enters slab form as a read-only view: the pass merges no view
        view = col(0, 9)
        view[j][1][4] = 0.0
        attempt(_matrix(nt, view, n=n), near, MS, fold, 1)
        # gated, counted nowhere: one matrix given twice, a complex operand, the option below 2
        attempt(MD, MD, MS, fold, 0)
        attempt(MD, near, MD, fold, 0)
        MC = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, 3, complex_=True))
        attempt(MC, near, MS, fold, 0)
        attempt(MD, near, MC, fold, 0)
        for below in (1, 0):
            nt.set_option("purify_session", below)
            attempt(MD, near, MS, fold, 0)
        nt.set_option("purify_session", 2)
    # the same column with the runs side by side is taken
    d, m, s = np.zeros(31), np.zeros(31), np.linspace(0.1, 0.9, 31)   # (adding an absent entry as +0.0 gives the merge's values)
    d[0:10], m[4:21] = np.linspace(0.1, 0.9, 10), np.linspace(0.1, 0.9, 17)
    for fold in (1, 0):
        O = nt.Matrix_ps(n)
        with nt.solver_session(False):
            got = nt.purify_tail_step(MD, near, MS, fold, O)
        assert got is not None
        o = 2.0 * d + (-m) if fold else m
        e = -1.0 * o + d
        kept = np.flatnonzero(o != 0.0)
        assert len(kept) == (21 if fold else 17) and np.all(e[:21] != 0.0)
        cc, rr, vv = srt(O.triplets())
        assert np.all(cc == j + 1) and np.array_equal(rr, kept + 1) and np.array_equal(vv, o[kept])
        exact_n, bound_n = _sum_bound(np.abs(e))
        exact_d, bound_d = _sum_bound(o * s)
        assert abs(got[0] - exact_n) <= bound_n and abs(got[1] - exact_d) <= bound_d


# ------------------------------------------------------------------ the solver
SOLVE_N, TRACE, THR, CONV, MAXIT = 1024, 512.0, 1e-8, 1e-6, 20


def solve_operands(n=SOLVE_N, c0=0, c1=None):
    """(col, row, val) of D and of S, 1-based, columns [c0, c1): occ_i = ((i 7919) mod 1000) < 500 with 1-based i, D_ii = 0.9 if
    occupied else 0.1, D_ij = -0.02 exp(-0.05 k) / k for 0 < k = |i - j| <= 12; S = I + 0.05 exp(-0.5 k) / k for 0 < k <= 3"""
    c1 = n if c1 is None else c1
    out = []
    for width, diag, off in ((12, lambda i: 0.9 if (i * 7919) % 1000 < 500 else 0.1, lambda k: -0.02 * np.exp(-0.05 * k) / k),
                             (3, lambda i: 1.0, lambda k: 0.05 * np.exp(-0.5 * k) / k)):
        col, row, val = [], [], []
        for j in range(c0 + 1, c1 + 1):
            for i in range(max(1, j - width), min(n, j + width) + 1):
                col.append(j)
                row.append(i)
                val.append(diag(i) if i == j else off(float(abs(i - j))))
        out.append((np.array(col, np.int32), np.array(row, np.int32), np.array(val)))
    return out


def purify_solve(nt, D, S, n, trace=TRACE, thr=THR, conv=CONV, maxit=MAXIT, monitor=False):
    p = nt.SolverParameters()
    p.SetThreshold(thr)
    p.SetConvergeDiff(conv)
    if maxit is not None:
        p.SetMaxIterations(maxit)
    if monitor is not None:
        p.SetMonitorConvergence(monitor)
    K = nt.Matrix_ps(n)
    c0, s0 = nt.purify_session_counts(), nt.slab_algebra_counts()
    nt.GeometryOptimization.PurificationExtrapolate(D, S, trace, K, p)
    c1, s1 = nt.purify_session_counts(), nt.slab_algebra_counts()
    tr = nt.solver_trace()
    return dict(out=srt(K.triplets()), iters=tr["iterations"], sigma=np.asarray(tr["sigma"]).copy(), nnz=np.asarray(tr["nnz"]).copy(),
                trace=np.asarray(tr["energy"]).copy(), norm=np.asarray(tr["value"]).copy(), counts=delta(c0, c1),
                refusals=s1["refusals"] - s0["refusals"])


def equal(x, y):
    return (x["iters"] == y["iters"] and same(x["out"], y["out"]) and np.array_equal(x["sigma"], y["sigma"]) and
            np.array_equal(x["trace"], y["trace"]) and np.array_equal(x["norm"], y["norm"]) and np.array_equal(x["nnz"], y["nnz"]))


def dense(t, n):
    M = np.zeros((n, n))
    M[t[1] - 1, t[0] - 1] = t[2]
    return M


@pytest.fixture(scope="module")
def solve_matrices(nt):
    d, s = solve_operands()
    return nt.Matrix_ps.from_triplets(SOLVE_N, *d), nt.Matrix_ps.from_triplets(SOLVE_N, *s)


def test_solver_2_against_1_against_0(nt, fma, solve_matrices):
    """2 against 1 bit for bit: the pass has the values, the pattern, the norm's and the dot's bits of the session's calls.  1 against
    0: the same iterations and branches, the density within 100 threshold max(1, max|K|), the bound tests/test_gpu_extras.py gives
    this solver against the reference (the session's dot and norm sum in another order).  The option-0 run takes both branches with
    every decision at least 1e-11 trace away from a tie (a condition on the inputs, checked on that run)"""
    D, S = solve_matrices
    runs = {}
    for v in (0, 1, 2):
        nt.set_option("purify_session", v)
        runs[v] = purify_solve(nt, D, S, SOLVE_N)
    nt.set_option("purify_session", 2)
    r0, r1, r2 = runs[0], runs[1], runs[2]
    margins = np.abs(TRACE - r0["trace"]) / TRACE
    print("iterations", r0["iters"], r1["iters"], r2["iters"], "branches of option 0", r0["sigma"].tolist(), "margins", margins.tolist())
    print("counts", r0["counts"], r1["counts"], r2["counts"], "refusals", r0["refusals"], r1["refusals"], r2["refusals"])
    assert set(r0["sigma"].tolist()) == {-1.0, 1.0}, "the reference run takes both branches"
    assert np.all(margins > 1e-11), "no decision of the reference run is near a rounding tie"
    assert 2 <= r0["iters"] < MAXIT
    assert r0["counts"] == dict.fromkeys(KEYS, 0)
    assert r1["counts"] == dict(solves=1, fold_passes=0, plain_passes=0, refused=0)
    # 2 against 1
    assert r2["iters"] == r1["iters"]
    assert np.array_equal(r2["sigma"], r1["sigma"]), "branch sequence"
    assert np.array_equal(r2["trace"], r1["trace"]), "every trace_value, bit for bit"
    assert np.array_equal(r2["norm"], r1["norm"]), "every norm, bit for bit"
    assert np.array_equal(r2["nnz"], r1["nnz"])
    assert same(r2["out"], r1["out"]), "density triplets, bit for bit"
    c = r2["counts"]
    assert c["solves"] == 1 and c["refused"] == 0 and c["fold_passes"] >= 1 and c["plain_passes"] >= 1, c
    assert c["fold_passes"] + c["plain_passes"] >= r2["iters"] - 1, c
    assert r2["refusals"] <= r1["refusals"]
    # 1 against 0
    assert r1["iters"] == r0["iters"]
    assert np.array_equal(r1["sigma"], r0["sigma"]), "branch sequence"
    K0, K1 = dense(r0["out"], SOLVE_N), dense(r1["out"], SOLVE_N)
    diff = float(np.abs(K1 - K0).max())
    print("max |K1 - K0|", diff, "bound", 100 * THR * max(1.0, np.abs(K0).max()), "max relative trace difference",
          float(np.max(np.abs(r1["trace"] - r0["trace"]) / np.abs(r0["trace"]))))
    assert diff <= 100 * THR * max(1.0, np.abs(K0).max())


def test_golden_case_with_the_session(nt, fma):
    """the `purify` case of tests/golden/extras.npz (D, S_old, trace 30) with options 1 and 2 against the reference's result, in the
    bound tests/test_gpu_extras.py gives it"""
    g = Golden("extras")
    hits = [(i, c) for i, c in enumerate(g.cases) if c["kind"] == "purify"]
    assert len(hits) == 1
    i, c = hits[0]
    assert c["A"] == "D" and c["B"] == "S_old" and c["p1"] == 30
    tA, tB = g.tri(None, "M_D"), g.tri(None, "M_S_old")
    A, B = nt.Matrix_ps.from_triplets(tA[0], tA[2], tA[3], tA[4]), nt.Matrix_ps.from_triplets(tB[0], tB[2], tB[3], tB[4])
    want = g.tri(i, "K")
    wd = to_dense(want)
    for v in (1, 2):
        nt.set_option("purify_session", v)
        r = purify_solve(nt, A, B, tA[0], trace=c["p1"], thr=c["thr"], conv=c["conv"], maxit=None, monitor=None)
        gd = to_dense((want[0], want[1]) + tuple(r["out"]))
        diff = float(np.abs(gd - wd).max())
        print("option", v, "iterations", r["iters"], "counts", r["counts"], "max |K - K_ref|", diff, "bound", 100 * c["thr"] * max(1.0, np.abs(wd).max()))
        assert r["counts"]["solves"] == 1 and r["counts"]["refused"] == 0
        assert diff <= 100 * c["thr"] * max(1.0, np.abs(wd).max())
    nt.set_option("purify_session", 2)


def test_gates(nt, fma, solve_matrices):
    """slab_algebra = 0, the option at 0 and a complex operand fuse nothing, refuse nothing and open no session: the results of
    option 0 bit for bit"""
    D, S = solve_matrices
    iters = 4
    none = dict.fromkeys(KEYS, 0)
    nt.set_option("purify_session", 0)
    want = purify_solve(nt, D, S, SOLVE_N, maxit=iters)
    again = purify_solve(nt, D, S, SOLVE_N, maxit=iters)
    assert want["counts"] == none == again["counts"] and equal(want, again)
    nt.set_option("purify_session", 2)
    nt.set_option("slab_algebra", 0)
    a = purify_solve(nt, D, S, SOLVE_N, maxit=iters)
    nt.set_option("purify_session", 0)
    want_a = purify_solve(nt, D, S, SOLVE_N, maxit=iters)
    nt.set_option("slab_algebra", 1)
    nt.set_option("purify_session", 2)
    assert a["counts"] == none == want_a["counts"] and equal(a, want_a)
    nc = 1024
    Dc = nt.Matrix_ps.from_triplets(nc, *banded_triplets(nc, 12, complex_=True))
    c = purify_solve(nt, Dc, S, nc, maxit=iters)
    nt.set_option("purify_session", 0)
    d = purify_solve(nt, Dc, S, nc, maxit=iters)
    nt.set_option("purify_session", 2)
    assert c["counts"] == none == d["counts"] and equal(c, d)


# ------------------------------------------------------------------ two ranks
def run_world(world, tmp_path):
    out = str(tmp_path / ("purify%d" % world))
    name = "s%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name, NTPOLY_AMD_SHM_MB="64",
                   NTPOLY_AMD_SPGEMM_FMA="1")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "purify_session_worker.py"), out],
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


def test_two_ranks(tmp_path):
    """the solver test's operands as column panels on two ranks sharing one GPU (shared-memory transport, FMA arithmetic), options
    2, 1 and 0 in the same processes: 2 against 1 bit for bit on every rank and in the gathered density, fused passes of both kinds
    on both ranks; against 0 the same counts and branch sequence and the solver test's bound; one branch sequence on both ranks"""
    two = run_world(2, tmp_path)
    for r, p in enumerate(two):
        it = {v: int(p["iters_%d" % v][0]) for v in (0, 1, 2)}
        print("rank", r, "iterations", it, "counts (solves, fold, plain, refused)", [p["counts_%d" % v].tolist() for v in (2, 1, 0)],
              "branches", p["sigma_0"].tolist())
        assert it[2] == it[1] == it[0] >= 2
        for k in ("sigma", "trace", "norm", "nnz"):
            assert np.array_equal(p["%s_2" % k], p["%s_1" % k]), k
        assert np.array_equal(p["sigma_1"], p["sigma_0"]), "branch sequence against option 0"
        assert set(p["sigma_0"].tolist()) == {-1.0, 1.0}
        assert p["counts_0"].tolist() == [0, 0, 0, 0] and p["counts_1"].tolist() == [1, 0, 0, 0]
        c = p["counts_2"]
        assert c[0] == 1 and c[1] >= 1 and c[2] >= 1 and c[3] == 0 and c[1] + c[2] >= it[2] - 1, (r, c)
    gathered = {}
    for v in (0, 1, 2):
        gathered[v] = tuple(np.concatenate([p["%s_%d" % (k, v)] for p in two]) for k in ("col", "row", "val"))
    assert same(srt(gathered[2]), srt(gathered[1])), "gathered density, 2 against 1"
    assert len(gathered[2][2]) > SOLVE_N
    K0, K1 = dense(gathered[0], SOLVE_N), dense(gathered[1], SOLVE_N)
    diff = float(np.abs(K1 - K0).max())
    print("two ranks: max |K1 - K0|", diff)
    assert diff <= 100 * THR * max(1.0, np.abs(K0).max())
    for v in (0, 1, 2):
        assert np.array_equal(two[0]["sigma_%d" % v], two[1]["sigma_%d" % v]), "one branch sequence on both ranks"
