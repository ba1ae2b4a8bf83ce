"""GPU: ComputeExponentialPade in a slab session (option pade_session; csrc/pade_chain.hip k_pade_chain, engine.hpp ps_pade_chain).
Around its CG solve the call builds, with the vocabulary at threshold 0,
    P1      = 17297280 I + 1995840 B1 + 25200 B2 + 56 B3          TempMat  = 8648640 I + 277200 B1 + 1512 B2 + B3
    LeftMat = P1 - P2                                              RightMat = P1 + P2
each as CopyMatrix(Base, Out); ScaleMatrix(Out, s); IncrementMatrix(A_k, Out, c_k, 0) for k = 1..m.  With the option at 1 the whole
call runs in a slab session, at 2 each of the two groups is one pass over the runs with two outputs.

The kernel is reached with crafted operands through nt.pade_chain_step and compared with (i) the same vocabulary calls on
compressed columns (slab_algebra = 0) and (ii) a numpy restatement of AddSparseVectors.f90 at threshold 0 written here -- never
with the fused code itself.  numpy's float64 products and sums are the correctly rounded ones the kernel spells as __dmul_rn /
__dadd_rn, so patterns are compared for equality and values with np.array_equal.  The solver is held to bit equality between the
options 2, 1 and 0: the session's products and merges have the bits of the calls on compressed columns, and the call's only
reductions are the norm taken before the session opens and CG's own."""
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
KEYS = ("solves", "sum_passes", "pair_passes", "refused")
PADE_S = (17297280.0, 8648640.0)
PADE_C = ((1995840.0, 25200.0, 56.0), (277200.0, 1512.0, 1.0))
FREE_S = (2.0, 3.0)
FREE_C = ((-1.5, 0.625, 4.0), (0.25, -1.75, 2.0))
PAIR_S = (1.0, 1.0)
PAIR_C = ((-1.0,), (1.0,))


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture(params=[1, 0], ids=["fma", "unfused"])
def fma(nt, request):
    """both arithmetic modes: slots padded to the tile kernel's row alignment, and runs packed back to back"""
    before = {k: nt.get_option(k) for k in ("spgemm_fma", "slab_algebra", "pade_session", "cg_dots")}
    nt.set_option("spgemm_fma", request.param)
    nt.set_option("pade_session", 2)
    yield request.param
    for k, v in before.items():
        nt.set_option(k, v)


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
EMPTY = {"B": {7}, "A1": {8, 40}, "A2": {9, 40}, "A3": {10, 40}}   # empty in each input in turn; column 40 in every addend
BELOW, ABOVE = 60, 150        # columns whose addend runs all lie below / above the Base entry (the diagonal row)
FULL = 120                    # A2 fills all N rows of this column: a second trip of the chunk loop
CANCEL, REAPPEAR, LAST = 30, 31, 32   # the planted columns, each on its own diagonal row


def _runs(rng, n, empty):
    """{column: (rows, values)}: a run around the diagonal with half-widths 6..90 drawn per side, ~12 % holes inside, values
    log-uniform in [1e-6, 1] with a random sign"""
    cols = {}
    for j in range(n):
        if j in empty:
            continue
        if j == BELOW:
            f, l = j + 3, j + int(rng.integers(30, 60))
        elif j == ABOVE:
            f, l = j - int(rng.integers(30, 60)), j - 3
        elif j == FULL:
            f, l = 0, n - 1
        else:
            f, l = max(0, j - int(rng.integers(6, 91))), min(n - 1, j + int(rng.integers(6, 91)))
        rows = np.arange(f, l + 1)
        keep = rng.random(len(rows)) > 0.12
        keep[0] = keep[-1] = True
        rows = rows[keep]
        cols[j] = (rows, 10.0 ** rng.uniform(-6.0, 0.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows)))
    return cols


def _diagonal(rng, n, empty):
    """one entry per column, on the diagonal row: what the identity is in slab form"""
    return {j: (np.array([j]), 10.0 ** rng.uniform(-1.0, 0.0, 1)) for j in range(n) if j not in empty}


def _set(cols, j, r, v):
    rows, vals = cols[j]
    if r in rows:
        vals[rows == r] = v
    else:
        k = int(np.searchsorted(rows, r))
        cols[j] = (np.insert(rows, k, r), np.insert(vals, k, v))


def _unset(cols, j, r):
    rows, vals = cols[j]
    if len(rows) > 1 and r in (rows[0], rows[-1]):   # (keep the run's extent: move the hole's neighbour in instead)
        raise AssertionError("planted rows lie inside the runs")
    cols[j] = (rows[rows != r], vals[rows != r])


def _plant(B, A1, A2, A3):
    """exact by construction and checked here in numpy, with the FREE scalars; every planted row is its column's diagonal row"""
    (s1, s2), (c1, c2) = FREE_S, FREE_C
    b, a1, a3, a3l = 0.375, 0.5, 0.25, -0.1875
    # CANCEL: c_11 a_1 + s_1 b == 0 while output 2 keeps the row; addends 2 and 3 do not hold it
    assert c1[0] * a1 + s1 * b == 0.0 and c2[0] * a1 + s2 * b == 1.25
    # REAPPEAR: the same, and addend 3 holds the row again: the entry comes back one-sided
    assert c1[2] * a3 == 1.0 and (c2[0] * a1 + s2 * b) + c2[2] * a3 == 1.75
    for j in (CANCEL, REAPPEAR):
        _set(B, j, j, b)
        _set(A1, j, j, a1)
        _unset(A2, j, j)
        _unset(A3, j, j)
    _set(A3, REAPPEAR, REAPPEAR, a3)
    # LAST: addends 1 and 2 do not hold the row, the LAST addend cancels it in output 1
    assert s1 * b + c1[2] * a3l == 0.0 and s2 * b + c2[2] * a3l == 0.75
    _set(B, LAST, LAST, b)
    _unset(A1, LAST, LAST)
    _unset(A2, LAST, LAST)
    _set(A3, LAST, LAST, a3l)


def _crafted():
    rng = np.random.default_rng(20261021)
    A1, A2, A3 = (_runs(rng, N, EMPTY[k]) for k in ("A1", "A2", "A3"))
    B = _diagonal(rng, N, EMPTY["B"])
    _plant(B, A1, A2, A3)
    R = _runs(rng, N, EMPTY["B"])   # a Base with runs of its own (what P1 is to the pair pass)
    # the pair pass's own cancellation: P1 - P2 == 0 on one row, P1 + P2 keeps it
    _set(R, CANCEL, CANCEL + 3, 0.5)
    _set(A1, CANCEL, CANCEL + 3, 0.5)
    return dict(B=B, A1=A1, A2=A2, A3=A3, R=R)


# name: (Base, addends, scales, coefficients)
CASES = {"pade": ("B", ("A1", "A2", "A3"), PADE_S, PADE_C), "free": ("B", ("A1", "A2", "A3"), FREE_S, FREE_C),
         "free_runs": ("R", ("A3", "A1", "A2"), FREE_S, FREE_C), "pair": ("R", ("A1",), PAIR_S, PAIR_C),
         "pair_diagonal": ("B", ("A2",), PAIR_S, PAIR_C)}


@pytest.fixture(scope="module")
def operands():
    return _crafted()


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
def add_sparse(a, alpha, b, stats):
    """alpha a + b on sorted sparse vectors (rows, values), the scaled value rounded, then added: inside the overlap of the two
    lists an entry is kept iff its value is not zero, beyond the end of one list the tail of the other is copied unfiltered"""
    (ra, va), (rb, vb) = a, b
    if len(ra) == 0 and len(rb) == 0:
        return ra, va
    rows = np.union1d(ra, rb)
    ia, ib = np.isin(rows, ra), np.isin(rows, rb)
    wa, wb = np.zeros(len(rows)), np.zeros(len(rows))
    wa[ia] = alpha * va
    wb[ib] = vb
    s = np.where(ia & ib, wa + wb, np.where(ia, wa, wb))
    lim = min(ra[-1] if len(ra) else -1, rb[-1] if len(rb) else -1)
    nz = s != 0.0
    keep = (rows > lim) | nz
    stats["both_kept"] = stats.get("both_kept", 0) + int((ia & ib & nz).sum())
    stats["cancelled"] = stats.get("cancelled", 0) + int((ia & ib & ~nz).sum())
    stats["only_a"] = stats.get("only_a", 0) + int((ia & ~ib).sum())
    stats["only_b"] = stats.get("only_b", 0) + int((~ia & ib).sum())
    stats["underflow"] = stats.get("underflow", 0) + int((~nz & ~(ia & ib)).sum())
    return rows[keep], s[keep]


def restated(ops, case, n=N):
    """both outputs of the chain as {column: (rows, values)}, and branch statistics per output"""
    base, addends, scales, coeffs = CASES[case] if isinstance(case, str) else case
    empty = (np.zeros(0, dtype=np.int64), np.zeros(0))
    outs, stats = [], []
    for q in range(2):
        st, res = {}, {}
        for j in range(n):
            rb, vb = ops[base].get(j, empty)
            v = (rb, scales[q] * vb)                                           # CopyMatrix(Base, Out); ScaleMatrix(Out, s)
            st["underflow"] = st.get("underflow", 0) + int((v[1] == 0.0).sum())
            for name, c in zip(addends, coeffs[q]):
                v = add_sparse(ops[name].get(j, empty), c, v, st)             # IncrementMatrix(A_k, Out, c_k, 0)
            if len(v[0]):
                res[j] = v
        outs.append(res)
        stats.append(st)
    return outs, stats


def _has(cols, j, r):
    return j in cols and r in cols[j][0]


def test_the_inputs_reach_every_branch(operands):
    """from the operands and the numpy restatement alone: a column empty in each input in turn and one empty in every addend (the
    output is Base alone), addend runs wholly below and wholly above the Base entry, a run that fills all N > 256 rows, columns 0
    and N - 1, holes inside runs, both-present sums that are kept, the three planted exact cases, one-sided entries from either
    side; no scaled value is zero where an entry is held, nothing is far apart"""
    o = operands
    assert N % 4 != 0 and N > 256
    assert 7 not in o["B"] and 8 not in o["A1"] and 9 not in o["A2"] and 10 not in o["A3"]
    assert 40 in o["B"] and all(40 not in o[k] for k in ("A1", "A2", "A3"))
    for k in ("A1", "A2", "A3"):
        M = o[k]
        assert 0 in M and N - 1 in M and M[BELOW][0][0] > BELOW and M[ABOVE][0][-1] < ABOVE
        holes = sum(int(r[-1] - r[0] + 1 - len(r)) for r, _ in M.values())
        span = sum(int(r[-1] - r[0] + 1) for r, _ in M.values())
        assert 0.08 < holes / span < 0.16, holes / span
    assert o["A2"][FULL][0][0] == 0 and o["A2"][FULL][0][-1] == N - 1
    assert all(list(r) == [j] for j, (r, _) in o["B"].items())
    # nothing lies far apart: per column the hull is covered by the runs themselves (every run touches or overlaps the next)
    for case, (base, addends, _, _) in CASES.items():
        for j in range(N):
            ext = sorted((int(o[k][j][0][0]), int(o[k][j][0][-1])) for k in (base,) + addends if j in o[k])
            reach = ext[0][1] if ext else 0
            for f, l in ext[1:]:
                assert f <= reach + 3, (case, j, ext)
                reach = max(reach, l)
    for case in CASES:
        outs, stats = restated(o, case)
        print(case, stats)
        for st in stats:
            assert st["underflow"] == 0
            # (a diagonal Base meets its one addend on the diagonal rows only)
            assert st["both_kept"] > (100 if case == "pair_diagonal" else 1000) and st["only_a"] > 0 and st["only_b"] > 0, (case, st)
    (o1, o2), (st1, st2) = restated(o, "free")
    assert st1["cancelled"] == 3 and st2["cancelled"] == 0, (st1, st2)
    assert not _has(o1, CANCEL, CANCEL) and o2[CANCEL][1][o2[CANCEL][0] == CANCEL][0] == 1.25
    assert o1[REAPPEAR][1][o1[REAPPEAR][0] == REAPPEAR][0] == 1.0 and o2[REAPPEAR][1][o2[REAPPEAR][0] == REAPPEAR][0] == 1.75
    assert not _has(o1, LAST, LAST) and o2[LAST][1][o2[LAST][0] == LAST][0] == 0.75
    assert list(o1[40][0]) == [40] and o1[40][1][0] == FREE_S[0] * o["B"][40][1][0], "Base alone"
    assert 7 in o1 and 7 in o2
    (l, r), (stl, str_) = restated(o, "pair")
    assert stl["cancelled"] == 1 and str_["cancelled"] == 0
    assert not _has(l, CANCEL, CANCEL + 3) and r[CANCEL][1][r[CANCEL][0] == CANCEL + 3][0] == 1.0
    # the two outputs end with different patterns
    assert not np.array_equal(_triplets(o1)[1], _triplets(o2)[1]) and len(_triplets(l)[1]) == len(_triplets(r)[1]) - 1


def _vocabulary(nt, Base, addends, scales, coeffs):
    """the calls of solvers_extra.cpp compute_exponential_pade for one group, through the C ABI"""
    outs = []
    for q in range(2):
        V = nt.Matrix_ps(Base)
        if scales[q] != 1.0:
            V.Scale(scales[q])
        for A, c in zip(addends, coeffs[q]):
            V.Increment(A, c, 0.0)
        outs.append(V)
    return outs


@pytest.mark.parametrize("case", sorted(CASES))
def test_pass_bit_for_bit(nt, fma, operands, case):
    base, addends, scales, coeffs = CASES[case]
    want = [_triplets(o) for o in restated(operands, case)[0]]
    names = (base,) + addends
    Ms = [_matrix(nt, operands[k]) for k in names]
    before = [srt(m.triplets()) for m in Ms]
    # (i) the vocabulary on compressed columns against (ii) the restatement
    nt.set_option("slab_algebra", 0)
    V = _vocabulary(nt, Ms[0], Ms[1:], scales, coeffs)
    nt.set_option("slab_algebra", 1)
    for q in range(2):
        assert same(srt(V[q].triplets()), want[q]), "compressed columns against the restatement, output %d" % (q + 1)
    O1, O2 = nt.Matrix_ps(N), nt.Matrix_ps(N)
    c0, s0 = nt.pade_session_counts(), nt.slab_algebra_counts()
    with nt.solver_session(False):
        got = nt.pade_chain_step(Ms[0], Ms[1:], scales, coeffs, O1, O2)
        c1, s1 = nt.pade_session_counts(), nt.slab_algebra_counts()
    print(case, "counts", c0, c1, "slab algebra", s0, s1, "entries", len(want[0][2]), len(want[1][2]))
    assert got is True
    m = len(addends)
    assert delta(c0, c1) == dict(solves=0, sum_passes=1 if m == 3 else 0, pair_passes=1 if m == 1 else 0, refused=0)
    assert s1["refusals"] == s0["refusals"]
    for M, bf in zip(Ms, before):
        assert same(srt(M.triplets()), bf), "the operands are as they were"
    for q, O in enumerate((O1, O2)):
        g = srt(O.triplets())
        assert np.array_equal(g[0], want[q][0]) and np.array_equal(g[1], want[q][1]), "pattern, output %d" % (q + 1)
        assert same(g, want[q]), "values against the restatement, output %d" % (q + 1)
        assert same(g, srt(V[q].triplets())), "values against compressed columns, output %d" % (q + 1)


# ------------------------------------------------------------------ refusals
def test_refusals_leave_everything_as_it_was(nt, fma):
    n, j = 4099, 5
    col = lambda f, l, v=None: {j: (np.arange(f, l + 1), np.linspace(0.1, 0.9, l - f + 1) if v is None else np.asarray(v, dtype=np.float64))}

    def attempt(Base, addends, counted, scales=PAIR_S, coeffs=None, outs=None, call=None):
        coeffs = tuple((c,) * len(addends) for c in (-1.0, 1.0)) if coeffs is None else coeffs
        O1, O2 = outs if outs else (nt.Matrix_ps(n), nt.Matrix_ps(n))
        ms = [Base] + list(addends)
        before = [srt(m.triplets()) for m in ms]
        c0, s0 = nt.pade_session_counts(), nt.slab_algebra_counts()
        with nt.solver_session(False):
            got = call() if call else nt.pade_chain_step(Base, addends, scales, coeffs, O1, O2)
        c1, s1 = nt.pade_session_counts(), nt.slab_algebra_counts()
        assert not got
        assert c1 == dict(c0, refused=c0["refused"] + counted), (c0, c1)
        assert s1 == s0, (s0, s1)   # (a refused pass is no operation and no refusal of the session)
        for m, bf in zip(ms, before):
            assert same(srt(m.triplets()), bf)
        if not outs:
            assert len(O1.triplets()[2]) == 0 and len(O2.triplets()[2]) == 0

    mk = lambda c: _matrix(nt, c, n=n)
    MB, near, near2, near3 = mk(col(0, 9)), mk(col(4, 20)), mk(col(8, 30)), mk(col(2, 12))
    far = mk(col(n // 2 + 1, n // 2 + 11))
    # two runs n / 2 rows apart in one column, in either role: the hull is beyond what the column's slots and pads bound
    attempt(MB, [far], 1)
    attempt(far, [MB], 1)
    attempt(MB, [near, far, near2], 1)
    # an input that stores a zero enters slab form as a read-only view: the pass merges no view
    view = col(0, 9)
    view[j][1][4] = 0.0
    attempt(mk(view), [near], 1)
    attempt(MB, [mk(view)], 1)
    # a coefficient and a value whose product underflows to zero where the entry is held: Base's own, and a one-sided addend's
    tiny = mk(col(0, 9, [1e-300] + [0.5] * 9))
    assert 1e-300 * 1e-300 == 0.0
    attempt(tiny, [near], 1, scales=(1e-300, 1.0))
    tiny_tail = mk(col(4, 20, [0.5] * 16 + [1e-300]))
    attempt(MB, [tiny_tail], 1, coeffs=((1e-300,), (1.0,)))
    # an Inf
    attempt(MB, [mk(col(4, 20, [0.5] * 8 + [np.inf] + [0.5] * 8))], 1)
    attempt(mk(col(0, 9, [0.5] * 9 + [-np.inf])), [near], 1)
    # gated, counted nowhere: one matrix given twice, a complex input, the option below 2, two addends
    attempt(MB, [MB], 0)
    attempt(MB, [near, near2, near], 0)
    attempt(MB, [near], 0, outs=(MB, nt.Matrix_ps(n)))
    O = nt.Matrix_ps(n)
    attempt(MB, [near], 0, outs=(O, O))
    MC = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, 3, complex_=True))
    attempt(MC, [near], 0)
    attempt(MB, [MC], 0)
    attempt(MB, [near, MC, near2], 0)
    for below in (1, 0):
        nt.set_option("pade_session", below)
        attempt(MB, [near], 0)
        attempt(MB, [near, near2, near3], 0)
    nt.set_option("pade_session", 2)
    attempt(MB, [near, near2], 0, coeffs=((1.0, 1.0), (1.0, 1.0)))
    # the same column with the runs side by side is taken, in both instances
    b, a1, a2, a3 = np.zeros(31), np.zeros(31), np.zeros(31), np.zeros(31)   # (adding an absent entry as +0.0 gives the merge's values)
    b[0:10], a1[4:21], a2[8:31], a3[2:13] = np.linspace(0.1, 0.9, 10), np.linspace(0.1, 0.9, 17), np.linspace(0.1, 0.9, 23), np.linspace(0.1, 0.9, 11)
    for addends, dense, scales, coeffs in (([near], [a1], PAIR_S, PAIR_C), ([near, near2, near3], [a1, a2, a3], PADE_S, PADE_C)):
        O1, O2 = nt.Matrix_ps(n), nt.Matrix_ps(n)
        c0 = nt.pade_session_counts()
        with nt.solver_session(False):
            got = nt.pade_chain_step(MB, addends, scales, coeffs, O1, O2)
        assert got is True and nt.pade_session_counts()["refused"] == c0["refused"]
        for q, O in enumerate((O1, O2)):
            o = scales[q] * b
            for c, a in zip(coeffs[q], dense):
                o = c * a + o
            kept = np.flatnonzero(o != 0.0)
            assert len(kept) >= 21
            cc, rr, vv = srt(O.triplets())
            assert np.all(cc == j + 1) and np.array_equal(rr, kept + 1) and np.array_equal(vv, o[kept])


# ------------------------------------------------------------------ the solver
# (n, half bandwidth, shift, threshold, sigma, squarings behind CG, CG iterations, longest column of B1 / B2 / B3 / P2 in rows)
SOLVES = {"shifted": (259, 8, 2.0, 1e-9, 8.0, 3, 6, (33, 63, 61, 79)), "wide": (400, 20, 0.0, 1e-12, 4.0, 2, 8, (81, 161, 226, 229))}
CONV = 1e-6


def solve_triplets(name, c0=0, c1=None):
    n, h, shift = SOLVES[name][:3]
    return banded_triplets(n, h, shift=shift, c0=c0, c1=c1)


def dense(t, n):
    M = np.zeros((n, n), dtype=np.asarray(t[2]).dtype)
    M[t[1] - 1, t[0] - 1] = t[2]
    return M


def _longest(M):
    out = 0
    for j in range(M.shape[1]):
        nz = np.flatnonzero(M[:, j])
        if len(nz):
            out = max(out, int(nz[-1] - nz[0] + 1))
    return out


@pytest.mark.parametrize("name", sorted(SOLVES))
def test_the_solver_operands_in_numpy(name):
    """what the solver tests rely on, from a dense restatement: the norm that chooses sigma, a well-conditioned LeftMat, and powers
    that prune -- B3 is NOT wider than B2 on the shifted operand, so the pass must not assume that the runs nest"""
    n, h, shift, thr, sigma, squarings, _, longest = SOLVES[name]
    A = dense(solve_triplets(name), n)
    norm = np.abs(A).sum(axis=0).max()
    s, counter = 1.0, 1
    while norm / s > 1.0:
        s *= 2
        counter += 1
    assert (s, counter - 1) == (sigma, squarings), (norm, s, counter)
    prune = lambda M: np.where(np.abs(M) > thr / s, M, 0.0)
    S = A / s
    B1 = prune(S @ S)
    B2 = prune(B1 @ B1)
    B3 = prune(B2 @ B2)
    I = np.eye(n)
    P1 = PADE_S[0] * I + PADE_C[0][0] * B1 + PADE_C[0][1] * B2 + PADE_C[0][2] * B3
    T = PADE_S[1] * I + PADE_C[1][0] * B1 + PADE_C[1][1] * B2 + PADE_C[1][2] * B3
    P2 = prune(S @ T)
    cond = np.linalg.cond(P1 - P2)
    print(name, "norm", norm, "sigma", s, "cond(LeftMat)", cond, "longest columns", [_longest(M) for M in (B1, B2, B3, P2)])
    if name == "shifted":
        assert abs(norm - 4.17) < 0.01 and abs(cond - 1.2) < 0.05
    assert cond < 1.5
    assert tuple(_longest(M) for M in (B1, B2, B3, P2)) == longest
    assert squarings >= 2


def pade_solve(nt, A, n, thr, conv=CONV, perm=None):
    p = nt.SolverParameters()
    p.SetThreshold(thr)
    p.SetConvergeDiff(conv)
    if perm is not None:
        p.SetLoadBalance(perm)
    Out = nt.Matrix_ps(n)
    c0, g0, s0 = nt.pade_session_counts(), nt.cg_dots_counts(), nt.slab_algebra_counts()
    nt.ExponentialSolvers.ComputeExponentialPade(A, Out, p)
    c1, g1, s1 = nt.pade_session_counts(), nt.cg_dots_counts(), nt.slab_algebra_counts()
    return dict(out=srt(Out.triplets()), counts=delta(c0, c1), cg=delta(g0, g1), refusals=s1["refusals"] - s0["refusals"])


NONE = dict.fromkeys(KEYS, 0)
SESSION = dict(solves=1, sum_passes=0, pair_passes=0, refused=0)
FUSED = dict(solves=1, sum_passes=1, pair_passes=1, refused=0)


@pytest.mark.parametrize("name", sorted(SOLVES))
def test_solver_2_against_1_against_0(nt, fma, name):
    """Out equal in pattern and bits across the options 2, 1 and 0, the same number of CG iterations (two dot passes each), the
    counters of each option; and with cg_dots = 0 under option 2 the CG loop on compressed columns: the same Out, no CG counter"""
    n, _, _, thr, _, _, cg_iterations, _ = SOLVES[name]
    A = nt.Matrix_ps.from_triplets(n, *solve_triplets(name))
    assert nt.get_option("cg_dots") == 1
    runs = {}
    for v in (2, 1, 0):
        nt.set_option("pade_session", v)
        runs[v] = pade_solve(nt, A, n, thr)
    nt.set_option("pade_session", 2)
    nt.set_option("cg_dots", 0)
    try:
        plain_cg = pade_solve(nt, A, n, thr)
    finally:
        nt.set_option("cg_dots", 1)
    for v in (2, 1, 0):
        print(name, "option", v, "counts", runs[v]["counts"], "cg", runs[v]["cg"], "refusals", runs[v]["refusals"], "entries", len(runs[v]["out"][2]))
    print(name, "cg_dots 0", plain_cg["counts"], plain_cg["cg"], plain_cg["refusals"])
    assert np.isfinite(runs[0]["out"][2]).all() and len(runs[0]["out"][2]) > n
    assert runs[0]["counts"] == NONE and runs[1]["counts"] == SESSION and runs[2]["counts"] == FUSED
    for v in (2, 1, 0):
        assert runs[v]["cg"]["solves"] == 1 and runs[v]["cg"]["refused"] == 0
        assert runs[v]["cg"]["passes"] == 2 * cg_iterations, "CG iterations"
    for v in (1, 2):
        first = ("pattern" if not (np.array_equal(runs[v]["out"][0], runs[0]["out"][0]) and np.array_equal(runs[v]["out"][1], runs[0]["out"][1]))
                 else "values")
        assert same(runs[v]["out"], runs[0]["out"]), "option %d against 0: %s differ" % (v, first)
    assert plain_cg["counts"] == FUSED
    assert plain_cg["cg"] == dict.fromkeys(plain_cg["cg"], 0)
    assert same(plain_cg["out"], runs[0]["out"])


def balance_lookup(n):
    """a fixed permutation for the load balancer, the same in every process: 1-based, seeded"""
    return (np.random.default_rng(20261021).permutation(n) + 1).astype(np.int32)


@pytest.mark.parametrize("kind", ("reverse", "seeded"))
def test_solver_with_a_load_balancer_permutation(nt, fma, kind):
    """SetLoadBalance reaches CGSolver through the solver parameters, and CGSolver permutes its operands before its own session
    opens: with a permutation LeftMat and RightMat leave slab form before the solve.  Out with 2, 1 and 0 bit for bit, the
    counters of each option, and the permuted solve agrees with the plain one within 100 threshold max(1, max|K|) (the bound of
    the two-rank test: CG sums its traces over permuted columns in another order).  `reverse` keeps the band; `seeded`
    scatters it, so CG's operands are not run-like"""
    n, _, _, thr = SOLVES["shifted"][:4]
    A = nt.Matrix_ps.from_triplets(n, *solve_triplets("shifted"))
    perm = nt.Permutation(n)
    if kind == "reverse":
        perm.SetReversePermutation()
    else:
        perm.set_lookup(balance_lookup(n))
    runs = {}
    for v in (2, 1, 0):
        nt.set_option("pade_session", v)
        runs[v] = pade_solve(nt, A, n, thr, perm=perm)
        print(kind, "option", v, "counts", runs[v]["counts"], "cg", runs[v]["cg"], "refusals", runs[v]["refusals"], "entries", len(runs[v]["out"][2]))
    plain = pade_solve(nt, A, n, thr)
    nt.set_option("pade_session", 2)
    assert runs[0]["counts"] == NONE and runs[1]["counts"] == SESSION and runs[2]["counts"] == FUSED
    assert np.isfinite(runs[0]["out"][2]).all() and len(runs[0]["out"][2]) > n
    for v in (1, 2):
        assert runs[v]["cg"] == runs[0]["cg"], "CG took the same path"
        assert same(runs[v]["out"], runs[0]["out"]), "option %d against 0" % v
    K0, Kp = dense(plain["out"], n), dense(runs[0]["out"], n)
    diff = float(np.abs(Kp - K0).max())
    print(kind, "permuted against plain: max |difference|", diff, "bound", 100 * thr * max(1.0, np.abs(K0).max()))
    assert diff <= 100 * thr * max(1.0, np.abs(K0).max())


def test_gates(nt, fma):
    """a complex operand, a grid with two process slices and slab_algebra = 0 open no session, fuse nothing and refuse nothing: the
    result of option 0 bit for bit.  An operand that stores a zero on its diagonal gives option 0's result whatever path it takes"""
    n, h, shift, thr = SOLVES["shifted"][:4]

    def pair(A, nn):
        nt.set_option("pade_session", 2)
        a = pade_solve(nt, A, nn, thr)
        nt.set_option("pade_session", 0)
        b = pade_solve(nt, A, nn, thr)
        nt.set_option("pade_session", 2)
        return a, b

    a, b = pair(nt.Matrix_ps.from_triplets(n, *banded_triplets(n, h, complex_=True, shift=shift)), n)
    assert a["counts"] == NONE == b["counts"] and same(a["out"], b["out"]) and len(a["out"][2]) > n
    nt.set_option("slab_algebra", 0)
    a, b = pair(nt.Matrix_ps.from_triplets(n, *solve_triplets("shifted")), n)
    nt.set_option("slab_algebra", 1)
    assert a["counts"] == NONE == b["counts"] and same(a["out"], b["out"]) and len(a["out"][2]) > n
    nt.set_option("virtual_grid", 1)
    try:
        nt.ConstructGlobalProcessGrid(1, 1, 2)
        a, b = pair(nt.Matrix_ps.from_triplets(n, *solve_triplets("shifted")), n)
    finally:
        nt.ConstructGlobalProcessGrid(1, 1, 1)
        nt.set_option("virtual_grid", 0)
    assert a["counts"] == NONE == b["counts"] and same(a["out"], b["out"]) and len(a["out"][2]) > n
    c, r, v = solve_triplets("shifted")
    v = v.copy()
    v[(c == 101) & (r == 101)] = 0.0
    assert np.count_nonzero(v == 0.0) == 1
    Z = nt.Matrix_ps.from_triplets(n, c, r, v)
    assert len(Z.triplets()[2]) == len(v)
    a, b = pair(Z, n)
    print("stored zero: counts", a["counts"], "refusals", a["refusals"])
    assert b["counts"] == NONE and same(a["out"], b["out"]) and len(a["out"][2]) > n


def test_golden_case_with_the_session(nt, fma):
    """the `pade` case of tests/golden/extras.npz with options 1 and 2 against the reference's result, in the bound
    tests/test_gpu_extras.py gives this solver: 1e-7 max(1, largest entry)"""
    g = Golden("extras")
    hits = [(i, c) for i, c in enumerate(g.cases) if c["kind"] == "pade"]
    assert len(hits) == 1
    i, c = hits[0]
    tA = g.tri(None, "M_" + c["A"])
    A = nt.Matrix_ps.from_triplets(tA[0], tA[2], tA[3], tA[4])
    want = g.tri(i, "K")
    wd = to_dense(want)
    for v in (1, 2):
        nt.set_option("pade_session", v)
        r = pade_solve(nt, A, tA[0], c["thr"], conv=c["conv"])
        gd = to_dense((want[0], want[1]) + tuple(r["out"]))
        diff = float(np.abs(gd - wd).max())
        print("option", v, "counts", r["counts"], "max |K - K_ref|", diff, "bound", 1e-7 * max(1.0, np.abs(wd).max()))
        assert r["counts"]["solves"] == 1
        assert diff <= 1e-7 * max(1.0, np.abs(wd).max())
    nt.set_option("pade_session", 2)


# ------------------------------------------------------------------ two ranks
def run_world(world, tmp_path):
    out = str(tmp_path / ("pade%d" % world))
    name = "s%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name, NTPOLY_AMD_SHM_MB="64",
                   NTPOLY_AMD_SPGEMM_FMA="1")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "pade_session_worker.py"), out],
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


def test_two_ranks(nt, tmp_path):
    """the shifted operand as column panels on two ranks sharing one GPU (shared-memory transport, FMA arithmetic), options 2, 1 and
    0 in the same processes: 2 against 1 (and 0) bit for bit on every rank, the counters of the one-rank test on every rank; the
    assembled result against the one-rank result within 100 threshold max(1, max|K|), the bound the sibling's two-rank test gives
    its solver (CG's traces are summed across ranks in another order, so bit equality with one rank is not expected: the largest
    difference is printed).  Not tested: a refusal on one rank alone"""
    n, _, _, thr, _, _, cg_iterations, _ = SOLVES["shifted"]
    two = run_world(2, tmp_path)
    for r, p in enumerate(two):
        print("rank", r, "counts (solves, sum, pair, refused)", [p["counts_%d" % v].tolist() for v in (2, 1, 0)], "cg passes",
              [int(p["passes_%d" % v][0]) for v in (2, 1, 0)])
        assert p["counts_0"].tolist() == [0, 0, 0, 0] and p["counts_1"].tolist() == [1, 0, 0, 0] and p["counts_2"].tolist() == [1, 1, 1, 0]
        for v in (2, 1, 0):
            assert int(p["passes_%d" % v][0]) == 2 * cg_iterations
        for v in (1, 0):
            assert same(srt(tuple(p["%s_2" % k] for k in ("col", "row", "val"))), srt(tuple(p["%s_%d" % (k, v)] for k in ("col", "row", "val")))), (r, v)
        # ... and under a load balancer's permutation (the reverse one): the same counters, 2 and 1 against 0 bit for bit
        print("rank", r, "with a permutation: counts", [p["lb_counts_%d" % v].tolist() for v in (2, 1, 0)])
        assert p["lb_counts_0"].tolist() == [0, 0, 0, 0] and p["lb_counts_1"].tolist() == [1, 0, 0, 0] and p["lb_counts_2"].tolist() == [1, 1, 1, 0]
        for v in (1, 0):
            assert same(srt(tuple(p["lb_%s_2" % k] for k in ("col", "row", "val"))), srt(tuple(p["lb_%s_%d" % (k, v)] for k in ("col", "row", "val")))), (r, v)
    gathered = srt(tuple(np.concatenate([p["%s_2" % k] for p in two]) for k in ("col", "row", "val")))
    before = {k: nt.get_option(k) for k in ("spgemm_fma", "pade_session")}
    try:
        nt.set_option("spgemm_fma", 1)
        nt.set_option("pade_session", 2)
        one = pade_solve(nt, nt.Matrix_ps.from_triplets(n, *solve_triplets("shifted")), n, thr)
    finally:
        for k, v in before.items():
            nt.set_option(k, v)
    assert one["counts"] == FUSED
    K1, K2 = dense(one["out"], n), dense(gathered, n)
    diff = float(np.abs(K2 - K1).max())
    print("two ranks against one: bit for bit", same(gathered, one["out"]), "max |difference|", diff, "bound", 100 * thr * max(1.0, np.abs(K1).max()))
    assert len(gathered[2]) > n
    assert diff <= 100 * thr * max(1.0, np.abs(K1).max())
    balanced = srt(tuple(np.concatenate([p["lb_%s_2" % k] for p in two]) for k in ("col", "row", "val")))
    diff = float(np.abs(dense(balanced, n) - K1).max())
    print("two ranks with a permutation against one rank without: max |difference|", diff)
    assert len(balanced[2]) > n and diff <= 100 * thr * max(1.0, np.abs(K1).max())
