"""GPU: the real Chebyshev / Hermite step in one pass and ComputeExponential's squarings in a slab session (option poly_step;
csrc/poly_step.hip k_poly_step, engine.hpp ps_poly_step).  Behind every product P = 2 X T(k-1) the recurrences make, with the
vocabulary at threshold 0,
    IncrementMatrix(T(k-2), P, a, 0)   Tk = P + a T(k-2)          IncrementMatrix(Tk, R, c, 0)   R' = R + c Tk
With the option at 2 the two merges are one pass over the runs of P, T(k-2) and R with two outputs; at 1 (and 2) ComputeExponential
squares its Chebyshev evaluation in a slab session.

The kernel is reached with crafted operands through nt.poly_step and compared with (i) the same two Increment calls on compressed
columns (slab_algebra = 0) and (ii) a numpy restatement of AddSparseVectors.f90 at threshold 0 written here, applied twice in a
chain -- never with the fused code itself.  numpy's float64 products and sums are the correctly rounded ones the kernel spells as
__dmul_rn / __dadd_rn, so patterns are compared for equality and values with np.array_equal.  The solvers are held to bit equality
between the options 2, 1 and 0: the session's products and merges have the bits of the calls on compressed columns, and the only
reduction of these calls is PowerBounds, which runs before any session opens."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from gen import banded_triplets
from golden_util import Golden, to_dense
from test_gpu_complex_poly_sessions import HERMITE, POLY

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 259   # (not a multiple of the 4 waves of a workgroup, and more than 256 rows: a second trip of the chunk loop)
KEYS = ("exp_sessions", "steps", "refused")
SCALARS = ((-1.0, 0.25), (-1.0, -1.5), (0.625, 4.0))   # (a, c): the recurrences' a = -1 with two coefficients, and a free pair
OPTIONS = ("spgemm_fma", "slab_algebra", "poly_step", "virtual_grid", "complex_poly_sessions")


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture(params=[1, 0], ids=["fma", "unfused"])
def fma(nt, request):
    """both arithmetic modes: slots padded to the tile kernel's row alignment, and runs packed back to back"""
    before = {k: nt.get_option(k) for k in OPTIONS}
    nt.set_option("spgemm_fma", request.param)
    nt.set_option("poly_step", 2)
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
EMPTY = {"P": {7, 40}, "Q": {8, 40}, "R": {9, 40}}   # empty in each input in turn; column 40 in all three
BELOW, ABOVE = 60, 150        # columns whose Q run lies wholly below (at larger rows than) / wholly above P's run
FULL = 120                    # P fills all N rows of this column: a second trip of the chunk loop
HELD, LACKED, SECOND = 30, 31, 32   # the planted columns: the first merge cancels on a row R holds / R lacks; the second merge cancels


def _runs(rng, n, empty, role):
    """{column: (rows, values)}: a run around the diagonal with half-widths 6..90 drawn per side, ~12 % holes inside, values
    log-uniform in [1e-6, 1] with a random sign"""
    cols = {}
    for j in range(n):
        if j in empty:
            continue
        f, l = max(0, j - int(rng.integers(6, 91))), min(n - 1, j + int(rng.integers(6, 91)))
        if j == BELOW and role in "PQ":
            f, l = (j - 10, j + 2) if role == "P" else (j + 3, j + int(rng.integers(30, 60)))
        elif j == ABOVE and role in "PQ":
            f, l = (j - 2, j + 10) if role == "P" else (j - int(rng.integers(30, 60)), j - 3)
        elif j == FULL and role == "P":
            f, l = 0, n - 1
        rows = np.arange(f, l + 1)
        keep = rng.random(len(rows)) > 0.12
        keep[0] = keep[-1] = True
        if role == "R":
            keep[rows == j] = True   # (R holds its diagonal: the first step's R is c0 I + c1 X)
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
    if r not in rows:
        return
    assert rows[0] < r < rows[-1], "planted rows lie inside the runs"
    cols[j] = (rows[rows != r], vals[rows != r])


def _plant(P, Q, R, a, c):
    """exact by construction (dyadic numbers) and checked here in numpy.  HELD and SECOND sit on their column's diagonal row, which
    R holds as runs and as a diagonal; LACKED one row below it, which R holds in neither"""
    q, r = 0.5, 0.375
    # HELD: a q + p == 0 on a row R holds: Tk lacks the row, R' keeps R's value
    p = -(a * q)
    assert a * q + p == 0.0
    _set(P, HELD, HELD, p)
    _set(Q, HELD, HELD, q)
    _set(R, HELD, HELD, r)
    # LACKED: a q + p == 0 on a row R lacks: the row is absent from both outputs
    _set(P, LACKED, LACKED + 1, p)
    _set(Q, LACKED, LACKED + 1, q)
    _unset(R, LACKED, LACKED + 1)
    # SECOND: c t + r == 0 with t = a q + p kept: Tk holds the row, R' lacks it
    p2 = 0.25
    t = a * q + p2
    r2 = -(c * t)
    assert t != 0.0 and (a * q + p2) * c + r2 == 0.0 and float(np.float64(c) * np.float64(t)) == c * t
    _set(P, SECOND, SECOND, p2)
    _set(Q, SECOND, SECOND, q)
    _set(R, SECOND, SECOND, r2)
    return dict(held_r=r, second_t=t)


def crafted(a, c, diagonal):
    """P, Q, R for one pair of scalars (the planted values depend on them); R as runs or as a diagonal"""
    rng = np.random.default_rng(20261021)
    P, Q = _runs(rng, N, EMPTY["P"], "P"), _runs(rng, N, EMPTY["Q"], "Q")
    R = _runs(rng, N, EMPTY["R"], "R")
    D = _diagonal(rng, N, EMPTY["R"])
    if diagonal:
        R = D
    planted = _plant(P, Q, R, a, c)
    return dict(P=P, Q=Q, R=R), planted


CASES = [(a, c, d) for a, c in SCALARS for d in (False, True)]
IDS = ["a%g_c%g_%s" % (a, c, "diagonal" if d else "runs") for a, c, d in CASES]


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
    stats["underflow"] = stats.get("underflow", 0) + int((~nz & ~(ia & ib)).sum()) + int((ia & (wa == 0.0)).sum())
    return rows[keep], s[keep]


def restated(ops, a, c, n=N):
    """(Tk, R') of the chain as {column: (rows, values)}, and the branch statistics of the two merges"""
    empty = (np.zeros(0, dtype=np.int64), np.zeros(0))
    Tk, Rn, st = {}, {}, ({}, {})
    for j in range(n):
        t = add_sparse(ops["Q"].get(j, empty), a, ops["P"].get(j, empty), st[0])   # IncrementMatrix(Q, P, a, 0)
        r = add_sparse(t, c, ops["R"].get(j, empty), st[1])                       # IncrementMatrix(Tk, R, c, 0)
        if len(t[0]):
            Tk[j] = t
        if len(r[0]):
            Rn[j] = r
    return (Tk, Rn), st


def _has(cols, j, r):
    return j in cols and r in cols[j][0]


def _at(cols, j, r):
    return cols[j][1][cols[j][0] == r][0]


@pytest.mark.parametrize("a,c,diagonal", CASES, ids=IDS)
def test_the_inputs_reach_every_branch(a, c, diagonal):
    """from the operands and the numpy restatement alone (no GPU is touched): a column empty in each input in turn and one empty in
    all three, a Q run wholly below and wholly above P's, a run that fills all N > 256 rows, columns 0 and N - 1, holes inside runs,
    both-present sums that are kept, the three planted exact cases, one-sided entries from either side in both merges; no scaled
    value is zero where an entry is held, nothing is far apart, the two outputs end with different patterns.
    More than 1000 both-present kept rows per output where R has runs; a diagonal R holds N - 2 = 257 entries, so its second merge
    can keep no more than that many both-present rows: more than 200 there."""
    o, planted = crafted(a, c, diagonal)
    P, Q, R = o["P"], o["Q"], o["R"]
    assert N % 4 != 0 and N > 256
    assert 7 not in P and 7 in Q and 7 in R and 8 not in Q and 8 in P and 8 in R and 9 not in R and 9 in P and 9 in Q
    assert all(40 not in M for M in (P, Q, R))
    assert all(0 in M and N - 1 in M for M in (P, Q, R))
    assert Q[BELOW][0][0] > P[BELOW][0][-1] and Q[ABOVE][0][-1] < P[ABOVE][0][0]
    assert P[FULL][0][0] == 0 and P[FULL][0][-1] == N - 1
    for M in (P, Q) + (() if diagonal else (R,)):
        holes = sum(int(r[-1] - r[0] + 1 - len(r)) for r, _ in M.values())
        span = sum(int(r[-1] - r[0] + 1) for r, _ in M.values())
        assert 0.08 < holes / span < 0.16, holes / span
    if diagonal:
        assert all(list(r) == [j] for j, (r, _) in R.items()) and len(R) == N - 2
    # nothing lies far apart: per column every run touches or overlaps the hull of the ones before it
    for j in range(N):
        ext = sorted((int(M[j][0][0]), int(M[j][0][-1])) for M in (P, Q, R) if j in M)
        reach = ext[0][1] if ext else 0
        for f, l in ext[1:]:
            assert f <= reach + 1, (j, ext)
            reach = max(reach, l)
    (Tk, Rn), (st1, st2) = restated(o, a, c)
    print(a, c, diagonal, st1, st2)
    for st in (st1, st2):
        assert st["underflow"] == 0
        assert st["only_a"] > 0 and st["only_b"] > 0, st
    assert st1["both_kept"] > 1000 and st2["both_kept"] > (200 if diagonal else 1000), (st1, st2)
    # the planted rows
    assert st1["cancelled"] == 2 and st2["cancelled"] == 1, (st1, st2)
    assert not _has(Tk, HELD, HELD) and _at(Rn, HELD, HELD) == planted["held_r"] == _at(R, HELD, HELD)
    assert not _has(Tk, LACKED, LACKED + 1) and not _has(Rn, LACKED, LACKED + 1) and not _has(R, LACKED, LACKED + 1)
    assert _at(Tk, SECOND, SECOND) == planted["second_t"] and not _has(Rn, SECOND, SECOND)
    assert 40 not in Tk and 40 not in Rn and 7 in Tk and 8 in Tk and 9 in Rn
    assert not np.array_equal(_triplets(Tk)[1], _triplets(Rn)[1])


@pytest.mark.parametrize("a,c,diagonal", CASES, ids=IDS)
def test_pass_bit_for_bit(nt, fma, a, c, diagonal):
    o, _ = crafted(a, c, diagonal)
    want = [_triplets(x) for x in restated(o, a, c)[0]]
    Ms = [_matrix(nt, o[k]) for k in "PQR"]
    before = [srt(m.triplets()) for m in Ms]
    # (i) the two calls on compressed columns against (ii) the restatement
    nt.set_option("slab_algebra", 0)
    VT = nt.Matrix_ps(Ms[0])
    VT.Increment(Ms[1], a, 0.0)
    VR = nt.Matrix_ps(Ms[2])
    VR.Increment(VT, c, 0.0)
    nt.set_option("slab_algebra", 1)
    V = [srt(VT.triplets()), srt(VR.triplets())]
    for q in range(2):
        assert same(V[q], want[q]), "compressed columns against the restatement, output %d" % (q + 1)
    TkOut, ROut = nt.Matrix_ps(N), nt.Matrix_ps(N)
    c0, s0 = nt.poly_step_counts(), nt.slab_algebra_counts()
    with nt.solver_session(False):
        got = nt.poly_step(Ms[0], Ms[1], Ms[2], a, c, TkOut, ROut)
        c1, s1 = nt.poly_step_counts(), nt.slab_algebra_counts()
    print("counts", c0, c1, "slab algebra", s0, s1, "entries", len(want[0][2]), len(want[1][2]))
    assert got is True
    assert delta(c0, c1) == dict(exp_sessions=0, steps=1, refused=0)
    assert s1["refusals"] == s0["refusals"]
    for M, bf in zip(Ms, before):
        assert same(srt(M.triplets()), bf), "the operands are as they were"
    for q, O in enumerate((TkOut, ROut)):
        g = srt(O.triplets())
        assert np.array_equal(g[0], want[q][0]) and np.array_equal(g[1], want[q][1]), "pattern, output %d" % (q + 1)
        assert same(g, want[q]), "values against the restatement, output %d" % (q + 1)
        assert same(g, V[q]), "values against compressed columns, output %d" % (q + 1)


# ------------------------------------------------------------------ refusals
def test_refusals_and_gates_leave_everything_as_it_was(nt, fma):
    n, j = 4099, 5
    col = lambda f, l, v=None: {j: (np.arange(f, l + 1), np.linspace(0.1, 0.9, l - f + 1) if v is None else np.asarray(v, dtype=np.float64))}

    def attempt(P, Q, R, counted, a=-1.0, c=0.25, outs=None):
        TkOut, ROut = outs if outs else (nt.Matrix_ps(n), nt.Matrix_ps(n))
        ms = [P, Q, R]
        before = [srt(m.triplets()) for m in ms]
        c0, s0 = nt.poly_step_counts(), nt.slab_algebra_counts()
        with nt.solver_session(False):
            got = nt.poly_step(P, Q, R, a, c, TkOut, ROut)
        c1, s1 = nt.poly_step_counts(), nt.slab_algebra_counts()
        assert got is False
        assert c1 == dict(c0, refused=c0["refused"] + counted), (c0, c1)
        assert s1 == s0, (s0, s1)   # (a refused pass is no operation and no refusal of the session)
        for m, bf in zip(ms, before):
            assert same(srt(m.triplets()), bf)
        if not outs:
            assert len(TkOut.triplets()[2]) == 0 and len(ROut.triplets()[2]) == 0

    mk = lambda cc: _matrix(nt, cc, n=n)
    MP, MQ, MR = mk(col(0, 9)), mk(col(4, 20)), mk(col(2, 12))
    far = mk(col(n // 2 + 1, n // 2 + 11))
    # runs n / 2 rows apart in one column, in each of the three roles: the hull is beyond what the column's slots and pads bound
    attempt(far, MQ, MR, 1)
    attempt(MP, far, MR, 1)
    attempt(MP, MQ, far, 1)
    # an input that stores a zero enters slab form as a read-only view: the pass merges no view
    view = col(0, 9)
    view[j][1][4] = 0.0
    attempt(mk(view), MQ, MR, 1)
    attempt(MP, mk(view), MR, 1)
    attempt(MP, MQ, mk(view), 1)
    # a q underflows to zero where Q alone holds the row; c t underflows where Tk alone holds it
    assert 1e-300 * 1e-300 == 0.0
    attempt(MP, mk(col(4, 20, [0.5] * 16 + [1e-300])), MR, 1, a=1e-300)
    attempt(mk(col(0, 9, [1e-300] + [0.5] * 9)), MQ, MR, 1, c=1e-300)
    # an Inf in each input
    attempt(mk(col(0, 9, [0.5] * 9 + [-np.inf])), MQ, MR, 1)
    attempt(MP, mk(col(4, 20, [0.5] * 8 + [np.inf] + [0.5] * 8)), MR, 1)
    attempt(MP, MQ, mk(col(2, 12, [0.5] * 5 + [np.inf] + [0.5] * 5)), 1)
    # gated, counted nowhere: one matrix given twice, an output that is an input, one output handle for both, a complex input,
    # a zero scalar, the option below 2
    attempt(MP, MP, MR, 0)
    attempt(MP, MQ, MP, 0)
    attempt(MP, MQ, MQ, 0)
    attempt(MP, MQ, MR, 0, outs=(MP, nt.Matrix_ps(n)))
    attempt(MP, MQ, MR, 0, outs=(nt.Matrix_ps(n), MR))
    attempt(MP, MQ, MR, 0, outs=(MQ, nt.Matrix_ps(n)))
    O = nt.Matrix_ps(n)
    attempt(MP, MQ, MR, 0, outs=(O, O))
    MC = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, 3, complex_=True))
    attempt(MC, MQ, MR, 0)
    attempt(MP, MC, MR, 0)
    attempt(MP, MQ, MC, 0)
    attempt(MP, MQ, MR, 0, a=0.0)
    attempt(MP, MQ, MR, 0, c=0.0)
    for below in (1, 0):
        nt.set_option("poly_step", below)
        attempt(MP, MQ, MR, 0)
    nt.set_option("poly_step", 2)
    # the same column with the runs side by side IS taken: against a dense numpy chain (adding an absent entry as 0.0 gives the
    # merge's values)
    p, q, r = np.zeros(21), np.zeros(21), np.zeros(21)
    p[0:10], q[4:21], r[2:13] = np.linspace(0.1, 0.9, 10), np.linspace(0.1, 0.9, 17), np.linspace(0.1, 0.9, 11)
    for a, c in SCALARS:
        TkOut, ROut = nt.Matrix_ps(n), nt.Matrix_ps(n)
        c0 = nt.poly_step_counts()
        with nt.solver_session(False):
            got = nt.poly_step(MP, MQ, MR, a, c, TkOut, ROut)
        assert got is True and delta(c0, nt.poly_step_counts()) == dict(exp_sessions=0, steps=1, refused=0)
        t = a * q + p
        o = c * t + r
        for O, d in ((TkOut, t), (ROut, o)):
            kept = np.flatnonzero(d != 0.0)
            assert len(kept) >= 19
            cc, rr, vv = srt(O.triplets())
            assert np.all(cc == j + 1) and np.array_equal(rr, kept + 1) and np.array_equal(vv, d[kept])


# ------------------------------------------------------------------ the solvers
# name: (n, half bandwidth, shift, threshold, squarings of ComputeExponential)
SOLVES = {"shifted": (259, 8, 2.0, 1e-9, 2), "wide": (400, 20, 0.0, 1e-12, 1)}
NONE = dict.fromkeys(KEYS, 0)


def solve_triplets(name, c0=0, c1=None):
    n, h, shift = SOLVES[name][:3]
    return banded_triplets(n, h, shift=shift, c0=c0, c1=c1)


def dense(t, n):
    M = np.zeros((n, n), dtype=np.asarray(t[2]).dtype)
    M[t[1] - 1, t[0] - 1] = t[2]
    return M


@pytest.mark.parametrize("name", sorted(SOLVES))
def test_the_exponential_operands_in_numpy(name):
    """no GPU is touched: the spectral radius (dense eigvalsh) of each operand lies at least 5 % away from a power of two, so
    PowerBounds' estimate chooses the same scaling whatever its last digits are and the number of squarings is fixed: 2 on the
    shifted operand (radius 3.17).  The wide operand's radius is 1.67: it has ONE squaring, which is asserted as such -- the
    hand-over into the squarings' session is the same, the second trip of the loop is the shifted operand's"""
    n, _, _, _, squarings = SOLVES[name]
    A = dense(solve_triplets(name), n)
    assert np.array_equal(A, A.T)
    radius = float(np.abs(np.linalg.eigvalsh(A)).max())
    power = 2.0 ** np.round(np.log2(radius))
    s, counter = 1.0, 1
    while radius / s > 1.0:
        s *= 2
        counter += 1
    print(name, "spectral radius", radius, "nearest power of two", power, "sigma", s, "squarings", counter - 1)
    assert abs(radius - power) >= 0.05 * power
    assert counter - 1 == squarings
    if name == "shifted":
        assert squarings >= 2


def run_solver(nt, kind, A, n, thr, perm=None):
    p = nt.SolverParameters()
    p.SetThreshold(thr)
    if perm is not None:
        p.SetLoadBalance(perm)
    Out = nt.Matrix_ps(n)
    c0, s0, r0 = nt.poly_step_counts(), nt.slab_algebra_counts(), nt.recurrence_step_count()
    if kind == "exp":
        nt.ExponentialSolvers.ComputeExponential(A, Out, p)
    else:
        coef = POLY if kind == "cheby" else HERMITE
        poly = (nt.ChebyshevPolynomial if kind == "cheby" else nt.HermitePolynomial)(len(coef))
        for k, v in enumerate(coef):
            poly.SetCoefficient(k, v)
        poly.Compute(A, Out, p)
    c1, s1, r1 = nt.poly_step_counts(), nt.slab_algebra_counts(), nt.recurrence_step_count()
    return dict(out=srt(Out.triplets()), counts=delta(c0, c1), slab=delta(s0, s1), recurrence=r1 - r0)


def expected_counts(kind, option):
    if option == 0:
        return NONE
    if kind == "exp":
        return dict(exp_sessions=1, steps=14 if option == 2 else 0, refused=0)
    steps = len(POLY if kind == "cheby" else HERMITE) - 2
    return dict(exp_sessions=0, steps=steps if option == 2 else 0, refused=0)


def three_options(nt, kind, A, n, thr, perm=None, tag=""):
    runs = {}
    for v in (2, 1, 0):
        nt.set_option("poly_step", v)
        runs[v] = run_solver(nt, kind, A, n, thr, perm=perm)
        print(tag, kind, "option", v, "counts", runs[v]["counts"], "slab algebra", runs[v]["slab"], "entries", len(runs[v]["out"][2]))
    nt.set_option("poly_step", 2)
    assert np.isfinite(runs[0]["out"][2]).all() and len(runs[0]["out"][2]) > n
    for v in (1, 2):
        first = ("pattern" if not (np.array_equal(runs[v]["out"][0], runs[0]["out"][0]) and np.array_equal(runs[v]["out"][1], runs[0]["out"][1]))
                 else "values")
        assert same(runs[v]["out"], runs[0]["out"]), "option %d against 0: %s differ" % (v, first)
    return runs


@pytest.mark.parametrize("kind", ("cheby", "hermite", "exp"))
@pytest.mark.parametrize("name", sorted(SOLVES))
def test_solvers_2_against_1_against_0(nt, fma, name, kind):
    """the result equal in pattern and bits across the options 2, 1 and 0, and the counters of each option; for the exponential
    the session products with the option at 1 and 2 are those of option 0 (the evaluation's) plus the squarings, on the sparse operand"""
    n, _, _, thr, squarings = SOLVES[name]
    A = nt.Matrix_ps.from_triplets(n, *solve_triplets(name))
    runs = three_options(nt, kind, A, n, thr, tag=name)
    for v in (2, 1, 0):
        assert runs[v]["counts"] == expected_counts(kind, v), (v, runs[v]["counts"])
    if kind == "exp" and name == "shifted":   # (the wide operand's exponential is 82 % full: its squaring is a dense product, which no session counts)
        for v in (1, 2):
            assert runs[v]["slab"]["products"] - runs[0]["slab"]["products"] == squarings, (v, runs[v]["slab"], runs[0]["slab"], squarings)


def balance_lookup(n):
    """a fixed permutation for the load balancer, the same in every process: 1-based, seeded"""
    return (np.random.default_rng(20261021).permutation(n) + 1).astype(np.int32)


@pytest.mark.parametrize("kind", ("cheby", "exp"))
@pytest.mark.parametrize("perm_kind", ("reverse", "seeded"))
def test_solvers_with_a_load_balancer_permutation(nt, fma, perm_kind, kind):
    """`reverse` keeps the band: the counters of the plain run (the exponential's result is packed, un-permuted, permuted and
    re-enters the squarings' session once).  `seeded` scatters it: the operands are not run-like, no step is fused; the other
    counters are printed only.  2, 1 and 0 bit for bit either way"""
    n, _, _, thr, _ = SOLVES["shifted"]
    A = nt.Matrix_ps.from_triplets(n, *solve_triplets("shifted"))
    perm = nt.Permutation(n)
    if perm_kind == "reverse":
        perm.SetReversePermutation()
    else:
        perm.set_lookup(balance_lookup(n))
    runs = three_options(nt, kind, A, n, thr, perm=perm, tag=perm_kind)
    assert runs[0]["counts"] == NONE
    for v in (2, 1):
        if perm_kind == "reverse":
            assert runs[v]["counts"] == expected_counts(kind, v), (v, runs[v]["counts"])
        else:
            assert runs[v]["counts"]["steps"] == 0, (v, runs[v]["counts"])


def test_gates_at_solver_level(nt, fma):
    """a complex operand, slab_algebra = 0 and a grid with two process slices fuse nothing, open no session of this option and
    refuse nothing: the result of option 0 bit for bit, the counters untouched; the complex loops' own fused step counts as it
    does with the option at 0.  An operand that stores a zero on its diagonal gives option 0's result whatever path it takes"""
    n, h, shift, thr, _ = SOLVES["shifted"]

    def pair(kind, A):
        nt.set_option("poly_step", 2)
        a = run_solver(nt, kind, A, n, thr)
        nt.set_option("poly_step", 0)
        b = run_solver(nt, kind, A, n, thr)
        nt.set_option("poly_step", 2)
        return a, b

    def untouched(kind, A):
        a, b = pair(kind, A)
        assert a["counts"] == NONE == b["counts"], (kind, a["counts"], b["counts"])
        assert same(a["out"], b["out"]) and len(a["out"][2]) > n
        return a, b

    AC = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, h, complex_=True, shift=shift))
    for kind in ("cheby", "hermite", "exp"):
        a, b = untouched(kind, AC)
        print("complex", kind, "fused complex steps", a["recurrence"], b["recurrence"])
        assert a["recurrence"] == b["recurrence"]
    AR = nt.Matrix_ps.from_triplets(n, *solve_triplets("shifted"))
    nt.set_option("slab_algebra", 0)
    for kind in ("cheby", "exp"):
        untouched(kind, AR)
    nt.set_option("slab_algebra", 1)
    nt.set_option("virtual_grid", 1)
    try:
        nt.ConstructGlobalProcessGrid(1, 1, 2)
        AS = nt.Matrix_ps.from_triplets(n, *solve_triplets("shifted"))
        for kind in ("cheby", "exp"):
            untouched(kind, AS)
    finally:
        nt.ConstructGlobalProcessGrid(1, 1, 1)
        nt.set_option("virtual_grid", 0)
    c, r, v = solve_triplets("shifted")
    v = v.copy()
    v[(c == 101) & (r == 101)] = 0.0
    assert np.count_nonzero(v == 0.0) == 1
    Z = nt.Matrix_ps.from_triplets(n, c, r, v)
    assert len(Z.triplets()[2]) == len(v)
    for kind in ("cheby", "hermite", "exp"):
        a, b = pair(kind, Z)
        print("stored zero:", kind, "counts", a["counts"], "slab algebra", a["slab"])
        assert b["counts"] == NONE and same(a["out"], b["out"]) and len(a["out"][2]) > n


# ------------------------------------------------------------------ golden
def _golden_diff(want, out):
    gd = to_dense((want[0], want[1]) + tuple(out))
    wd = to_dense(want)
    return float(np.abs(gd - wd).max()), float(max(1.0, np.abs(wd).max()))


def test_golden_polynomials_with_the_option(nt, fma):
    """the real `cheby` and `hermite` cases of tests/golden/polynomials.npz with the option at 1 and 2 against the reference's
    results, in the bound tests/test_gpu_extras.py gives them: max(100 thr, 1e-12) max(1, max|K|)"""
    g = Golden("polynomials")
    t = g.tri(None, "A0")
    A = nt.Matrix_ps.from_triplets(t[0], t[2], t[3], t[4])
    n = t[0]
    hits = [(i, c) for i, c in enumerate(g.cases) if c["kind"] in ("cheby", "hermite") and not c["complex"]]
    assert len(hits) >= 2
    fused = 0
    for i, c in hits:
        for v in (1, 2):
            nt.set_option("poly_step", v)
            p = nt.SolverParameters()
            p.SetThreshold(c["thr"])
            poly = (nt.ChebyshevPolynomial if c["kind"] == "cheby" else nt.HermitePolynomial)(len(c["coef"]))
            for k, x in enumerate(c["coef"]):
                poly.SetCoefficient(k, x)
            Out = nt.Matrix_ps(n)
            c0 = nt.poly_step_counts()
            poly.Compute(A, Out, p)
            d = delta(c0, nt.poly_step_counts())
            diff, scale = _golden_diff(g.tri(i, "K"), Out.triplets())
            print(i, c["kind"], "degree", len(c["coef"]) - 1, "thr", c["thr"], "option", v, "counts", d, "max |K - K_ref|", diff, "bound",
                  max(100 * c["thr"], 1e-12) * scale)
            assert diff <= max(100 * c["thr"], 1e-12) * scale, (i, c["kind"], v, diff)
            assert d["exp_sessions"] == 0 and (v == 2 or d["steps"] == 0)
            fused += d["steps"]
    nt.set_option("poly_step", 2)
    assert fused > 0


def test_golden_exponential_with_the_option(nt, fma):
    """the real `exp` cases of tests/golden/functions.npz with the option at 1 and 2: max(1000 thr, 1e-11) max(1, max|K|)"""
    g = Golden("functions")
    hits = [(i, c) for i, c in enumerate(g.cases) if c["kind"] == "exp" and c["matrix"] != "csym"]
    assert len(hits) >= 1
    mats = {}
    for i, c in hits:
        if c["matrix"] not in mats:
            t = g.tri(None, "M_" + c["matrix"])
            mats[c["matrix"]] = (nt.Matrix_ps.from_triplets(t[0], t[2], t[3], t[4]), t[0])
        A, n = mats[c["matrix"]]
        for v in (1, 2):
            nt.set_option("poly_step", v)
            p = nt.SolverParameters()
            p.SetThreshold(c["thr"])
            p.SetConvergeDiff(c["conv"])
            Out = nt.Matrix_ps(n)
            c0 = nt.poly_step_counts()
            nt.ExponentialSolvers.ComputeExponential(A, Out, p)
            d = delta(c0, nt.poly_step_counts())
            diff, scale = _golden_diff(g.tri(i, "K"), Out.triplets())
            print(i, c["matrix"], "thr", c["thr"], "option", v, "counts", d, "max |K - K_ref|", diff, "bound", max(1000 * c["thr"], 1e-11) * scale)
            assert d["exp_sessions"] == 1
            assert diff <= max(1000 * c["thr"], 1e-11) * scale, (i, v, diff)
    nt.set_option("poly_step", 2)


# ------------------------------------------------------------------ two ranks
def run_world(world, tmp_path):
    out = str(tmp_path / ("poly%d" % world))
    name = "s%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name, NTPOLY_AMD_SHM_MB="64",
                   NTPOLY_AMD_SPGEMM_FMA="1")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "poly_step_worker.py"), out],
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
    """the shifted operand as column panels on two ranks sharing one GPU (shared-memory transport, FMA arithmetic), Chebyshev and
    the exponential with options 2, 1 and 0 in the same processes: 2 against 1 against 0 bit for bit on every rank, the counters
    of the one-rank test on every rank (each panel makes its own pass); the assembled result against the one-rank result within
    100 threshold max(1, max|K|), the bound the sibling's two-rank test gives (whether it is bit for bit is printed).
    Not tested: a refusal on one rank alone"""
    n, _, _, thr, _ = SOLVES["shifted"]
    two = run_world(2, tmp_path)
    before = {k: nt.get_option(k) for k in ("spgemm_fma", "poly_step")}
    try:
        nt.set_option("spgemm_fma", 1)
        nt.set_option("poly_step", 2)
        A = nt.Matrix_ps.from_triplets(n, *solve_triplets("shifted"))
        for kind in ("cheby", "exp"):
            for r, p in enumerate(two):
                print("rank", r, kind, "counts (exp_sessions, steps, refused)", [p["%s_counts_%d" % (kind, v)].tolist() for v in (2, 1, 0)])
                for v in (2, 1, 0):
                    assert p["%s_counts_%d" % (kind, v)].tolist() == [expected_counts(kind, v)[k] for k in KEYS], (r, kind, v)
                for v in (1, 0):
                    assert same(srt(tuple(p["%s_%s_2" % (kind, k)] for k in ("col", "row", "val"))),
                                srt(tuple(p["%s_%s_%d" % (kind, k, v)] for k in ("col", "row", "val")))), (r, kind, v)
            gathered = srt(tuple(np.concatenate([p["%s_%s_2" % (kind, k)] for p in two]) for k in ("col", "row", "val")))
            one = run_solver(nt, kind, A, n, thr)
            assert one["counts"] == expected_counts(kind, 2)
            K1, K2 = dense(one["out"], n), dense(gathered, n)
            diff = float(np.abs(K2 - K1).max())
            print(kind, "two ranks against one: bit for bit", same(gathered, one["out"]), "max |difference|", diff, "bound",
                  100 * thr * max(1.0, np.abs(K1).max()))
            assert len(gathered[2]) > n
            assert diff <= 100 * thr * max(1.0, np.abs(K1).max())
    finally:
        for k, v in before.items():
            nt.set_option(k, v)
