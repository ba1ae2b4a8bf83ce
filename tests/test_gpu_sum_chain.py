"""GPU: the scaled sum chain of the real solver loops in one pass (option sum_chain; csrc/sum_chain.hip k_sum_chain<M>, engine.hpp
ps_sum_chain).  Sine / Cosine, the Paterson-Stockmeyer evaluation, the factorized Chebyshev evaluation (and ComputeLogarithm
through it) and the inverse-root iteration (ComputeInverseRoot, ComputeRoot, ComputeLogarithm) build, with the vocabulary at
threshold 0,
    CopyMatrix(Base, Out); ScaleMatrix(Out, s); IncrementMatrix(A_k, Out, c_k, 0) for k = 1..M; [ScaleMatrix(Out, post)]
With the option at 1 such a sequence is one pass over the runs of Base and the addends.

The kernel is reached with crafted operands through nt.sum_chain and compared with (i) the same vocabulary calls on compressed
columns (slab_algebra = 0) and (ii) a numpy restatement of AddSparseVectors.f90 at threshold 0 written here, applied M times in a
chain -- never with the fused code itself.  numpy's float64 products and sums are the correctly rounded ones the kernel spells as
__dmul_rn / __dadd_rn, so patterns are compared for equality and values with np.array_equal.  The solvers are held to bit equality
between the options 1 and 0: the pass and the calls it replaces are local and enter no reduction."""
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
N = 259   # (not a multiple of the 4 waves of a workgroup, and more than 256 rows: a second trip of the chunk loop)
KEYS = ("passes", "refused")
OPTIONS = ("spgemm_fma", "slab_algebra", "sum_chain", "virtual_grid")
# M: (s, coefficients) -- the doubling's 2 R - I, the Chebyshev combine's s = 1, and two free sets; all dyadic, so that the planted
# cancellations are exact
SCALARS = {1: (2.0, [-1.0]), 2: (1.0, [1.0, -0.25]), 3: (-1.5, [0.25, -1.0, 0.375]), 5: (0.75, [0.25, -1.0, 0.625, 4.0, -0.5])}
POST = 1.0 / 3.0   # (the inverse-root iteration's 1 / t is no dyadic number)


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
    nt.set_option("sum_chain", 1)
    yield request.param
    for k, v in before.items():
        nt.set_option(k, v)


def srt(t):
    c, r, v = t
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def same(a, b):
    """sorted triplets: equal patterns, equal values (a NaN the refusal test plants equals itself)"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2], equal_nan=True)


def delta(c0, c1):
    return {k: c1[k] - c0[k] for k in c1}


# ------------------------------------------------------------------ operands
# a column is (rows, values); role 0 is Base, role k the addend k
EMPTY_ALL = 40                # empty in every role; role q is empty in column 7 + q
BELOW, ABOVE = 60, 150        # columns whose A_1 run lies wholly below (at larger rows than) / wholly above Base's run
FULL = 120                    # Base fills all N rows of this column: a second trip of the chunk loop
BACK, LAST, ONLY = 30, 31, 32   # the planted columns, each on its diagonal row: (a) cancels at A_1 and is brought back by A_2 (M >= 2);
#                                 (b) cancels at the last addend; (c) only the last addend holds the row


def _runs(rng, n, role):
    """{column: (rows, values)}: a run around the diagonal with half-widths 6..90 drawn per side, ~12 % holes inside (never on the
    diagonal), values log-uniform in [1e-6, 1] with a random sign"""
    cols = {}
    for j in range(n):
        if j == EMPTY_ALL or j == 7 + role:
            continue
        f, l = max(0, j - int(rng.integers(6, 91))), min(n - 1, j + int(rng.integers(6, 91)))
        if j == BELOW and role <= 1:
            f, l = (j - 10, j + 2) if role == 0 else (j + 3, j + int(rng.integers(30, 60)))
        elif j == ABOVE and role <= 1:
            f, l = (j - 2, j + 10) if role == 0 else (j - int(rng.integers(30, 60)), j - 3)
        elif j == FULL and role == 0:
            f, l = 0, n - 1
        rows = np.arange(f, l + 1)
        keep = rng.random(len(rows)) > 0.12
        keep[0] = keep[-1] = True
        keep[rows == j] = True
        rows = rows[keep]
        cols[j] = (rows, 10.0 ** rng.uniform(-6.0, 0.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows)))
    return cols


def _diagonal(rng, n, role):
    """one entry per column, on the diagonal row: what the identity is in slab form"""
    return {j: (np.array([j]), 10.0 ** rng.uniform(-1.0, 0.0, 1)) for j in range(n) if j != EMPTY_ALL and j != 7 + role}


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
    if len(rows) == 1:   # (a diagonal operand: the column becomes empty)
        del cols[j]
        return
    assert rows[0] < r < rows[-1], "planted rows lie inside the runs"
    cols[j] = (rows[rows != r], vals[rows != r])


def crafted(M, ident):
    """Base and A_1..A_M for the scalars of M; ident: None, "base" (Base is a diagonal) or "last" (A_M is).  The planted values are
    exact by construction (dyadic numbers) and checked in test_the_inputs_reach_every_branch"""
    s, c = SCALARS[M]
    rng = np.random.default_rng(20261021)
    ops = [_runs(rng, N, q) for q in range(M + 1)]
    diag = [_diagonal(rng, N, q) for q in range(M + 1)]
    if ident == "base":
        ops[0] = diag[0]
        for r in (BELOW + 1, BELOW + 2):   # (A_1's runs reach the one row Base holds there: nothing lies far apart)
            _set(ops[1], BELOW, r, 0.3)
        for r in (ABOVE - 2, ABOVE - 1):
            _set(ops[1], ABOVE, r, 0.3)
    elif ident == "last":
        ops[M] = diag[M]
    b = 0.5
    if M >= 2:
        # (a) s b + c_1 a_1 == 0 on a row A_2 holds: absent behind A_1, back behind A_2 with the value c_2 a_2
        _set(ops[0], BACK, BACK, b)
        _set(ops[1], BACK, BACK, -(s * b) / c[0])
        _set(ops[2], BACK, BACK, 0.375)
    # (b) only Base and A_M hold the row, s b + c_M a_M == 0: absent from the result
    _set(ops[0], LAST, LAST, b)
    for q in range(1, M):
        _unset(ops[q], LAST, LAST)
    _set(ops[M], LAST, LAST, -(s * b) / c[M - 1])
    # (c) only A_M holds the row: the result holds post c_M a_M
    for q in range(M):
        _unset(ops[q], ONLY, ONLY)
    _set(ops[M], ONLY, ONLY, 0.625)
    return ops


CASES = [(M, post, inplace) for M in sorted(SCALARS) for post in (1.0, POST) for inplace in (True, False)]
IDENT = {(1, True): None, (1, False): "base", (2, True): "last", (2, False): None, (3, True): "base", (3, False): None, (5, True): None,
         (5, False): "last"}   # (M, in place): which operand is a diagonal; both kinds with and without `post`
IDS = ["M%d_%s_%s" % (M, "post" if post != 1.0 else "nopost", "inplace" if inplace else "fresh") for M, post, inplace in CASES]


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


def restated(ops, s, c, post, n=N, trace=None):
    """the chain as {column: (rows, values)} and the branch statistics of the copy-and-scale, each merge and the trailing scaling;
    trace = (column, row): the value of that row behind every step (None where it is absent)"""
    empty = (np.zeros(0, dtype=np.int64), np.zeros(0))
    out, st, seen = {}, [{} for _ in range(len(c) + 2)], []

    def look(v):
        if trace and j == trace[0]:
            seen.append(float(v[1][v[0] == trace[1]][0]) if trace[1] in v[0] else None)

    for j in range(n):
        rows, vals = ops[0].get(j, empty)
        v = (rows, s * vals)   # CopyMatrix; ScaleMatrix
        st[0]["underflow"] = st[0].get("underflow", 0) + int((v[1] == 0.0).sum())
        look(v)
        for k, ck in enumerate(c):
            v = add_sparse(ops[k + 1].get(j, empty), ck, v, st[k + 1])   # IncrementMatrix(A_k, Out, c_k, 0)
            look(v)
        if post != 1.0:
            v = (v[0], post * v[1])
            st[-1]["underflow"] = st[-1].get("underflow", 0) + int((v[1] == 0.0).sum())
        if len(v[0]):
            out[j] = v
    return out, st, seen


def _has(cols, j, r):
    return j in cols and r in cols[j][0]


def _at(cols, j, r):
    return cols[j][1][cols[j][0] == r][0]


@pytest.mark.parametrize("M,post,inplace", CASES, ids=IDS)
def test_the_inputs_reach_every_branch(M, post, inplace):
    """from the operands and the numpy restatement alone (no GPU is touched): a column empty in each role in turn and one empty in
    all, an A_1 run wholly below and wholly above Base's, a run that fills all N > 256 rows, columns 0 and N - 1, holes inside runs,
    an operand with one entry per column, both-present sums that are kept in every merge, one-sided entries from either side in
    every merge, the planted rows (a) cancelled at A_1 and brought back by A_2, (b) cancelled at the last addend, (c) held by the
    last addend only; no scaled value is zero where an entry is held and nothing is far apart"""
    ident = IDENT[M, inplace]
    s, c = SCALARS[M]
    ops = crafted(M, ident)
    assert N % 4 != 0 and N > 256
    for q in range(M + 1):
        assert 7 + q not in ops[q] and all(7 + q in ops[p] for p in range(M + 1) if p != q)
        assert EMPTY_ALL not in ops[q] and 0 in ops[q] and N - 1 in ops[q]
    if ident != "base":
        assert ops[1][BELOW][0][0] > ops[0][BELOW][0][-1] and ops[1][ABOVE][0][-1] < ops[0][ABOVE][0][0]
        assert ops[0][FULL][0][0] == 0 and ops[0][FULL][0][-1] == N - 1
    diagonal = {"base": 0, "last": M}.get(ident)
    for q in range(M + 1):
        if q == diagonal:
            assert all(list(r) == [j] for j, (r, _) in ops[q].items()) and len(ops[q]) >= N - 3
            continue
        holes = sum(int(r[-1] - r[0] + 1 - len(r)) for r, _ in ops[q].values())
        span = sum(int(r[-1] - r[0] + 1) for r, _ in ops[q].values())
        assert 0.08 < holes / span < 0.16, holes / span
    # nothing lies far apart: per column every run touches or overlaps the hull of the ones before it
    for j in range(N):
        ext = sorted((int(o[j][0][0]), int(o[j][0][-1])) for o in ops if j in o)
        reach = ext[0][1] if ext else 0
        for f, l in ext[1:]:
            assert f <= reach + 1, (j, ext)
            reach = max(reach, l)
    out, st, _ = restated(ops, s, c, post)
    print(M, post, ident, st)
    assert all(x.get("underflow", 0) == 0 for x in st)
    for k in range(1, M + 1):
        assert st[k]["only_a"] > 0 and st[k]["only_b"] > 0, (k, st[k])
        assert st[k]["both_kept"] > (200 if diagonal in (0, k) else 1000), (k, st[k])
    # the planted rows
    want_cancelled = [0] * (M + 1)
    want_cancelled[M] += 1
    b = 0.5
    if M >= 2:
        want_cancelled[1] += 1
        seen = restated(ops, s, c, post, trace=(BACK, BACK))[2]
        assert seen[0] == s * b and seen[1] is None and seen[2] == c[1] * 0.375, seen
        assert _has(out, BACK, BACK)
    assert [st[k]["cancelled"] for k in range(1, M + 1)] == want_cancelled[1:], st
    seen = restated(ops, s, c, post, trace=(LAST, LAST))[2]
    assert all(x == s * b for x in seen[:M]) and seen[M] is None, seen
    assert not _has(out, LAST, LAST)
    seen = restated(ops, s, c, post, trace=(ONLY, ONLY))[2]
    assert all(x is None for x in seen[:M]) and seen[M] == c[M - 1] * 0.625, seen
    assert _at(out, ONLY, ONLY) == post * (c[M - 1] * 0.625)
    assert EMPTY_ALL not in out and all(7 + q in out for q in range(M + 1))


@pytest.mark.parametrize("M,post,inplace", CASES, ids=IDS)
def test_pass_bit_for_bit(nt, fma, M, post, inplace):
    s, c = SCALARS[M]
    ops = crafted(M, IDENT[M, inplace])
    want = _triplets(restated(ops, s, c, post)[0])
    Ms = [_matrix(nt, o) for o in ops]
    before = [srt(m.triplets()) for m in Ms]
    # (i) the calls on compressed columns against (ii) the restatement
    nt.set_option("slab_algebra", 0)
    V = nt.Matrix_ps(Ms[0])
    if s != 1.0:
        V.Scale(s)
    for k in range(M):
        V.Increment(Ms[k + 1], c[k], 0.0)
    if post != 1.0:
        V.Scale(post)
    nt.set_option("slab_algebra", 1)
    V = srt(V.triplets())
    assert same(V, want), "compressed columns against the restatement"
    Out = Ms[0] if inplace else nt.Matrix_ps(N)
    c0, s0 = nt.sum_chain_counts(), nt.slab_algebra_counts()
    with nt.solver_session(False):
        got = nt.sum_chain(Ms[0], s, Ms[1:], c, post, Out)
        c1, s1 = nt.sum_chain_counts(), nt.slab_algebra_counts()
    print("counts", c0, c1, "slab algebra", s0, s1, "entries", len(want[2]))
    assert got is True
    assert delta(c0, c1) == dict(passes=1, refused=0)
    assert s1["refusals"] == s0["refusals"]
    for m, bf in list(zip(Ms, before))[1 if inplace else 0:]:
        assert same(srt(m.triplets()), bf), "the operands are as they were"
    g = srt(Out.triplets())
    assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]), "pattern"
    assert same(g, want), "values against the restatement"
    assert same(g, V), "values against compressed columns"


# ------------------------------------------------------------------ refusals
def test_refusals_and_gates_leave_everything_as_it_was(nt, fma):
    n, j = 4099, 5
    col = lambda f, l, v=None: {j: (np.arange(f, l + 1), np.linspace(0.1, 0.9, l - f + 1) if v is None else np.asarray(v, dtype=np.float64))}

    def attempt(B, As, counted, s=2.0, c=None, post=1.0, out=None):
        Out = out if out is not None else nt.Matrix_ps(n)
        c = [0.25, -1.0, 0.625, 4.0, -0.5, 1.5][:len(As)] if c is None else c
        ms = [B] + list(As) + ([Out] if out is not None else [])
        before = [srt(m.triplets()) for m in ms]
        c0, s0 = nt.sum_chain_counts(), nt.slab_algebra_counts()
        with nt.solver_session(False):
            got = nt.sum_chain(B, s, As, c, post, Out)
        c1, s1 = nt.sum_chain_counts(), nt.slab_algebra_counts()
        assert got is False
        assert c1 == dict(c0, refused=c0["refused"] + counted), (c0, c1)
        assert s1 == s0, (s0, s1)   # (a refused pass is no operation and no refusal of the session)
        for m, bf in zip(ms, before):
            assert same(srt(m.triplets()), bf)
        if out is None:
            assert len(Out.triplets()[2]) == 0

    mk = lambda cc: _matrix(nt, cc, n=n)
    MB, M1, M2 = mk(col(0, 9)), mk(col(4, 20)), mk(col(2, 12))
    far = mk(col(n // 2 + 1, n // 2 + 11))
    # runs n / 2 rows apart in one column, in each role: the hull is beyond what the column's slots and pads bound
    attempt(far, [M1, M2], 1)
    attempt(MB, [far], 1)
    attempt(MB, [M1, far], 1)
    # a product that underflows to zero where an entry is held: c_k a_k where the addend alone holds the row and where both do,
    # s base, and the trailing scaling
    assert 1e-200 * 1e-200 == 0.0
    attempt(MB, [mk(col(4, 20, [0.5] * 16 + [1e-200]))], 1, c=[1e-200])
    attempt(MB, [M2, mk(col(4, 20, [1e-200] + [0.5] * 16))], 1, c=[0.25, 1e-200])
    attempt(mk(col(0, 9, [1e-200] + [0.5] * 9)), [M1], 1, s=1e-200)
    attempt(mk(col(0, 9, [1e-200] + [0.5] * 9)), [M1], 1, s=1.0, post=1e-200)
    # an entry that is not finite, in each role
    attempt(mk(col(0, 9, [0.5] * 9 + [np.nan])), [M1], 1)
    attempt(MB, [mk(col(4, 20, [0.5] * 8 + [np.nan] + [0.5] * 8))], 1)
    attempt(MB, [M1, mk(col(2, 12, [0.5] * 5 + [np.inf] + [0.5] * 5))], 1)
    # an input that stores a zero enters slab form as a read-only view: the pass merges no view
    view = col(0, 9)
    view[j][1][4] = 0.0
    attempt(mk(view), [M1], 1)
    attempt(MB, [mk(view)], 1)
    # gated, counted nowhere: the option at 0, a zero or non-finite scalar, six addends, Out an addend, one matrix twice, a
    # complex operand
    nt.set_option("sum_chain", 0)
    attempt(MB, [M1, M2], 0)
    nt.set_option("sum_chain", 1)
    attempt(MB, [M1, M2], 0, c=[0.25, 0.0])
    attempt(MB, [M1, M2], 0, s=0.0)
    attempt(MB, [M1, M2], 0, post=0.0)
    attempt(MB, [M1, M2], 0, post=np.inf)
    six = [mk(col(k, 12 + k)) for k in range(6)]
    attempt(MB, six, 0)
    attempt(MB, [M1, M2], 0, out=M2)
    attempt(MB, [M1, M1], 0)
    attempt(MB, [MB], 0)
    attempt(MB, [M1, MB], 0, out=MB)
    MC = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, 3, complex_=True))
    attempt(MC, [M1], 0)
    attempt(MB, [M1, MC], 0)
    # the same column with the runs side by side IS taken, five addends of them: against a dense numpy chain (adding an absent
    # entry as 0.0 gives the merge's values)
    dense_col = lambda M: np.bincount(M.triplets()[1] - 1, weights=M.triplets()[2], minlength=40)[:40]
    for post in (1.0, POST):
        s, c = SCALARS[5]
        Out = nt.Matrix_ps(n)
        c0 = nt.sum_chain_counts()
        with nt.solver_session(False):
            got = nt.sum_chain(MB, s, six[:5], c, post, Out)
        assert got is True and delta(c0, nt.sum_chain_counts()) == dict(passes=1, refused=0)
        d = s * dense_col(MB)
        for k in range(5):
            d = c[k] * dense_col(six[k]) + d
        d = post * d if post != 1.0 else d
        kept = np.flatnonzero(d != 0.0)
        assert len(kept) >= 17
        cc, rr, vv = srt(Out.triplets())
        assert np.all(cc == j + 1) and np.array_equal(rr, kept + 1) and np.array_equal(vv, d[kept])


# ------------------------------------------------------------------ the solvers
THR = 1e-9
# The inverse-root loop's Mk starts at A^(1/4) / e_max^t and the solver's threshold is absolute: above that scale the first product
# empties Mk, which no slab form holds (the pass is then refused, the calls run on compressed columns, and the result is a multiple
# of the identity).  ComputeRoot(5) iterates on A^4, whose Mk starts near 1e-21 at shift 6: threshold 1e-25.  The inverse roots at
# 1e-6 stay narrow enough for the unfused products of the session at n = 1024; everything else at 1e-9
THRESHOLDS = {"invroot5": 1e-6, "invroot6": 1e-6, "root5": 1e-25}
# the inverse-root loop runs exactly this many iterations (run_solver).  30 let the inverse roots and 60 the logarithm's root
# converge (the iterate starts at I / e_max and first grows by (t + 1) / t per iteration; a converged iterate stays where it is).
# ComputeRoot(5) would need 60 as well, but without a threshold that bites its iterates fill the matrix, and in unfused arithmetic
# the session of the loop gives up on such products (with the option at 0 too) after 41 to 50 iterations, measured at shifts 3.5
# and 6: 30 iterations, an iterate on its way, compared bit for bit like every other
ITERATIONS = {"invroot5": 30, "invroot6": 30, "root5": 30, "log": 60}
SIZES = ((512, 8), (1024, 40))   # (n, half bandwidth)
# Chebyshev coefficients of log(1 + x) on [-1, 1], as ComputeLogarithm holds them: 32 that decay to 2e-13
LOG_COEF = [-0.485101351704, 1.58828112379, -0.600947731795, 0.287304748177, -0.145496447103, 0.0734013668818, -0.0356277942958,
            0.0161605505166, -0.0066133591188, 0.00229833505456, -0.000577804103964, 2.2849332964e-05, 8.37426826403e-05,
            -6.10822859027e-05, 2.58132364523e-05, -5.87577322647e-06, -8.56711062722e-07, 1.52066488969e-06, -7.12760496253e-07,
            1.23102245249e-07, 6.03168259043e-08, -5.1865499826e-08, 1.43185107512e-08, 2.58449717089e-09, -3.73189861771e-09,
            1.18469334815e-09, 1.51569931066e-10, -2.89595999673e-10, 1.26720668874e-10, -3.00079067694e-11, 3.91175568865e-12,
            -2.21155654398e-13]
# solver: (shift of the band, argument).  trig: a Gershgorin radius in (2, 4) for Cosine and for Sine's operand A - pi/2 I: two
# doublings.  roots, log: a Gershgorin lower bound above 0.5; log: a spectral radius in (4, 16): ComputeRoot(8) behind it, so the
# inverse-root iteration runs there too.  The polynomials: the band nearly unshifted (radius below 2.5), coefficients that decay; the
# factorized Chebyshev evaluation merges the operand itself (T1), and with a shift that is a multiple of 0.002 one diagonal entry in
# a thousand is an exact zero -- a stored zero makes the operand a read-only view, which the pass refuses: 0.001 stores none
SOLVERS = {"cos": (1.0, None), "sin": (1.0, None), "ps7": (0.0, 7), "ps16": (0.0, 16), "chebyfact5": (0.001, 5), "chebyfact32": (0.001, 32),
           "log": (3.5, None), "invroot5": (3.5, 5), "invroot6": (3.5, 6), "root5": (6.0, 5)}


def solve_triplets(kind, n, h, c0=0, c1=None):
    return banded_triplets(n, h, shift=SOLVERS[kind][0], c0=c0, c1=c1)


def dense(t, n):
    M = np.zeros((n, n), dtype=np.asarray(t[2]).dtype)
    M[t[1] - 1, t[0] - 1] = t[2]
    return M


def gershgorin(A):
    r = np.abs(A).sum(axis=0) - np.abs(np.diag(A))
    return float((np.diag(A) - r).min()), float((np.diag(A) + r).max())


def doublings(radius):
    sigma, counter = 1.0, 1
    while radius / sigma > 1.0:
        sigma *= 2
        counter += 1
    return counter - 1


def chebyfact_passes(n):
    """cheby_recursive on n coefficients: a two-coefficient leaf is one chain, every combine is one"""
    if n <= 1:
        return 0
    if n == 2:
        return 1
    return chebyfact_passes(n // 2) + chebyfact_passes(n - n // 2) + 1


def paterson_stockmeyer_passes(degree):
    """one chain per Bk that has 1 .. 5 addends (all coefficients of the test are non-zero)"""
    m = degree - 1
    s = int(np.sqrt(np.float32(m)))
    r = m // s
    groups = [m - s * r] + [s - 1] * r
    return sum(1 for g in groups if 1 <= g <= 5)


def inverse_root_target(root):
    return root // 4 if root % 4 == 0 else root if root % 2 == 1 else (root - 2) // 2 + 1


def expected_passes(kind, n, h):
    """the number of chains the loop structure gives, from the operand in numpy"""
    shift, arg = SOLVERS[kind]
    A = dense(solve_triplets(kind, n, h), n)
    assert np.array_equal(A, A.T)
    if kind in ("cos", "sin"):
        if kind == "sin":
            A = A - np.eye(n) * (math.pi / 2.0)
        lo, hi = gershgorin(A)
        radius = max(abs(lo), abs(hi))
        assert 2.0 * 1.05 < radius < 4.0 / 1.05, radius
        assert doublings(radius) >= 2
        return 2 + doublings(radius)
    if kind.startswith("ps"):
        return paterson_stockmeyer_passes(arg)
    if kind.startswith("chebyfact"):
        assert np.count_nonzero(solve_triplets(kind, n, h)[2] == 0.0) == 0, "the operand stores no zero"
        return chebyfact_passes(arg)
    assert gershgorin(A)[0] > 0.5, gershgorin(A)
    if kind == "log":
        # PowerBounds' estimate chooses the root; at least 5 % from the boundaries sqrt(2)^(2^k) its last digits do not matter
        radius = float(np.abs(np.linalg.eigvalsh(A)).max())
        assert 4.0 * 1.05 < radius < 16.0 / 1.05, radius
        sigma = 1
        while radius > math.sqrt(2.0):
            radius, sigma = math.sqrt(radius), 2 * sigma
        assert sigma == 8 and inverse_root_target(8) == 2
        return chebyfact_passes(32) + ITERATIONS[kind]   # (the unit polynomial of ComputeRoot has zero coefficients: its groups take the calls)
    assert inverse_root_target(arg) >= 2
    return ITERATIONS[kind]   # (root5: the unit polynomial before the iteration makes no chain)


def coefficients(k):
    return [LOG_COEF[q] if k == 32 else (-1.0) ** q * 0.8 ** q / (q + 1.0) for q in range(k)]


def run_solver(nt, kind, A, n, perm=None):
    """the loops whose length a convergence test decides run ITERATIONS[kind] iterations (a converge_diff no norm reaches, no
    monitor): the count of chains is then the loop structure's"""
    p = nt.SolverParameters()
    p.SetThreshold(THRESHOLDS.get(kind, THR))
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(ITERATIONS.get(kind, 8))
    p.SetMonitorConvergence(False)
    if perm is not None:
        p.SetLoadBalance(perm)
    Out = nt.Matrix_ps(n)
    arg = SOLVERS[kind][1]
    c0, s0 = nt.sum_chain_counts(), nt.slab_algebra_counts()
    if kind == "cos":
        nt.TrigonometrySolvers.Cosine(A, Out, p)
    elif kind == "sin":
        nt.TrigonometrySolvers.Sine(A, Out, p)
    elif kind.startswith("ps") or kind.startswith("chebyfact"):
        poly = (nt.Polynomial if kind.startswith("ps") else nt.ChebyshevPolynomial)(arg)
        for k, v in enumerate(coefficients(arg)):
            poly.SetCoefficient(k, v)
        getattr(poly, "PatersonStockmeyerCompute" if kind.startswith("ps") else "ComputeFactorized")(A, Out, p)
    elif kind == "log":
        nt.ExponentialSolvers.ComputeLogarithm(A, Out, p)
    elif kind.startswith("invroot"):
        nt.RootSolvers.ComputeInverseRoot(A, Out, arg, p)
    else:
        nt.RootSolvers.ComputeRoot(A, Out, arg, p)
    c1, s1 = nt.sum_chain_counts(), nt.slab_algebra_counts()
    return dict(out=srt(Out.triplets()), counts=delta(c0, c1), slab=delta(s0, s1))


def both_options(nt, kind, A, n, perm=None, tag=""):
    runs = {}
    for v in (1, 0):
        nt.set_option("sum_chain", v)
        runs[v] = run_solver(nt, kind, A, n, perm=perm)
        print(tag, kind, "option", v, "counts", runs[v]["counts"], "slab algebra", runs[v]["slab"], "entries", len(runs[v]["out"][2]))
    nt.set_option("sum_chain", 1)
    assert np.isfinite(runs[0]["out"][2]).all() and len(runs[0]["out"][2]) > n
    first = ("pattern" if not (np.array_equal(runs[1]["out"][0], runs[0]["out"][0]) and np.array_equal(runs[1]["out"][1], runs[0]["out"][1]))
             else "values")
    assert same(runs[1]["out"], runs[0]["out"]), "option 1 against 0: %s differ" % first
    return runs


@pytest.mark.parametrize("kind", sorted(SOLVERS))
@pytest.mark.parametrize("n,h", SIZES, ids=["n%d_h%d" % s for s in SIZES])
def test_solvers_1_against_0(nt, fma, n, h, kind):
    """the result equal in pattern and bits with the option at 1 and at 0; with 1 as many passes as the loop structure gives and
    none refused, with 0 none at all"""
    want = expected_passes(kind, n, h)
    A = nt.Matrix_ps.from_triplets(n, *solve_triplets(kind, n, h))
    runs = both_options(nt, kind, A, n, tag="n%d h%d" % (n, h))
    assert runs[0]["counts"] == dict(passes=0, refused=0), runs[0]["counts"]
    assert runs[1]["counts"] == dict(passes=want, refused=0), (runs[1]["counts"], want)


def balance_lookup(n):
    """a fixed permutation for the load balancer, the same in every process: 1-based, seeded"""
    return (np.random.default_rng(20261021).permutation(n) + 1).astype(np.int32)


@pytest.mark.parametrize("kind", ("cos", "chebyfact32"))
@pytest.mark.parametrize("perm_kind", ("reverse", "seeded"))
def test_solvers_with_a_load_balancer_permutation(nt, fma, perm_kind, kind):
    """`reverse` keeps the band: the passes of the plain run.  `seeded` scatters it: whatever passes are taken or refused (printed),
    1 and 0 bit for bit either way"""
    n, h = SIZES[0]
    A = nt.Matrix_ps.from_triplets(n, *solve_triplets(kind, n, h))
    perm = nt.Permutation(n)
    if perm_kind == "reverse":
        perm.SetReversePermutation()
    else:
        perm.set_lookup(balance_lookup(n))
    runs = both_options(nt, kind, A, n, perm=perm, tag=perm_kind)
    assert runs[0]["counts"] == dict(passes=0, refused=0)
    if perm_kind == "reverse":
        assert runs[1]["counts"] == dict(passes=expected_passes(kind, n, h), refused=0), runs[1]["counts"]


# ------------------------------------------------------------------ golden
@pytest.fixture
def option_on(nt):
    before = nt.get_option("sum_chain")
    nt.set_option("sum_chain", 1)
    yield
    nt.set_option("sum_chain", before)


def test_golden_cases_with_the_option(nt, option_on):
    """the real cases of tests/golden/functions.npz (log, sin, cos, root, inverse root) and polynomials.npz (ps, chebyfact) that
    tests/test_gpu_extras.py runs for these solvers, with the option at 1, in the bounds that test gives them:
    max(1000 thr, 1e-11) max(1, max|K|) and max(100 thr, 1e-12) max(1, max|K|)"""
    fused = 0

    def check(i, c, want, Out, factor, floor, d):
        gd, wd = to_dense((want[0], want[1]) + tuple(Out.triplets())), to_dense(want)
        if not np.isfinite(wd).all() or np.abs(wd).max() > 1e100:
            return   # (the reference's own Newton iteration diverges for this root on this matrix: no meaningful comparison)
        diff, bound = float(np.abs(gd - wd).max()), max(factor * c["thr"], floor) * max(1.0, float(np.abs(wd).max()))
        print(i, c["kind"], c.get("matrix"), c.get("root"), "thr", c["thr"], "counts", d, "max |K - K_ref|", diff, "bound", bound)
        assert diff <= bound, (i, c["kind"], diff, bound)

    g = Golden("functions")
    mats = {}
    for i, c in enumerate(g.cases):
        if c["kind"] in ("exp", "power") or c["matrix"] == "csym":   # (every other kind: log, sin, cos, root, and the inverse roots)
            continue
        if c["matrix"] not in mats:
            t = g.tri(None, "M_" + c["matrix"])
            mats[c["matrix"]] = (nt.Matrix_ps.from_triplets(t[0], t[2], t[3], t[4]), t[0])
        A, n = mats[c["matrix"]]
        p = nt.SolverParameters()
        p.SetThreshold(c["thr"])
        p.SetConvergeDiff(c["conv"])
        Out = nt.Matrix_ps(n)
        c0 = nt.sum_chain_counts()
        if c["kind"] == "log":
            nt.ExponentialSolvers.ComputeLogarithm(A, Out, p)
        elif c["kind"] == "sin":
            nt.TrigonometrySolvers.Sine(A, Out, p)
        elif c["kind"] == "cos":
            nt.TrigonometrySolvers.Cosine(A, Out, p)
        elif c["kind"] == "root":
            nt.RootSolvers.ComputeRoot(A, Out, c["root"], p)
        else:
            nt.RootSolvers.ComputeInverseRoot(A, Out, c["root"], p)
        d = delta(c0, nt.sum_chain_counts())
        fused += d["passes"]
        check(i, c, g.tri(i, "K"), Out, 1000, 1e-11, d)
    assert fused > 0
    g, fused_poly = Golden("polynomials"), 0
    t = g.tri(None, "A0")
    A, n = nt.Matrix_ps.from_triplets(t[0], t[2], t[3], t[4]), t[0]
    for i, c in enumerate(g.cases):
        if c["kind"] not in ("ps", "chebyfact") or c["complex"]:
            continue
        p = nt.SolverParameters()
        p.SetThreshold(c["thr"])
        poly = (nt.Polynomial if c["kind"] == "ps" else nt.ChebyshevPolynomial)(len(c["coef"]))
        for k, x in enumerate(c["coef"]):
            poly.SetCoefficient(k, x)
        Out = nt.Matrix_ps(n)
        c0 = nt.sum_chain_counts()
        getattr(poly, "PatersonStockmeyerCompute" if c["kind"] == "ps" else "ComputeFactorized")(A, Out, p)
        d = delta(c0, nt.sum_chain_counts())
        fused_poly += d["passes"]
        check(i, dict(c, matrix="A0", root=None), g.tri(i, "K"), Out, 100, 1e-12, d)
    assert fused_poly > 0


# ------------------------------------------------------------------ two ranks
WORKER_KINDS = ("cos", "chebyfact32")


def run_world(world, tmp_path):
    out = str(tmp_path / ("sum%d" % world))
    name = "s%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name, NTPOLY_AMD_SHM_MB="64",
                   NTPOLY_AMD_SPGEMM_FMA="1")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "sum_chain_worker.py"), out],
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
    """the operands as column panels on two ranks sharing one GPU (shared-memory transport, FMA arithmetic), Cosine and the
    factorized Chebyshev evaluation with options 1 and 0 in the same processes: 1 against 0 bit for bit on every rank, the passes
    of the one-rank test on every rank (each panel makes its own pass) and none with 0.  Both ranks hold equal results: each
    rank's worker gathers the whole result of option 1, and the two copies are compared here, pattern and bits"""
    n, h = SIZES[0]
    two = run_world(2, tmp_path)
    for kind in WORKER_KINDS:
        want = expected_passes(kind, n, h)
        for r, p in enumerate(two):
            print("rank", r, kind, "counts (passes, refused)", [p["%s_counts_%d" % (kind, v)].tolist() for v in (1, 0)])
            assert p["%s_counts_1" % kind].tolist() == [want, 0], (r, kind)
            assert p["%s_counts_0" % kind].tolist() == [0, 0], (r, kind)
            assert same(srt(tuple(p["%s_%s_1" % (kind, k)] for k in ("col", "row", "val"))),
                        srt(tuple(p["%s_%s_0" % (kind, k)] for k in ("col", "row", "val")))), (r, kind)
        whole = [srt(tuple(p["%s_all_%s" % (kind, k)] for k in ("col", "row", "val"))) for p in two]
        assert len(whole[0][2]) > n and same(whole[0], whole[1]), kind
        panels = srt(tuple(np.concatenate([p["%s_%s_1" % (kind, k)] for p in two]) for k in ("col", "row", "val")))
        assert same(panels, whole[0]), kind
