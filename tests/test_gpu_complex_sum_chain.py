"""GPU: the complex side of the scaled sum chain (option complex_sum_chain; csrc/sum_chain.hip k_sum_chain<double2, M>, engine.hpp
ps_sum_chain on complex operands).  Level 1: the inverse-root iteration (ComputeInverseRoot, ComputeRoot, ComputeLogarithm) runs in
a complex slab session.  Level 2: and inside any session that takes complex operands a sequence
    CopyMatrix(Base, Out); ScaleMatrix(Out, s); IncrementMatrix(A_k, Out, c_k, 0) for k = 1..M; [ScaleMatrix(Out, post)]
on operands that are all complex is one pass over their runs of (re, im) pairs.

The kernel is reached with crafted operands through nt.sum_chain and compared with (i) the same vocabulary calls on compressed
columns (slab_algebra = 0) and (ii) a numpy restatement of AddSparseVectors.f90 at threshold 0 on complex vectors written here,
applied M times in a chain -- never with the fused code itself.  Every scalar is real and scales each part by itself (never numpy's
complex product of a promoted scalar), a sum is taken part by part, an entry is held iff it is not (0, 0).  numpy's float64
products and sums are the correctly rounded ones the kernel spells as __dmul_rn / __dadd_rn, so patterns are compared for equality
and both parts with np.array_equal.  The solvers are held to bit equality between levels 2 and 1 (the pass and the calls it
replaces are local and enter no reduction); level 1 against 0 changes the products' kernel (the complex tile kernel's tolerance
mode) and is held to the rule of tests/test_gpu_complex_poly_sessions.py against a dense evaluation."""
import math
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from gen import banded_triplets
from golden_util import Golden, to_dense
from test_gpu_sum_chain import (ABOVE, BACK, BELOW, CASES, EMPTY_ALL, FULL, IDENT, IDS, ITERATIONS, LAST, LOG_COEF, N, ONLY, POST, SCALARS,
                                SIZES, SOLVERS, THR, THRESHOLDS, _has, _set, _unset, chebyfact_passes, coefficients, crafted, delta, dense,
                                doublings, inverse_root_target, paterson_stockmeyer_passes, srt)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION = "complex_sum_chain"
OPTIONS = ("spgemm_fma", "slab_algebra", OPTION, "sum_chain", "virtual_grid")
RE_ONLY, IM_ONLY = 33, 34   # the diagonal row of these columns: Base and the last addend alone hold it and exactly ONE part cancels
B = 0.5 - 0.25j             # the planted Base value
OTHER = 0.6875              # the part of the last addend that does not cancel (0.75 would cancel the real part at M = 5)


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture
def level2(nt):
    """FMA arithmetic (what a complex session needs) and the option at 2"""
    before = {k: nt.get_option(k) for k in OPTIONS}
    nt.set_option("spgemm_fma", 1)
    nt.set_option(OPTION, 2)
    yield
    for k, v in before.items():
        nt.set_option(k, v)


def same(a, b):
    """sorted triplets: equal patterns, equal real parts, equal imaginary parts (a NaN the refusal test plants equals itself)"""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(np.real(a[2]), np.real(b[2]), equal_nan=True) and
            np.array_equal(np.imag(a[2]), np.imag(b[2]), equal_nan=True))


def scaled(alpha, v):
    """ScaleMatrix by a real scalar on complex values: each part by itself"""
    v = np.asarray(v, dtype=np.complex128)
    return alpha * v.real + 1j * (alpha * v.imag)


def part_by_part(z, factor):
    return complex(factor * z.real, factor * z.imag)


# ------------------------------------------------------------------ operands
def crafted_complex(M, ident):
    """patterns and real parts of crafted(M, ident); imaginary parts log-uniform in [1e-6, 1] with a random sign from a second
    generator; the planted rows complex (all dyadic: every cancellation is exact)"""
    s, c = SCALARS[M]
    rng = np.random.default_rng(20261022)
    ops = []
    for o in crafted(M, ident):
        ops.append({j: (rows, vals + 1j * (10.0 ** rng.uniform(-6.0, 0.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows))))
                    for j, (rows, vals) in sorted(o.items())})
    if M >= 2:   # (a) cancels at A_1 in both parts, brought back by A_2
        _set(ops[0], BACK, BACK, B)
        _set(ops[1], BACK, BACK, part_by_part(B, -s / c[0]))
        _set(ops[2], BACK, BACK, 0.375 - 0.125j)
    cancel = part_by_part(B, -s / c[M - 1])
    _set(ops[0], LAST, LAST, B)          # (b) cancels at the last addend in both parts
    _set(ops[M], LAST, LAST, cancel)
    _set(ops[M], ONLY, ONLY, 0.625 + 0.375j)   # (c) only the last addend holds the row
    for j, v in ((RE_ONLY, complex(cancel.real, OTHER)), (IM_ONLY, complex(OTHER, cancel.imag))):
        _set(ops[0], j, j, B)
        for q in range(1, M):
            _unset(ops[q], j, j)
        _set(ops[M], j, j, v)
    return ops


def _triplets(cols):
    c, r, v = [], [], []
    for j in sorted(cols):
        rows, vals = cols[j]
        c.append(np.full(len(rows), j + 1))
        r.append(rows + 1)
        v.append(np.asarray(vals, dtype=np.complex128))
    return np.concatenate(c).astype(np.int32), np.concatenate(r).astype(np.int32), np.concatenate(v)


def _matrix(nt, cols, n=N):
    c, r, v = _triplets(cols)
    M = nt.Matrix_ps.from_triplets(n, c, r, v)
    assert len(M.triplets()[2]) == len(v)
    return M


# ------------------------------------------------------------------ AddSparseVectors.f90 at threshold 0 on complex vectors, restated
def add_sparse(a, alpha, b, stats):
    """alpha a + b on sorted sparse complex vectors (rows, values): the scaled value rounded part by part, then added part by
    part; inside the overlap of the two lists an entry is kept iff it is not (0, 0), beyond the end of one list the tail of the
    other is copied unfiltered"""
    (ra, va), (rb, vb) = a, b
    if len(ra) == 0 and len(rb) == 0:
        return ra, va
    rows = np.union1d(ra, rb)
    ia, ib = np.isin(rows, ra), np.isin(rows, rb)
    wa, wb = np.zeros(len(rows), dtype=np.complex128), np.zeros(len(rows), dtype=np.complex128)
    wa[ia] = scaled(alpha, va)
    wb[ib] = vb
    both = wa.real + wb.real + 1j * (wa.imag + wb.imag)
    s = np.where(ia & ib, both, np.where(ia, wa, wb))
    lim = min(ra[-1] if len(ra) else -1, rb[-1] if len(rb) else -1)
    nz = (s.real != 0.0) | (s.imag != 0.0)
    keep = (rows > lim) | nz
    for key, count in (("both_kept", ia & ib & nz), ("cancelled", ia & ib & ~nz), ("only_a", ia & ~ib), ("only_b", ~ia & ib),
                       ("one_part", ia & ib & ((s.real == 0.0) != (s.imag == 0.0)))):
        stats[key] = stats.get(key, 0) + int(count.sum())
    stats["underflow"] = stats.get("underflow", 0) + int((~nz & ~(ia & ib)).sum()) + int((ia & (wa == 0.0)).sum())
    return rows[keep], s[keep]


def restated(ops, s, c, post, n=N, trace=None):
    """the chain as {column: (rows, values)} and the branch statistics of the copy-and-scale, each merge and the trailing scaling;
    trace = (column, row): the value of that row behind every step (None where it is absent)"""
    empty = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.complex128))
    out, st, seen = {}, [{} for _ in range(len(c) + 2)], []
    for j in range(n):
        def look(v):
            if trace and j == trace[0]:
                seen.append(complex(v[1][v[0] == trace[1]][0]) if trace[1] in v[0] else None)
        rows, vals = ops[0].get(j, empty)
        v = (rows, scaled(s, vals))   # CopyMatrix; ScaleMatrix
        st[0]["underflow"] = st[0].get("underflow", 0) + int((v[1] == 0.0).sum())
        look(v)
        for k, ck in enumerate(c):
            v = add_sparse(ops[k + 1].get(j, empty), ck, v, st[k + 1])   # IncrementMatrix(A_k, Out, c_k, 0)
            look(v)
        if post != 1.0:
            v = (v[0], scaled(post, v[1]))
            st[-1]["underflow"] = st[-1].get("underflow", 0) + int((v[1] == 0.0).sum())
        if len(v[0]):
            out[j] = v
    return out, st, seen


def _at(cols, j, r):
    return complex(cols[j][1][cols[j][0] == r][0])


@pytest.mark.parametrize("M,post,inplace", CASES, ids=IDS)
def test_the_inputs_reach_every_branch(M, post, inplace):
    """from the operands and the numpy restatement alone (no GPU is touched): the patterns are the real test's (empty columns, runs
    wholly below and above, a full column, holes, a diagonal operand), every merge has one-sided entries from either side, the rows
    that cancel in BOTH parts are exactly the planted ones per merge, exactly two rows cancel in ONE part, at the last merge, and
    are kept; no scaled value is (0, 0) where an entry is held"""
    ident = IDENT[M, inplace]
    s, c = SCALARS[M]
    ops, real = crafted_complex(M, ident), crafted(M, ident)
    moved = {(BACK, BACK), (LAST, LAST), (ONLY, ONLY), (RE_ONLY, RE_ONLY), (IM_ONLY, IM_ONLY)}
    for q in range(M + 1):
        for j in range(N):
            if j in (RE_ONLY, IM_ONLY):
                continue
            assert (j in ops[q]) == (j in real[q])
            if j in ops[q]:
                assert np.array_equal(ops[q][j][0], real[q][j][0]), "patterns of the real test"
                free = np.array([(j, int(r)) not in moved for r in ops[q][j][0]])
                assert np.array_equal(ops[q][j][1].real[free], real[q][j][1][free])
                assert (np.abs(ops[q][j][1].imag[free]) >= 1e-6).all() and (np.abs(ops[q][j][1].imag[free]) <= 1.0).all()
        assert EMPTY_ALL not in ops[q] and 7 + q not in ops[q]
    if ident != "base":
        assert ops[1][BELOW][0][0] > ops[0][BELOW][0][-1] and ops[1][ABOVE][0][-1] < ops[0][ABOVE][0][0]
        assert ops[0][FULL][0][0] == 0 and ops[0][FULL][0][-1] == N - 1
    out, st, _ = restated(ops, s, c, post)
    print(M, post, ident, st)
    assert all(x.get("underflow", 0) == 0 for x in st)
    for k in range(1, M + 1):
        assert st[k]["only_a"] > 0 and st[k]["only_b"] > 0, (k, st[k])
        assert st[k]["both_kept"] > 200, (k, st[k])
    want_cancelled = [0] * (M + 1)
    want_cancelled[M] += 1
    if M >= 2:
        want_cancelled[1] += 1
        seen = restated(ops, s, c, post, trace=(BACK, BACK))[2]
        assert seen[0] == scaled(s, B) and seen[1] is None and seen[2] == scaled(c[1], 0.375 - 0.125j), seen
        assert _has(out, BACK, BACK)
    assert [st[k]["cancelled"] for k in range(1, M + 1)] == want_cancelled[1:], st
    assert [st[k]["one_part"] for k in range(1, M + 1)] == [0] * (M - 1) + [2], st
    seen = restated(ops, s, c, post, trace=(LAST, LAST))[2]
    assert all(x == scaled(s, B) for x in seen[:M]) and seen[M] is None, seen
    assert not _has(out, LAST, LAST)
    seen = restated(ops, s, c, post, trace=(ONLY, ONLY))[2]
    assert all(x is None for x in seen[:M]) and seen[M] == scaled(c[M - 1], 0.625 + 0.375j), seen
    # the rows of which one part cancels are KEPT, with that part zero and the other not
    cm = c[M - 1]
    v = _at(out, RE_ONLY, RE_ONLY)
    assert v.real == 0.0 and v.imag == post * (s * B.imag + cm * OTHER) != 0.0, v
    v = _at(out, IM_ONLY, IM_ONLY)
    assert v.imag == 0.0 and v.real == post * (s * B.real + cm * OTHER) != 0.0, v


@pytest.mark.parametrize("M,post,inplace", CASES, ids=IDS)
def test_pass_bit_for_bit(nt, level2, M, post, inplace):
    s, c = SCALARS[M]
    ops = crafted_complex(M, IDENT[M, inplace])
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
    assert np.array_equal(V[0], want[0]) and np.array_equal(V[1], want[1]), "pattern: compressed columns against the restatement"
    assert same(V, want), "compressed columns against the restatement"
    Out = Ms[0] if inplace else nt.Matrix_ps(N)
    c0, r0, s0 = nt.complex_sum_chain_counts(), nt.sum_chain_counts(), nt.slab_algebra_counts()
    with nt.solver_session(True):
        got = nt.sum_chain(Ms[0], s, Ms[1:], c, post, Out)
        c1, s1 = nt.complex_sum_chain_counts(), nt.slab_algebra_counts()
    print("counts", c0, c1, "slab algebra", s0, s1, "entries", len(want[2]))
    assert got is True
    assert delta(c0, c1) == dict(sessions=0, passes=1, refused=0)
    assert nt.sum_chain_counts() == r0 and s1["refusals"] == s0["refusals"]
    for m, bf in list(zip(Ms, before))[1 if inplace else 0:]:
        assert same(srt(m.triplets()), bf), "the operands are as they were"
    g = srt(Out.triplets())
    assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]), "pattern"
    assert same(g, want), "values against the restatement"
    assert same(g, V), "values against compressed columns"
    rows = {(int(cc) - 1, int(rr) - 1) for cc, rr in zip(g[0], g[1])}
    assert (RE_ONLY, RE_ONLY) in rows and (IM_ONLY, IM_ONLY) in rows and (LAST, LAST) not in rows


# ------------------------------------------------------------------ refusals
def test_refusals_and_gates_leave_everything_as_it_was(nt, level2):
    n, j = 4099, 5

    def col(f, l, v=None):
        if v is None:
            v = np.linspace(0.1, 0.9, l - f + 1) + 1j * np.linspace(-0.7, 0.8, l - f + 1)
        return {j: (np.arange(f, l + 1), np.asarray(v, dtype=np.complex128))}

    def attempt(Base, As, counted, s=2.0, c=None, post=1.0, out=None, complex_ok=True, taken=False):
        Out = out if out is not None else nt.Matrix_ps(n)
        c = [0.25, -1.0, 0.625, 4.0, -0.5, 1.5][:len(As)] if c is None else c
        ms = [Base] + list(As) + ([Out] if out is not None else [])
        before = [srt(m.triplets()) for m in ms]
        c0, r0, s0 = nt.complex_sum_chain_counts(), nt.sum_chain_counts(), nt.slab_algebra_counts()
        with nt.solver_session(complex_ok):
            got = nt.sum_chain(Base, s, As, c, post, Out)
        c1, s1 = nt.complex_sum_chain_counts(), nt.slab_algebra_counts()
        assert nt.sum_chain_counts() == r0
        if taken:
            assert got is True and delta(c0, c1) == dict(sessions=0, passes=1, refused=0), (c0, c1)
            return Out
        assert got is False
        assert c1 == dict(c0, refused=c0["refused"] + counted), (c0, c1)
        assert s1 == s0, (s0, s1)   # (a refused pass is no operation and no refusal of the session)
        for m, bf in zip(ms, before):
            assert same(srt(m.triplets()), bf)
        if out is None:
            assert len(Out.triplets()[2]) == 0
        return None

    mk = lambda cc: _matrix(nt, cc, n=n)
    half = 0.5 + 0.25j
    MB, M1, M2 = mk(col(0, 9)), mk(col(4, 20)), mk(col(2, 12))
    far = mk(col(n // 2 + 1, n // 2 + 11))
    # runs n / 2 rows apart in one column, in each role
    attempt(far, [M1, M2], 1)
    attempt(MB, [far], 1)
    attempt(MB, [M1, far], 1)
    # a product of which BOTH parts underflow to zero where an entry is held: c_k a_k where the addend alone holds the row and where
    # both do, s base, and the trailing scaling
    tiny = 1e-200 + 1e-200j
    assert 1e-200 * 1e-200 == 0.0
    attempt(MB, [mk(col(4, 20, [half] * 16 + [tiny]))], 1, c=[1e-200])
    attempt(MB, [M2, mk(col(4, 20, [tiny] + [half] * 16))], 1, c=[0.25, 1e-200])
    attempt(mk(col(0, 9, [tiny] + [half] * 9)), [M1], 1, s=1e-200)
    attempt(mk(col(0, 9, [tiny] + [half] * 9)), [M1], 1, s=1.0, post=1e-200)
    # an entry that is not finite, in the real part or in the imaginary part, in each role
    attempt(mk(col(0, 9, [half] * 9 + [complex(np.nan, 0.5)])), [M1], 1)
    attempt(MB, [mk(col(4, 20, [half] * 8 + [complex(0.5, np.nan)] + [half] * 8))], 1)
    attempt(MB, [M1, mk(col(2, 12, [half] * 5 + [complex(np.inf, 0.5)] + [half] * 5))], 1)
    attempt(MB, [M1, mk(col(2, 12, [half] * 5 + [complex(0.5, -np.inf)] + [half] * 5))], 1)
    # an input that stores (0, 0) enters slab form as a read-only view: the pass merges no view
    view = col(0, 9)
    view[j][1][4] = 0.0
    attempt(mk(view), [M1], 1)
    attempt(MB, [mk(view)], 1)
    # ONE part underflows: an ordinary kept entry -- the pass is taken and equals the calls on compressed columns
    one = mk(col(4, 20, [half] * 16 + [1e-200 + 0.5j]))
    Out = attempt(MB, [one], 0, c=[1e-200], taken=True)
    nt.set_option("slab_algebra", 0)
    V = nt.Matrix_ps(MB)
    V.Scale(2.0)
    V.Increment(one, 1e-200, 0.0)
    nt.set_option("slab_algebra", 1)
    g, V = srt(Out.triplets()), srt(V.triplets())
    assert same(g, V) and g[1][-1] == 21 and g[2][-1] == complex(0.0, 0.5 * 1e-200)
    # gated, counted nowhere
    for v in (0, 1):
        nt.set_option(OPTION, v)
        attempt(MB, [M1, M2], 0)
    nt.set_option(OPTION, 2)
    attempt(MB, [M1, M2], 0, complex_ok=False)
    MR = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, 3))
    attempt(MR, [M1], 0)
    attempt(MB, [M1, MR], 0)
    six = [mk(col(k, 12 + k)) for k in range(6)]
    attempt(MB, six, 0)
    attempt(MB, [M1, M2], 0, out=M2)
    attempt(MB, [M1, M1], 0)
    attempt(MB, [MB], 0)
    attempt(MB, [M1, MB], 0, out=MB)
    attempt(MB, [M1, M2], 0, c=[0.25, 0.0])
    attempt(MB, [M1, M2], 0, s=0.0)
    attempt(MB, [M1, M2], 0, post=0.0)
    attempt(MB, [M1, M2], 0, post=np.inf)
    attempt(MB, [M1, M2], 0, s=np.inf)
    nt.set_option("spgemm_fma", 0)
    attempt(MB, [M1, M2], 0)
    nt.set_option("spgemm_fma", 1)
    # ... and the same operands ARE taken with everything in place, five addends of them
    attempt(MB, six[:5], 0, taken=True)


# ------------------------------------------------------------------ the solvers
KINDS = ("cos", "sin", "ps7", "ps16", "chebyfact5", "chebyfact32", "log", "invroot5", "invroot6", "root5")
ROOT_LOOPS = {"log": 1, "invroot5": 1, "invroot6": 1, "root5": 1}   # inverse-root loops per call


def solve_triplets(kind, n, h, c0=0, c1=None):
    return banded_triplets(n, h, complex_=True, shift=SOLVERS[kind][0], c0=c0, c1=c1)


def gershgorin(A):
    """the bounds of a Hermitian matrix: real diagonal, radii from the moduli"""
    d = np.diag(A).real
    r = np.abs(A).sum(axis=0) - np.abs(np.diag(A))
    return float((d - r).min()), float((d + r).max())


_OPERANDS = {}


def operand(kind, n, h):
    """the dense operand, computed once per (shift, n, h) and left unchanged"""
    key = (SOLVERS[kind][0], n, h)
    if key not in _OPERANDS:
        A = dense(solve_triplets(kind, n, h), n)
        assert np.array_equal(A, A.conj().T) and np.iscomplexobj(A)
        A.setflags(write=False)
        _OPERANDS[key] = A
    return _OPERANDS[key]


def expected_passes(kind, n, h):
    """the number of chains the loop structure gives, from the complex operand in numpy"""
    shift, arg = SOLVERS[kind]
    A = operand(kind, n, h)
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
        assert np.count_nonzero(solve_triplets(kind, n, h)[2] == 0.0) == 0, "the operand stores no (0, 0)"
        return chebyfact_passes(arg)
    assert gershgorin(A)[0] > 0.5, gershgorin(A)
    if kind == "log":
        radius = float(np.abs(np.linalg.eigvalsh(A)).max())
        assert 4.0 * 1.05 < radius < 16.0 / 1.05, radius
        sigma = 1
        while radius > math.sqrt(2.0):
            radius, sigma = math.sqrt(radius), 2 * sigma
        assert sigma == 8 and inverse_root_target(8) == 2
        return chebyfact_passes(32) + ITERATIONS[kind]
    assert inverse_root_target(arg) >= 2
    return ITERATIONS[kind]


def run_solver(nt, kind, A, n, perm=None, threshold=None):
    """the loops whose length a convergence test decides run ITERATIONS[kind] iterations (a converge_diff no norm reaches, no
    monitor): the count of chains is then the loop structure's"""
    p = nt.SolverParameters()
    p.SetThreshold(THRESHOLDS.get(kind, THR) if threshold is None else threshold)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(ITERATIONS.get(kind, 8))
    p.SetMonitorConvergence(False)
    if perm is not None:
        p.SetLoadBalance(perm)
    Out = nt.Matrix_ps(n)
    arg = SOLVERS[kind][1]
    c0, r0, s0 = nt.complex_sum_chain_counts(), nt.sum_chain_counts(), nt.slab_algebra_counts()
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
    assert nt.sum_chain_counts() == r0, "the real loops' counter never moves"
    return dict(out=srt(Out.triplets()), counts=delta(c0, nt.complex_sum_chain_counts()), slab=delta(s0, nt.slab_algebra_counts()))


def levels(nt, kind, A, n, which, perm=None, tag="", threshold=None):
    runs = {}
    for v in which:
        nt.set_option(OPTION, v)
        runs[v] = run_solver(nt, kind, A, n, perm=perm, threshold=threshold)
        print(tag, kind, "level", v, "counts", runs[v]["counts"], "slab algebra", runs[v]["slab"], "entries", len(runs[v]["out"][2]))
    nt.set_option(OPTION, 2)
    return runs


def check_2_against_1(runs, kind, n, want):
    assert np.isfinite(runs[1]["out"][2]).all() and len(runs[1]["out"][2]) > n
    first = ("pattern" if not (np.array_equal(runs[2]["out"][0], runs[1]["out"][0]) and np.array_equal(runs[2]["out"][1], runs[1]["out"][1]))
             else "values")
    assert same(runs[2]["out"], runs[1]["out"]), "level 2 against 1: %s differ" % first
    loops = ROOT_LOOPS.get(kind, 0)
    assert runs[2]["counts"] == dict(sessions=loops, passes=want, refused=0), (runs[2]["counts"], want)
    assert runs[1]["counts"] == dict(sessions=loops, passes=0, refused=0), runs[1]["counts"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,h", SIZES, ids=["n%d_h%d" % s for s in SIZES])
def test_solvers_2_against_1(nt, level2, n, h, kind):
    """the result equal in pattern and in both parts with the option at 2 and at 1; with 2 as many passes as the loop structure
    gives and none refused, with 1 none at all; one session per inverse-root loop with either"""
    want = expected_passes(kind, n, h)
    A = nt.Matrix_ps.from_triplets(n, *solve_triplets(kind, n, h))
    check_2_against_1(levels(nt, kind, A, n, (2, 1), tag="n%d h%d" % (n, h)), kind, n, want)


def test_solver_with_a_reverse_permutation(nt, level2):
    """SetReversePermutation keeps the band: the counts of the plain run, 2 against 1 bit for bit"""
    kind, (n, h) = "invroot5", SIZES[0]
    A = nt.Matrix_ps.from_triplets(n, *solve_triplets(kind, n, h))
    perm = nt.Permutation(n)
    perm.SetReversePermutation()
    check_2_against_1(levels(nt, kind, A, n, (2, 1), perm=perm, tag="reverse"), kind, n, expected_passes(kind, n, h))


# ------------------------------------------------------------------ level 1 against level 0: the new session
@pytest.fixture(scope="module")
def dense_references():
    """V f(w) V^H from numpy.linalg.eigh of the dense operand, once per (kind, n, h), left unchanged"""
    cache = {}

    def get(kind, n, h):
        if (kind, n, h) not in cache:
            w, V = np.linalg.eigh(np.array(operand(kind, n, h)))
            assert w.min() > 0.5
            f = np.log(w) if kind == "log" else w ** (-1.0 / SOLVERS[kind][1])
            F = (V * f) @ V.conj().T
            F.setflags(write=False)
            cache[kind, n, h] = F
        return cache[kind, n, h]
    return get


@pytest.mark.parametrize("kind", ("invroot5", "invroot6", "log"))
@pytest.mark.parametrize("n,h", SIZES, ids=["n%d_h%d" % s for s in SIZES])
def test_level_1_against_0_by_the_dense_evaluation(nt, level2, dense_references, n, h, kind):
    """dev = max|K - F| against the dense evaluation F: the session's deviation is at most 4 x that of the path that exists today
    (level 0: compressed columns between the operations), floored at 1e-12 max|F| -- the rule of
    test_values_against_dense_evaluation in tests/test_gpu_complex_poly_sessions.py"""
    F = dense_references(kind, n, h)
    A = nt.Matrix_ps.from_triplets(n, *solve_triplets(kind, n, h))
    runs = levels(nt, kind, A, n, (0, 1), tag="n%d h%d" % (n, h))
    K = {v: dense(runs[v]["out"], n) for v in (0, 1)}
    dev = {v: float(np.abs(K[v] - F).max()) for v in (0, 1)}
    bound = max(4.0 * dev[0], 1e-12 * float(np.abs(F).max()))
    print("%s n%d h%d: max|F| %.3g, deviation from the dense evaluation: level 0 %.3g, level 1 %.3g, bound %.3g, max|K1 - K0| %.3g" % (
        kind, n, h, np.abs(F).max(), dev[0], dev[1], bound, np.abs(K[1] - K[0]).max()))
    assert runs[0]["counts"] == dict(sessions=0, passes=0, refused=0), runs[0]["counts"]
    assert runs[1]["counts"] == dict(sessions=1, passes=0, refused=0), runs[1]["counts"]
    assert dev[1] <= bound, (kind, dev, bound)


LOG_THRESHOLD = 1e-25   # (what ComputeRoot(5) takes in THRESHOLDS, for the same reason)


@pytest.mark.parametrize("n,h", SIZES, ids=["n%d_h%d" % s for s in SIZES])
def test_level_1_against_0_logarithm_with_a_threshold_below_the_iterate(nt, level2, dense_references, n, h):
    """The logarithm at THR = 1e-9 above constrains little: ComputeRoot(8) behind it iterates on A^7, whose Mk lies below an
    absolute threshold of that size (the note at THRESHOLDS in tests/test_gpu_sum_chain.py describes it for ComputeRoot(5)) -- the
    path of before and the new one both end 0.7 from the dense evaluation.  With the threshold at 1e-25 both end 3e-11 from it, so here the deviation of the path of
    before is itself held: the evaluation's 32 Chebyshev coefficients are given to 12 digits and decay to 2.2e-13, the sum is
    scaled back by sigma = 8 -- 8 x 32 x 1e-12 = 2.6e-10 of coefficients of size 1, bounded here by 1e-9 max|F| -- and the session
    by the rule of the test above"""
    F = dense_references("log", n, h)
    A = nt.Matrix_ps.from_triplets(n, *solve_triplets("log", n, h))
    runs = levels(nt, "log", A, n, (0, 1), tag="n%d h%d thr %g" % (n, h, LOG_THRESHOLD), threshold=LOG_THRESHOLD)
    K = {v: dense(runs[v]["out"], n) for v in (0, 1)}
    dev = {v: float(np.abs(K[v] - F).max()) for v in (0, 1)}
    top = float(np.abs(F).max())
    bound = max(4.0 * dev[0], 1e-12 * top)
    print("log n%d h%d thr %g: max|F| %.3g, deviation from the dense evaluation: level 0 %.3g, level 1 %.3g, bound %.3g, max|K1 - K0| %.3g" % (
        n, h, LOG_THRESHOLD, top, dev[0], dev[1], bound, np.abs(K[1] - K[0]).max()))
    assert runs[0]["counts"] == dict(sessions=0, passes=0, refused=0), runs[0]["counts"]
    assert runs[1]["counts"] == dict(sessions=1, passes=0, refused=0), runs[1]["counts"]
    assert dev[0] <= 1e-9 * top, (dev, top)
    assert dev[1] <= bound, (dev, bound)


# ------------------------------------------------------------------ golden
def test_golden_cases_with_level_2(nt, level2):
    """the complex cases of tests/golden/functions.npz (cos on csym) and polynomials.npz (ps, chebyfact) that
    tests/test_gpu_extras.py runs for these solvers, with the option at 2, in the bounds that test gives them:
    max(1000 thr, 1e-11) max(1, max|K|) and max(100 thr, 1e-12) max(1, max|K|)"""
    fused, ran = 0, []

    def check(i, c, want, Out, factor, floor, d):
        gd, wd = to_dense((want[0], want[1]) + tuple(Out.triplets())), to_dense(want)
        assert np.isfinite(wd).all()
        diff, bound = float(np.abs(gd - wd).max()), max(factor * c["thr"], floor) * max(1.0, float(np.abs(wd).max()))
        print(i, c["kind"], "thr", c["thr"], "counts", d, "max |K - K_ref|", diff, "bound", bound)
        assert diff <= bound, (i, c["kind"], diff, bound)

    g = Golden("functions")
    t = g.tri(None, "M_csym")
    A, n = nt.Matrix_ps.from_triplets(t[0], t[2], t[3], t[4]), t[0]
    for i, c in enumerate(g.cases):
        if c["kind"] != "cos" or c["matrix"] != "csym":
            continue
        p = nt.SolverParameters()
        p.SetThreshold(c["thr"])
        p.SetConvergeDiff(c["conv"])
        Out = nt.Matrix_ps(n)
        c0 = nt.complex_sum_chain_counts()
        nt.TrigonometrySolvers.Cosine(A, Out, p)
        d = delta(c0, nt.complex_sum_chain_counts())
        fused += d["passes"]
        ran.append("cos")
        check(i, c, g.tri(i, "K"), Out, 1000, 1e-11, d)
    g = Golden("polynomials")
    t = g.tri(None, "A1")
    A, n = nt.Matrix_ps.from_triplets(t[0], t[2], t[3], t[4]), t[0]
    for i, c in enumerate(g.cases):
        if c["kind"] not in ("ps", "chebyfact") or not c["complex"]:
            continue
        p = nt.SolverParameters()
        p.SetThreshold(c["thr"])
        poly = (nt.Polynomial if c["kind"] == "ps" else nt.ChebyshevPolynomial)(len(c["coef"]))
        for k, x in enumerate(c["coef"]):
            poly.SetCoefficient(k, x)
        Out = nt.Matrix_ps(n)
        c0 = nt.complex_sum_chain_counts()
        getattr(poly, "PatersonStockmeyerCompute" if c["kind"] == "ps" else "ComputeFactorized")(A, Out, p)
        d = delta(c0, nt.complex_sum_chain_counts())
        fused += d["passes"]
        ran.append(c["kind"])
        check(i, c, g.tri(i, "K"), Out, 100, 1e-12, d)
    assert ran.count("cos") >= 1 and ran.count("ps") == 3 and ran.count("chebyfact") == 5, ran
    assert fused > 0


# ------------------------------------------------------------------ two ranks
WORKER_KINDS = ("cos", "invroot5")


def run_world(world, tmp_path):
    out = str(tmp_path / ("csum%d" % world))
    name = "c%s" % uuid.uuid4().hex[:12]
    drop = ("NTPOLY_AMD_COMPLEX_SUM_CHAIN",)
    procs = []
    for r in range(world):
        env = dict({k: v for k, v in os.environ.items() if k not in drop}, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0",
                   NTPOLY_AMD_COMM="shm:" + name, NTPOLY_AMD_SHM_MB="64", NTPOLY_AMD_SPGEMM_FMA="1")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "complex_sum_chain_worker.py"), out],
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
    """the operands as complex column panels on two ranks sharing one GPU (shared-memory transport, grid 1 x 2 x 1, FMA arithmetic),
    Cosine and ComputeInverseRoot(5) with levels 2 and 1 in the same processes: 2 against 1 bit for bit on each panel, passes on
    both ranks with 2 (each panel makes its own) and none refused, none with 1, one session per inverse-root loop with either"""
    n, h = SIZES[0]
    two = run_world(2, tmp_path)
    for kind in WORKER_KINDS:
        want = expected_passes(kind, n, h)
        for r, p in enumerate(two):
            print("rank", r, kind, "counts (sessions, passes, refused)", [p["%s_counts_%d" % (kind, v)].tolist() for v in (2, 1)])
            got2, got1 = p["%s_counts_2" % kind].tolist(), p["%s_counts_1" % kind].tolist()
            assert got2[1] > 0 and got2 == [ROOT_LOOPS.get(kind, 0), want, 0], (r, kind, got2, want)
            assert got1 == [ROOT_LOOPS.get(kind, 0), 0, 0], (r, kind, got1)
            a = srt(tuple(p["%s_%s_2" % (kind, k)] for k in ("col", "row", "val")))
            b = srt(tuple(p["%s_%s_1" % (kind, k)] for k in ("col", "row", "val")))
            assert len(a[2]) > n // 2 and np.iscomplexobj(a[2]) and same(a, b), (r, kind)


# ------------------------------------------------------------------ untouched defaults
_DEFAULTS = """
import sys
sys.path.insert(0, %r)
import numpy as np
import ntpoly_amd as nt
from gen import banded_triplets
nt.init_comm()
nt.ConstructGlobalProcessGrid(1, 1, 1)
assert nt.get_option("complex_sum_chain") == 0
n = 512
p = nt.SolverParameters()
p.SetThreshold(1e-6)
p.SetMaxIterations(30)
A = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, 8, complex_=True, shift=1.0))
K = nt.Matrix_ps(n)
nt.TrigonometrySolvers.Cosine(A, K, p)
A = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, 8, complex_=True, shift=3.5))
nt.RootSolvers.ComputeInverseRoot(A, K, 5, p)
assert len(K.triplets()[2]) > n
B, A1 = (nt.Matrix_ps.from_triplets(n, *banded_triplets(n, h, complex_=True, shift=1.0)) for h in (3, 5))
Out = nt.Matrix_ps(n)
with nt.solver_session(True):
    taken = nt.sum_chain(B, 2.0, [A1], [-1.0], 1.0, Out)
assert taken is False and len(Out.triplets()[2]) == 0
print("COUNTS", nt.complex_sum_chain_counts(), nt.sum_chain_counts())
assert nt.complex_sum_chain_counts() == dict(sessions=0, passes=0, refused=0)
"""


def test_untouched_defaults_in_a_fresh_process():
    """nothing set: complex Cosine and ComputeInverseRoot(5) leave all three counters at zero, nt.sum_chain on complex operands
    returns False"""
    drop = ("NTPOLY_AMD_COMPLEX_SUM_CHAIN", "NTPOLY_AMD_SUM_CHAIN")
    env = dict({k: v for k, v in os.environ.items() if k not in drop}, PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", _DEFAULTS % os.path.join(ROOT, "tests")], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:]
