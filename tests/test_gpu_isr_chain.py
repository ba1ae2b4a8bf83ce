"""GPU: the polynomial chain of the Taylor square-root step in one pass (option isr_chain; csrc/slab_extra.hip k_sa_isr_chain,
engine.hpp ps_isr_chain5 / ps_isr_chain3).  Between the product X2 = X X and the next product the order-5 step builds
Temp = X2 + a X, Temp2 = b I + X, Temp2 += Temp, Temp += c I and the order-3 step X = I - X / 2, X += 0.375 X2 with the vocabulary at
threshold 0; the fused kernel reads X and X2 once and writes the outputs.

The kernel is reached with crafted operands through nt.isr_chain_step and compared with (i) the same sequence of vocabulary calls on
compressed columns (slab_algebra = 0) and (ii) a numpy restatement of AddSparseVectors.f90 at threshold 0 written here, complex
values part by part -- never with the fused code itself.  numpy's float64 products and sums are the correctly rounded ones the
kernel spells as __dmul_rn / __dadd_rn, so patterns are compared for equality and values with np.array_equal."""
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

# the constants of the order-5 step as solvers.cpp isr_taylor computes them
_aa, _bb, _cc = -40.0 / 35.0, 48.0 / 35.0, -64.0 / 35.0
A5 = (_aa - 1.0) / 2.0
B5 = _bb * (A5 + 1.0) - _cc - A5 * ((A5 + 1.0) * (A5 + 1.0))
C5 = _bb - B5 - A5 * (A5 + 1.0)


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
    nt.set_option("isr_chain", 1)


@pytest.fixture
def fma_on(nt):
    nt.set_option("spgemm_fma", 1)
    yield 1
    nt.set_option("spgemm_fma", 0)
    nt.set_option("slab_algebra", 1)
    nt.set_option("isr_chain", 1)


def srt(t):
    c, r, v = t
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def same(a, b):
    """sorted triplets: equal patterns, values equal part by part"""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(np.real(a[2]), np.real(b[2])) and
            np.array_equal(np.imag(a[2]), np.imag(b[2])))


# ------------------------------------------------------------------ operands
# a column is (rows, values) with values of shape (entries, parts): one part for real operands, (re, im) for complex ones
EMPTY_X, EMPTY_X2, DIAG_ONLY = {7, 40, 100}, {8, 40, 100}, {13}
BELOW, ABOVE = 60, 150   # columns whose runs lie beyond / before the diagonal row in both operands
KINDS = ("real", "complex", "complex_im0")


def _values(rng, k, parts, im0):
    v = 10.0 ** rng.uniform(-6.0, 0.0, (k, parts)) * rng.choice([-1.0, 1.0], (k, parts))
    if parts == 2 and im0:
        v[:, 1] = 0.0
    return v


def _runs(rng, n, empty, parts, im0):
    """{column: (rows, values)}: a run around the diagonal with half-widths 6..90 drawn per side, ~12 % holes inside, values
    log-uniform in [1e-6, 1] with a random sign per part"""
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
        cols[j] = (rows, _values(rng, len(rows), parts, im0))
    return cols


def _set(cols, j, r, v):
    rows, vals = cols[j]
    if r in rows:
        vals[rows == r] = v
    else:
        k = int(np.searchsorted(rows, r))
        cols[j] = (np.insert(rows, k, r), np.insert(vals, k, v, axis=0))


def _plant(X, X2, parts, im0):
    """cancellations, exact by construction (checked here in numpy): t = 0, q = 0, p = 0 on a diagonal, and for order 3 y = 0 on a
    diagonal and o = 0"""
    def mk(re, im):
        return np.array([re, 0.0 if im0 else im])[:parts]
    one = mk(1.0, 0.0)
    x = mk(0.731, -0.0417)
    # t = x2 + a x = 0
    _set(X, 20, 25, x)
    _set(X2, 20, 25, -(A5 * x))
    # q = (x2 + a x) + x = 0 off the diagonal: x2 = -x - fl(a x) is exact (the two terms lie within a factor two of each other)
    w = A5 * x
    x2 = -x - w
    assert np.all((x2 + w) + x == 0.0)
    _set(X, 30, 33, x)
    _set(X2, 30, 33, x2)
    # p = (x2 + a x) + c d = 0 on a diagonal
    for cand in (0.5, 0.25, 1.0, 0.125, 2.0, 0.75, 0.375, 1.5):
        xd = mk(cand, 0.25 * cand)
        wd = A5 * xd
        x2d = -(C5 * one) - wd
        if np.all((x2d + wd) + C5 * one == 0.0):
            break
    else:
        raise AssertionError("no exact diagonal cancellation among the candidates")
    _set(X, 50, 50, xd)
    _set(X2, 50, 50, x2d)
    # order 3: y = d - x / 2 = 0 on a diagonal (x = 2); o = 0.375 x2 + (-x / 2) = 0 off it (x2 = 1/2, x = 3/8: every product is exact)
    _set(X, 70, 70, mk(2.0, 0.0))
    p2 = mk(0.5, 0.25)
    xo = 2.0 * (0.375 * p2)
    assert np.all(0.375 * p2 + (-0.5) * xo == 0.0)
    _set(X2, 80, 84, p2)
    _set(X, 80, 84, xo)


@pytest.fixture(scope="module")
def operands():
    out = {}
    for kind in KINDS:
        rng = np.random.default_rng(20261019)
        parts, im0 = (1 if kind == "real" else 2), kind == "complex_im0"
        X = _runs(rng, N, EMPTY_X, parts, im0)
        X2 = _runs(rng, N, EMPTY_X2, parts, im0)
        _plant(X, X2, parts, im0)
        out[kind] = (X, X2)
    return out


def _triplets(cols):
    c, r, v = [], [], []
    for j in sorted(cols):
        rows, vals = cols[j]
        c.append(np.full(len(rows), j + 1))
        r.append(rows + 1)
        v.append(vals[:, 0] if vals.shape[1] == 1 else vals[:, 0] + 1j * vals[:, 1])
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
    """alpha a + beta b on sorted sparse vectors (rows, values[entries, parts]), the scaled values rounded, then added, part by
    part: inside the overlap of the two lists an entry is kept iff its value is not zero (|value| > 0: some part is not zero),
    beyond the end of one list the tail of the other is copied unfiltered"""
    (ra, va), (rb, vb) = a, b
    parts = va.shape[1]
    if len(ra) == 0 and len(rb) == 0:
        return ra, va
    rows = np.union1d(ra, rb)
    ia, ib = np.isin(rows, ra), np.isin(rows, rb)
    wa, wb = np.zeros((len(rows), parts)), np.zeros((len(rows), parts))
    wa[ia] = alpha * va
    wb[ib] = beta * vb
    s = np.where((ia & ib)[:, None], wa + wb, np.where(ia[:, None], wa, wb))
    lim = min(ra[-1] if len(ra) else -1, rb[-1] if len(rb) else -1)
    nz = np.any(s != 0.0, axis=1)
    keep = (rows > lim) | nz
    stats[tag + "_cancelled"] = stats.get(tag + "_cancelled", 0) + int((ia & ib & ~nz).sum())
    stats[tag + "_only_a"] = stats.get(tag + "_only_a", 0) + int((ia & ~ib).sum())
    stats[tag + "_only_b"] = stats.get(tag + "_only_b", 0) + int((~ia & ib).sum())
    stats["underflow"] = stats.get("underflow", 0) + int((~nz & ~(ia & ib)).sum())
    return rows[keep], s[keep]


def restated(X, X2, order):
    """the outputs of the vocabulary sequence, column by column, and branch statistics"""
    parts = next(iter(X.values()))[1].shape[1]
    empty = (np.zeros(0, dtype=np.int64), np.zeros((0, parts)))
    one = np.array([[1.0, 0.0][:parts]])
    st, out1, out2 = {}, {}, {}
    for j in range(N):
        x, x2, d = X.get(j, empty), X2.get(j, empty), (np.array([j]), one)
        lo = min([c[0][0] for c in (x, x2) if len(c[0])] or [j])
        hi = max([c[0][-1] for c in (x, x2) if len(c[0])] or [j])
        st["diag_below_runs"] = st.get("diag_below_runs", 0) + int(j < lo)
        st["diag_above_runs"] = st.get("diag_above_runs", 0) + int(j > hi)
        st["diag_only"] = st.get("diag_only", 0) + int(len(x[0]) == 1 and len(x2[0]) == 1 and x[0][0] == j == x2[0][0])
        if order == 5:
            t = add_sparse(x, A5, x2, 1.0, st, "t")      # IncrementMatrix(X, Temp, a)
            u = add_sparse(x, 1.0, d, B5, st, "u")       # CopyMatrix(I, Temp2); ScaleMatrix(Temp2, b); IncrementMatrix(X, Temp2)
            q = add_sparse(t, 1.0, u, 1.0, st, "q")      # IncrementMatrix(Temp, Temp2)
            p = add_sparse(d, C5, t, 1.0, st, "p")       # IncrementMatrix(I, Temp, c)
            if len(q[0]):
                out1[j] = q
            if len(p[0]):
                out2[j] = p
        else:
            y = add_sparse(d, 1.0, x, -0.5, st, "y")     # ScaleMatrix(X, -1/2); IncrementMatrix(I, X)
            o = add_sparse(x2, 0.375, y, 1.0, st, "o")   # IncrementMatrix(Temp, X, 0.375)
            if len(o[0]):
                out1[j] = o
    return out1, out2, st


@pytest.fixture(scope="module")
def references(operands):
    return {(kind, order): restated(*operands[kind], order) for kind in KINDS for order in (5, 3)}


def test_the_inputs_reach_every_branch(operands, references):
    """from the operands and the numpy restatement alone: columns empty in one operand and in both, a diagonal-only column, the
    diagonal below and above both runs, columns 0 and N - 1, and in every merge both-present sums that cancel and one-sided
    entries from either side; no scaled entry underflows (the restatement would hold a stored zero the runs cannot)"""
    for kind in KINDS:
        X, X2 = operands[kind]
        assert 7 not in X and 7 in X2 and 8 in X and 8 not in X2 and 40 not in X and 40 not in X2
        assert 0 in X and 0 in X2 and N - 1 in X and N - 1 in X2
        assert X[BELOW][0][0] > BELOW < X2[BELOW][0][0] and X[ABOVE][0][-1] < ABOVE > X2[ABOVE][0][-1]
        if kind == "complex_im0":
            assert all(np.all(v[:, 1] == 0.0) for _, v in list(X.values()) + list(X2.values()))
        for order, merges in ((5, "tuqp"), (3, "yo")):
            st = references[(kind, order)][2]
            print(kind, order, st)
            assert st["underflow"] == 0
            assert st["diag_below_runs"] >= 1 and st["diag_above_runs"] >= 1 and st["diag_only"] == 1, st
            for m in merges:
                assert st[m + "_only_a"] > 0 and st[m + "_only_b"] > 0, (m, st)
                if m != "u":   # (x + b d with b > 1 and |x| <= 2 cannot cancel)
                    assert st[m + "_cancelled"] > 0, (m, st)


def _vocabulary(nt, MX, M2, order):
    """the calls of solvers.cpp isr_taylor through the C ABI on compressed columns"""
    I = nt.Matrix_ps(N)
    I.FillIdentity()
    if order == 5:
        T = nt.Matrix_ps(M2)
        T.Increment(MX, A5, 0.0)
        T2 = nt.Matrix_ps(I)
        T2.Scale(B5)
        T2.Increment(MX, 1.0, 0.0)
        T2.Increment(T, 1.0, 0.0)
        T.Increment(I, C5, 0.0)
        return T2, T
    Y = nt.Matrix_ps(MX)
    Y.Scale(-0.5)
    Y.Increment(I, 1.0, 0.0)
    Y.Increment(M2, 0.375, 0.0)
    return Y, None


def _check_chain(nt, operands, references, kind, order):
    X, X2 = operands[kind]
    w1, w2, _ = references[(kind, order)]
    want = [_triplets(w1)] + ([_triplets(w2)] if order == 5 else [])
    MX, M2 = _matrix(nt, X), _matrix(nt, X2)
    before = [srt(m.triplets()) for m in (MX, M2)]
    # (i) the vocabulary on compressed columns against (ii) the restatement
    nt.set_option("slab_algebra", 0)
    V1, V2 = _vocabulary(nt, MX, M2, order)
    nt.set_option("slab_algebra", 1)
    for V, w in zip((V1, V2), want):
        assert same(srt(V.triplets()), w), "compressed columns against the restatement"
    # the fused chain
    O1, O2 = nt.Matrix_ps(N), nt.Matrix_ps(N)
    c0, s0 = nt.isr_chain_counts(), nt.slab_algebra_counts()
    with nt.solver_session(True):
        took = nt.isr_chain_step(MX, M2, order, A5, B5, C5, O1, O2)
    c1, s1 = nt.isr_chain_counts(), nt.slab_algebra_counts()
    assert took is True
    key = "order5" if order == 5 else "order3"
    assert {k: c1[k] - c0[k] for k in c1} == {k: int(k == key) for k in c1}
    assert s1["merges"] - s0["merges"] == (4 if order == 5 else 2) and s1["refusals"] == s0["refusals"]
    for m, b in zip((MX, M2), before):
        assert same(srt(m.triplets()), b), "the operands are as they were"
    got = [srt(O1.triplets())] + ([srt(O2.triplets())] if order == 5 else [])
    for g, w, V, name in zip(got, want, (V1, V2), ("first output", "second output")):
        print(kind, order, name, "entries", len(w[2]))
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), name + ": pattern"
        assert same(g, w), name + ": values against the restatement"
        assert same(g, srt(V.triplets())), name + ": values against compressed columns"
    if order == 3:
        assert len(O2.triplets()[2]) == 0   # (untouched)


@pytest.mark.parametrize("order", [5, 3])
def test_chain_bit_for_bit_real(nt, fma, operands, references, order):
    _check_chain(nt, operands, references, "real", order)


@pytest.mark.parametrize("order", [5, 3])
@pytest.mark.parametrize("kind", ["complex", "complex_im0"])
def test_chain_bit_for_bit_complex(nt, fma_on, operands, references, kind, order):
    """(a complex session needs FMA arithmetic)"""
    _check_chain(nt, operands, references, kind, order)


# ------------------------------------------------------------------ refusals
def test_refusals_leave_everything_as_it_was(nt, fma):
    n, j = 4099, 5
    col = lambda f, l, v=None: {j: (np.arange(f, l + 1), (np.linspace(0.1, 0.9, l - f + 1) if v is None else v)[:, None])}

    def refused(MX, M2, order):
        O1, O2 = nt.Matrix_ps(n), nt.Matrix_ps(n)
        before = [srt(m.triplets()) for m in (MX, M2)]
        c0, s0 = nt.isr_chain_counts(), nt.slab_algebra_counts()
        with nt.solver_session(True):
            took = nt.isr_chain_step(MX, M2, order, A5, B5, C5, O1, O2)
        c1, s1 = nt.isr_chain_counts(), nt.slab_algebra_counts()
        assert took is None
        assert c1 == dict(c0, refused=c0["refused"] + 1), (c0, c1)
        assert s1 == s0, (s0, s1)   # (a refused chain is no operation and no refusal of the session)
        for m, b in zip((MX, M2), before):
            assert same(srt(m.triplets()), b)
        assert len(O1.triplets()[2]) == 0 and len(O2.triplets()[2]) == 0

    # the runs of X and X2 n / 2 rows apart in one column: the union extent is beyond what the column's slots bound
    MX, far, near = _matrix(nt, col(0, 9), n=n), _matrix(nt, col(n // 2 + 1, n // 2 + 11), n=n), _matrix(nt, col(4, 20), n=n)
    for order in (5, 3):
        refused(MX, far, order)
    # the same column with the runs side by side is taken
    for order in (5, 3):
        O1, O2 = nt.Matrix_ps(n), nt.Matrix_ps(n)
        with nt.solver_session(True):
            assert nt.isr_chain_step(MX, near, order, A5, B5, C5, O1, O2) is True
        c, r, v = O1.triplets()
        assert (c == j + 1).sum() == 21 and len(v) == 21 + (n - 1)   # (rows 0 .. 20 of the column, a diagonal everywhere else)
    # an operand with a stored zero enters as a read-only view
    v = np.linspace(0.1, 0.9, 17)
    v[8] = 0.0
    zero = _matrix(nt, col(4, 20, v), n=n)
    for order in (5, 3):
        refused(MX, zero, order)
        refused(zero, near, order)
    # order 3, a one-sided x2 = 5e-324 beyond X's last row: 0.375 x 5e-324 rounds to zero
    v = np.linspace(0.1, 0.9, 17)
    v[-1] = 5e-324
    tiny = _matrix(nt, col(4, 20, v), n=n)
    kept = tiny.triplets()[2]
    if kept[-1] != 5e-324:
        assert kept[-1] == 0.0
        pytest.skip("the triplet entry does not keep a subnormal: the underflow leg cannot be built")
    refused(MX, tiny, 3)


# ------------------------------------------------------------------ the solver
REAL = (2560, 20, 2.0, False)      # banded_triplets(2560, 20, shift = 2): the operand of test_gpu_slab_algebra.py's square-root case
CPLX = (4000, 30, 2.5, True)       # the complex operand of test_gpu_complex_tile.py's session test, at n = 4000


def isr_solve(nt, H, n, order, inverse):
    p = nt.SolverParameters()
    p.SetThreshold(1e-8)
    p.SetConvergeDiff(1e-8)
    Out = nt.Matrix_ps(n)
    c0, s0 = nt.isr_chain_counts(), nt.slab_algebra_counts()
    nt.SquareRootSolvers.with_order(H, Out, p, inverse, order)
    c1, s1 = nt.isr_chain_counts(), nt.slab_algebra_counts()
    tr = nt.solver_trace()
    return dict(out=srt(Out.triplets()), iters=tr["iterations"], value=np.asarray(tr["value"]).copy(),
                chain={k: c1[k] - c0[k] for k in c1}, refusals=s1["refusals"] - s0["refusals"], merges=s1["merges"] - s0["merges"])


@pytest.fixture(scope="module")
def solver_operands(nt):
    return {c: nt.Matrix_ps.from_triplets(spec[0], *banded_triplets(spec[0], spec[1], shift=spec[2], complex_=spec[3]))
            for c, spec in (("real", REAL), ("complex", CPLX))}


def _solver_case(nt, solver_operands, kind, order, inverse):
    H, n = solver_operands[kind], (REAL if kind == "real" else CPLX)[0]
    nt.set_option("isr_chain", 0)
    off = isr_solve(nt, H, n, order, inverse)
    nt.set_option("isr_chain", 1)
    on = isr_solve(nt, H, n, order, inverse)
    print(kind, "order", order, "inverse", inverse, "iterations", on["iters"], "chain", on["chain"], "refusals", on["refusals"],
          off["refusals"], "merges", on["merges"], off["merges"])
    assert off["chain"] == dict(order5=0, order3=0, refused=0)
    assert on["iters"] == off["iters"] and on["iters"] >= 6
    assert np.array_equal(on["value"], off["value"]), "convergence values, bit for bit"
    assert same(on["out"], off["out"]), "result triplets, bit for bit"
    key = "order5" if order == 5 else "order3"
    if nt.get_option("spgemm_fma") == 1:
        assert on["chain"] == {k: (on["iters"] if k == key else 0) for k in on["chain"]}, on["chain"]
    else:
        # (unfused arithmetic: a product whose operands have become sparse inside wide extents is handed to the general kernels
        # -- psmatrix.cpp runs_dense -- and near convergence X and X X both come back in compressed columns, not run-like: that
        # ONE iteration is kept out by the gate of ps_isr_chain5 / 3 before anything is counted -- neither fused nor refused, as
        # ntpoly_amd_isr_chain_counts documents -- and is the vocabulary's.  Measured on this operand: 11 of 12 iterations fused
        # in order 5, 13 of 14 in order 3)
        assert on["chain"] == {k: (on["iters"] - 1 if k == key else 0) for k in on["chain"]}, on["chain"]
    assert on["refusals"] <= off["refusals"]
    if on["refusals"] == off["refusals"] == 0:
        assert on["merges"] == off["merges"]   # (a fused chain counts as the merges it replaces)


@pytest.mark.parametrize("inverse", [True, False], ids=["inverse", "root"])
@pytest.mark.parametrize("order", [5, 3])
def test_solver_real(nt, fma, solver_operands, order, inverse):
    _solver_case(nt, solver_operands, "real", order, inverse)


@pytest.mark.parametrize("inverse", [True, False], ids=["inverse", "root"])
@pytest.mark.parametrize("order", [5, 3])
def test_solver_complex(nt, fma_on, solver_operands, order, inverse):
    _solver_case(nt, solver_operands, "complex", order, inverse)


def test_gates(nt, fma_on, solver_operands):
    """slab_algebra = 0, unfused arithmetic on a complex operand and order 2 fuse nothing: the results of option 0"""
    none = dict(order5=0, order3=0, refused=0)
    H, n = solver_operands["real"], REAL[0]
    nt.set_option("isr_chain", 0)
    want = isr_solve(nt, H, n, 5, True)
    want2 = isr_solve(nt, H, n, 2, True)
    nt.set_option("isr_chain", 1)
    nt.set_option("slab_algebra", 0)
    a = isr_solve(nt, H, n, 5, True)
    nt.set_option("slab_algebra", 1)
    b = isr_solve(nt, H, n, 2, True)
    assert a["chain"] == none == b["chain"]
    assert a["iters"] == want["iters"] and same(a["out"], want["out"])
    assert b["iters"] == want2["iters"] and same(b["out"], want2["out"]) and np.array_equal(b["value"], want2["value"])
    Hc, nc = solver_operands["complex"], CPLX[0]
    nt.set_option("spgemm_fma", 0)
    c = isr_solve(nt, Hc, nc, 5, True)
    nt.set_option("isr_chain", 0)
    d = isr_solve(nt, Hc, nc, 5, True)
    nt.set_option("isr_chain", 1)
    assert c["chain"] == none == d["chain"]
    assert c["iters"] == d["iters"] and same(c["out"], d["out"]) and np.array_equal(c["value"], d["value"])


# ------------------------------------------------------------------ two ranks
def run_world(world, tmp_path):
    out = str(tmp_path / ("isr%d" % world))
    name = "i%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name, NTPOLY_AMD_SHM_MB="64",
                   NTPOLY_AMD_SPGEMM_FMA="1")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "isr_chain_worker.py"), out],
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


def test_two_ranks_equal_one(tmp_path):
    """InverseSquareRoot (order 5) of a real band, n = 2500, as column panels on two ranks (shared-memory transport, FMA arithmetic):
    the chain counters move on both ranks, the gathered result has the pattern of the one-rank run and its values to 1e-10 -- the
    bound test_gpu_thin_panels.py holds this solver to across ranks (panel products sum in another order; the chain adds nothing)"""
    one = run_world(1, tmp_path)[0]
    two = run_world(2, tmp_path)
    cat = lambda k: np.concatenate([p[k] for p in two])
    assert np.array_equal(cat("col"), one["col"]) and np.array_equal(cat("row"), one["row"])
    print("max |d|", float(np.max(np.abs(cat("val") - one["val"]))))
    assert np.max(np.abs(cat("val") - one["val"])) <= 1e-10
    iters = int(one["iters"][0])
    assert one["counts"].tolist() == [iters, 0, 0]
    for r, p in enumerate(two):
        print("rank", r, "counts (order5, order3, refused)", p["counts"].tolist(), "iterations", int(p["iters"][0]))
        assert int(p["iters"][0]) == iters
        assert p["counts"][0] > 0 and p["counts"][1] == 0, (r, p["counts"])
