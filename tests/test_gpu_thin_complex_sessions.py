"""GPU, one rank, FMA arithmetic: the complex thin-operand gather kernels of slab sessions (ntpoly_amd/csrc/spgemm_thin.hip
k_thin_slab_left / k_thin_slab_right on (re, im) runs; kernels.hip slab_multiply_c, option thin_slab_complex).

A product of a complex session whose left or right operand holds at most 8 entries per column -- an identity, the factor
(3 I - Z Y) / 2 of a square-root loop near convergence -- is computed entry by entry with the reference's own complex
multiply-add over ascending k (MultiplyBlock.f90:9-36, PruneList.f90:8-38): bit for bit the oracle's product, where the
complex tile kernel is a 1e-13 tolerance mode.  The tests reach slab_multiply_c with operands of their own through the
diagnostic session hook (nt.solver_session)."""
import numpy as np
import pytest

from gen import banded_triplets
from test_gpu_complex_tile import close, srt

pytestmark = pytest.mark.gpu
CPLX = ("complex_left", "complex_right")


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture()
def fma(nt):
    nt.set_option("spgemm_fma", 1)
    nt.set_option("complex_tile", 1)
    nt.set_option("thin_slab_complex", 1)
    yield
    nt.set_option("thin_slab_complex", 1)
    nt.set_option("spgemm_fma", 0)


def nonzero(t):
    """slab form holds no stored zeros (slab_enter_c refuses them)"""
    c, r, v = t
    k = v != 0
    return c[k], r[k], v[k]


def wide_operand(n, h, empty_cols=()):
    c, r, v = nonzero(banded_triplets(n, h, complex_=True, shift=0.37))
    k = ~np.isin(c, np.asarray(empty_cols, dtype=np.int64))
    return c[k], r[k], v[k]


def thin_operand(n, seed, empty_rows=(), long_cols=()):
    """a diagonal with 2 % of its entries dropped plus extra entries within reach <= 4 of it (about 3 per column); long_cols:
    (column, entries) -- columns that list that many consecutive rows around their diagonal position"""
    rng = np.random.default_rng(seed)
    j = np.arange(1, n + 1)
    keep = rng.random(n) >= 0.02
    cols, rows = [j[keep]], [j[keep]]
    for _ in range(2):
        off = rng.integers(1, 5, n) * rng.choice([-1, 1], n)
        ok = (j + off >= 1) & (j + off <= n) & (rng.random(n) < 0.9)
        cols.append(j[ok])
        rows.append((j + off)[ok])
    for (cj, m) in long_cols:
        r0 = max(1, min(n - m + 1, cj - m // 2))
        cols.append(np.full(m, cj))
        rows.append(np.arange(r0, r0 + m))
    col, row = np.concatenate(cols), np.concatenate(rows)
    key = np.unique(col.astype(np.int64) * (n + 1) + row)
    col, row = (key // (n + 1)).astype(np.int32), (key % (n + 1)).astype(np.int32)
    k = ~np.isin(row, np.asarray(empty_rows, dtype=np.int64))
    col, row = col[k], row[k]
    val = np.where(col == row, 1.0, 0.05) * (rng.uniform(0.5, 1.5, len(col)) + 1j * rng.uniform(-0.7, 0.7, len(col)))
    return col, row, val


def delta(c1, c0):
    return {k: c1[k] - c0[k] for k in c0}


def assert_bits(got, want, what):
    assert len(got[2]) == len(want[2]) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what + ": pattern"
    assert np.array_equal(got[2].real, want[2].real) and np.array_equal(got[2].imag, want[2].imag), what + ": values"


def session_product(nt, X, Y, n, alpha, thr):
    C = nt.Matrix_ps(n)
    c0 = nt.thin_slab_counts()
    with nt.solver_session(True):
        C.Gemm(X, Y, None, alpha, 0.0, thr)
        thin = nt.last_spgemm_thin()
        slab = nt.last_spgemm_stats()["slab"]
    return srt(C.triplets()), thin, slab, delta(nt.thin_slab_counts(), c0)


@pytest.mark.parametrize("n,h", [(1003, 20), (2048, 70)])
@pytest.mark.parametrize("alpha,thr", [(-0.5, 1e-7), (1.0, 0.0)])
def test_one_thin_product_is_the_oracles_bit_for_bit(nt, fma, n, h, alpha, thr):
    """C = alpha T B (thin left operand) and C = alpha B T (thin right operand) inside a complex session: pattern and values are
    the oracle's, the complex counters move by one; n = 1003 is no multiple of 4, 8 or 64, h = 70 makes block windows of more
    than 128 rows (two passes of the left kernel's two-chunk unroll).  A few empty columns of B, a few empty rows of T.  With the
    option off the same products run on the complex tile kernel: its 1e-13 tolerance, and no counter moves."""
    from oracle import oracle_py as O
    bt = wide_operand(n, h, empty_cols=(1, 17, 500, n))
    tt = thin_operand(n, n + h, empty_rows=(3, 64, 700, n - 1))
    assert len(tt[2]) <= 8 * n < len(bt[2])
    B, T = nt.Matrix_ps.from_triplets(n, *bt), nt.Matrix_ps.from_triplets(n, *tt)
    Bo, To = O.Mat.from_triplets(n, n, *bt), O.Mat.from_triplets(n, n, *tt)
    for (X, Y, Xo, Yo, side) in ((T, B, To, Bo, "complex_left"), (B, T, Bo, To, "complex_right")):
        want = srt(O.ps_multiply(Xo, Yo, None, alpha, 0.0, thr).triplets())
        got, thin, slab, d = session_product(nt, X, Y, n, alpha, thr)
        print(side, "n", n, "h", h, "entries", len(got[2]), "counters", d)
        assert thin == 1 and slab == 1, (side, thin, slab)
        assert d[side] == 1 and sum(d.values()) == 1, d
        assert_bits(got, want, "%s n=%d h=%d" % (side, n, h))
        nt.set_option("thin_slab_complex", 0)
        try:
            got0, thin0, slab0, d0 = session_product(nt, X, Y, n, alpha, thr)
        finally:
            nt.set_option("thin_slab_complex", 1)
        assert thin0 == 0 and slab0 == 1 and sum(d0.values()) == 0, (thin0, slab0, d0)
        close(got0, want, n, thr, side + " on the tile kernel")


def test_thin_factor_inside_wide_extents(nt, fma):
    """P = A A with A = I + E, |E| ~ 1e-3 on a band of h = 40, pruned so that at most 8 entries per column survive -- a few of
    them far from the diagonal, so the runs of P stay wide and mostly holes: T_k late in a square-root loop.  P B and B P in the
    same session are thin products, each the oracle's product of the same operands (P read back) bit for bit."""
    from oracle import oracle_py as O
    n, h, thr = 1500, 40, 5e-5
    rng = np.random.default_rng(7)
    c, r, _ = banded_triplets(n, h, complex_=True)
    dist = np.abs(r.astype(np.int64) - c)
    far = (dist >= 35) & (rng.random(len(c)) < 0.02)   # (survivors far out: they keep the extents wide)
    mag = np.where(dist == 0, 1.0, np.where(far, 1e-3, 1e-3 * np.exp(-1.0 * dist)))
    v = mag * rng.uniform(0.5, 1.0, len(c)) * np.exp(1j * np.where(dist == 0, 0.0, rng.uniform(-3, 3, len(c))))
    bt = wide_operand(n, 30)
    A, B = nt.Matrix_ps.from_triplets(n, c, r, v), nt.Matrix_ps.from_triplets(n, *bt)
    P, PB, BP = nt.Matrix_ps(n), nt.Matrix_ps(n), nt.Matrix_ps(n)
    c0 = nt.thin_slab_counts()
    with nt.solver_session(True):
        P.Gemm(A, A, None, 1.0, 0.0, thr)
        c1 = nt.thin_slab_counts()
        PB.Gemm(P, B, None, 1.0, 0.0, 1e-9)
        c2 = nt.thin_slab_counts()
        BP.Gemm(B, P, None, 1.0, 0.0, 1e-9)
        c3 = nt.thin_slab_counts()
    pt = P.triplets()
    span = np.array([pt[1][pt[0] == j].max() - pt[1][pt[0] == j].min() for j in (100, 700, 1400)])
    print("entries of P per column", len(pt[2]) / n, "spans", span, "counters", delta(c1, c0), delta(c2, c1), delta(c3, c2))
    assert len(pt[2]) <= 8 * n
    assert sum(delta(c1, c0).values()) == 0        # (A A: both operands wide, the tile kernel)
    assert delta(c2, c1)["complex_left"] == 1 and delta(c3, c2)["complex_right"] == 1
    Po, Bo = O.Mat.from_triplets(n, n, *pt), O.Mat.from_triplets(n, n, *bt)
    assert_bits(srt(PB.triplets()), srt(O.ps_multiply(Po, Bo, None, 1.0, 0.0, 1e-9).triplets()), "P B")
    assert_bits(srt(BP.triplets()), srt(O.ps_multiply(Bo, Po, None, 1.0, 0.0, 1e-9).triplets()), "B P")


def test_long_columns_of_a_thin_right_operand(nt, fma):
    """three columns of the thin right operand list 65, 130 and 200 entries -- more than the kernel's LDS list of 64: the complex
    kernel lists such a run again in pieces for every chunk of rows (no hand-back to the tile kernel, which is another
    arithmetic): still a thin-right product, the oracle's bit for bit, nothing refused"""
    from oracle import oracle_py as O
    n, h, thr = 1500, 20, 1e-8
    bt = wide_operand(n, h)
    tt = thin_operand(n, 11, long_cols=((300, 65), (800, 130), (1290, 200)))
    per_col = np.bincount(tt[0], minlength=n + 1)
    assert len(tt[2]) <= 8 * n and sorted(per_col[[300, 800, 1290]]) == [65, 130, 200]
    B, T = nt.Matrix_ps.from_triplets(n, *bt), nt.Matrix_ps.from_triplets(n, *tt)
    r0 = nt.slab_algebra_counts()["refusals"]
    got, thin, slab, d = session_product(nt, B, T, n, 1.0, thr)
    assert thin == 1 and d["complex_right"] == 1 and sum(d.values()) == 1, (thin, d)
    assert nt.slab_algebra_counts()["refusals"] == r0
    want = srt(O.ps_multiply(O.Mat.from_triplets(n, n, *bt), O.Mat.from_triplets(n, n, *tt), None, 1.0, 0.0, thr).triplets())
    assert_bits(got, want, "B T with long columns")


@pytest.mark.parametrize("solver", ["inverse_square_root", "sign"])
def test_loops_with_and_without_the_thin_kernels(nt, fma, solver):
    """InverseSquareRoot and SignFunction on the operands of test_gpu_complex_tile.py's session tests (n = 4000, stored zeros
    filtered: a stored zero is what slab form cannot hold) with thin_slab_complex = 1 against 0: the same iteration count, the
    result within 1e-13 of the largest entry, convergence values to rtol 1e-8 (atol 1e-12 n: they are sums over n columns of
    differences of nearly equal iterates), at least one product on the complex gather kernels with the option on, none with
    it off."""
    n, thr = 4000, 1e-8
    h, shift, conv = (30, 2.5, 1e-8) if solver == "inverse_square_root" else (40, 0.0, 1e-9)
    A = nt.Matrix_ps.from_triplets(n, *nonzero(banded_triplets(n, h, complex_=True, shift=shift)))
    res = {}
    for opt in (1, 0):
        nt.set_option("thin_slab_complex", opt)
        try:
            p = nt.SolverParameters()
            p.SetThreshold(thr)
            p.SetConvergeDiff(conv)
            Out = nt.Matrix_ps(n)
            c0, s0 = nt.thin_slab_counts(), nt.slab_algebra_counts()
            if solver == "inverse_square_root":
                nt.SquareRootSolvers.InverseSquareRoot(A, Out, p)
            else:
                nt.SignSolvers.ComputeSign(A, Out, p)
            d, s = delta(nt.thin_slab_counts(), c0), delta(nt.slab_algebra_counts(), s0)
            tr = nt.solver_trace()
            print(solver, "thin_slab_complex", opt, "iterations", tr["iterations"], "thin products", d, "slab operations", s)
            res[opt] = (srt(Out.triplets()), tr["iterations"], np.asarray(tr["value"]), d)
        finally:
            nt.set_option("thin_slab_complex", 1)
    assert res[1][1] == res[0][1] and res[1][1] >= 3, (res[1][1], res[0][1])
    assert sum(res[1][3][k] for k in CPLX) >= 1, res[1][3]
    assert sum(res[0][3].values()) == 0, res[0][3]
    assert np.allclose(res[1][2], res[0][2], rtol=1e-8, atol=1e-12 * n), (res[1][2], res[0][2])
    close(res[1][0], res[0][0], n, thr, solver + " with / without the complex thin kernels")
