"""GPU, one rank, real operands: the `double` instantiations of the thin-operand gather kernels of slab sessions
(ntpoly_amd/csrc/spgemm_thin.hip k_thin_slab_left<double> / k_thin_slab_right<double>; kernels.hip slab_multiply) -- the kernels
every real square-root, inverse-square-root, sign and polynomial loop multiplies its near-identity factor with.

The contract is the engine's own: in FMA arithmetic every product of a session equals oracle_py.ps_multiply in FMA mode in
pattern and bits, whichever kernel computes it -- the gather kernels and the MFMA tile kernel run the same fma chain over
ascending k.  So every comparison here is np.array_equal; there is no tolerance.  The counters (nt.thin_slab_counts() real_left /
real_right) prove which kernel produced the bits.  Operands and their promised properties: tests/thin_cases.py, asserted without
a GPU by tests/test_thin_cases_cpu.py.  The tests reach slab_multiply with operands of their own through the diagnostic session
hook (nt.solver_session)."""
import time

import numpy as np
import pytest

import thin_cases as tc

pytestmark = pytest.mark.gpu
REAL = ("real_left", "real_right")


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    t0 = time.perf_counter()
    yield nt
    print("\n[wall time] tests/test_gpu_thin_real_sessions.py: %.1f s" % (time.perf_counter() - t0))


@pytest.fixture()
def fma(nt):
    from oracle import oracle_py as O
    nt.set_option("spgemm_fma", 1)
    nt.set_option("thin_left", 1)
    O.set_fma(True)
    yield O
    O.set_fma(False)
    nt.set_option("thin_left", 1)
    nt.set_option("spgemm_fma", 0)


def srt(t):
    c, r, v = (np.asarray(x) for x in t)
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def delta(c1, c0):
    return {k: c1[k] - c0[k] for k in c0}


def assert_bits(got, want, what):
    assert len(got[2]) == len(want[2]), "%s: %d vs %d entries" % (what, len(got[2]), len(want[2]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what + ": pattern"
    assert np.array_equal(got[2], want[2]), what + ": values"


def oracle_product(O, n, X, Y, alpha, thr):
    return srt(O.ps_multiply(O.Mat.from_triplets(n, n, *X), O.Mat.from_triplets(n, n, *Y), None, alpha, 0.0, thr).triplets())


def session_product(nt, X, Y, n, alpha, thr):
    """C = alpha X Y inside a real session -> (triplets, last_spgemm_thin, last_spgemm_stats slab, counter deltas, refusals)"""
    C = nt.Matrix_ps(n)
    c0, r0 = nt.thin_slab_counts(), nt.slab_algebra_counts()["refusals"]
    with nt.solver_session(False):
        C.Gemm(X, Y, None, alpha, 0.0, thr)
        thin = nt.last_spgemm_thin()
        slab = nt.last_spgemm_stats()["slab"]
    return srt(C.triplets()), thin, slab, delta(nt.thin_slab_counts(), c0), nt.slab_algebra_counts()["refusals"] - r0


def assert_taken(res, side, what):
    """the product ran on the gather kernel of `side` ("left" / "right"), or on the tile kernel in slab form ("none")"""
    _, thin, slab, d, refused = res
    print(what, "-> thin", thin, "slab", slab, "counters", d, "refusals", refused)
    assert slab == 1 and refused == 0, (what, slab, refused)
    if side == "none":
        assert thin == 0 and sum(d.values()) == 0, (what, thin, d)
    else:
        assert thin == 1 and d["real_" + side] == 1 and sum(d.values()) == 1, (what, thin, d)


@pytest.mark.parametrize("n,h", tc.BASE_SHAPES)
def test_one_thin_product_is_the_oracles_bit_for_bit(nt, fma, n, h):
    """C = alpha T B (k_thin_slab_left) and C = alpha B T (k_thin_slab_right): pattern and bits are the oracle's, the real counter
    of the side moves by one and nothing else moves.  n = 1003 is no multiple of 4, 16 or 64 (the clipped last column group, a
    last window past the last row); h = 70 makes windows of more than 128 rows (two passes of the left kernel's two-chunk
    unroll).  A few empty columns of B, a few empty rows of T.  With thin_left = 0 the same product runs on the tile kernel: no
    thin counter moves, the bits are the same."""
    case = tc.base_case(n, h)
    bt, tt = case["wide"], case["thin"]
    B, T = nt.Matrix_ps.from_triplets(n, *bt), nt.Matrix_ps.from_triplets(n, *tt)
    for alpha, thr in tc.BASE_SCALARS:
        for (X, Y, Xt, Yt, side) in ((T, B, tt, bt, "left"), (B, T, bt, tt, "right")):
            what = "%s n=%d h=%d alpha=%g thr=%g" % (side, n, h, alpha, thr)
            want = oracle_product(fma, n, Xt, Yt, alpha, thr)
            res = session_product(nt, X, Y, n, alpha, thr)
            assert_taken(res, side, what)
            assert_bits(res[0], want, what)
            nt.set_option("thin_left", 0)
            try:
                res0 = session_product(nt, X, Y, n, alpha, thr)
            finally:
                nt.set_option("thin_left", 1)
            assert_taken(res0, "none", what + " thin_left=0")
            assert_bits(res0[0], want, what + " on the tile kernel")


def test_64_and_65_entries_in_a_column_of_the_thin_right_operand(nt, fma):
    """k_thin_slab_right<double> lists THIN_MAXK = 64 non-zeros of a column in LDS (`q < THIN_MAXK` in list, `nk > THIN_MAXK`
    behind it).  Columns of exactly 64 -- one of them spread with holes over a run of 200 rows, listed by four calls of list --
    stay on the gather kernel.  One entry more in one column and the real kernel raises ThinSlabArgs::flag: slab_multiply reads it
    back, zeroes the counts and repeats the product on the tile kernel with the same plan and output slots -- real_right does not
    move, last_spgemm_thin() is 0, the product is still a slab product, nothing is refused, and the bits are the oracle's.
    Columns of 130 and 200 entries the same."""
    for kind, side in (("at_64", "right"), ("at_65", "none"), ("long", "none")):
        case = tc.boundary_case(kind)
        n, bt, tt = case["n"], case["wide"], case["thin"]
        assert tc.per_column(tt, n).max() == case["most"]
        B, T = nt.Matrix_ps.from_triplets(n, *bt), nt.Matrix_ps.from_triplets(n, *tt)
        res = session_product(nt, B, T, n, case["alpha"], case["thr"])
        assert_taken(res, side, "B T, thin columns of at most %d entries" % case["most"])
        assert_bits(res[0], oracle_product(fma, n, bt, tt, case["alpha"], case["thr"]), "B T " + kind)
        # on the left the same operand is the left kernel's whatever its columns hold (it walks rows of T)
        res = session_product(nt, T, B, n, case["alpha"], case["thr"])
        assert_taken(res, "left", "T B " + kind)
        assert_bits(res[0], oracle_product(fma, n, tt, bt, case["alpha"], case["thr"]), "T B " + kind)


def test_ties_of_the_thin_rule(nt, fma):
    """kernels.hpp slab_thin_rule at n = 256: nnz A == 8 n goes left, 8 n + 1 does not; both thin with nnz B == nnz A goes left,
    nnz B == nnz A - 1 right; nnz B == 8 n under a wide A goes right, 8 n + 1 to neither -- the counter that moved says so, and
    the bits are the oracle's every time"""
    n, cases = tc.rule_tie_cases()
    for name, At, Bt, side in cases:
        assert side == tc.thin_rule(len(At[2]), len(Bt[2]), n)
        A, B = nt.Matrix_ps.from_triplets(n, *At), nt.Matrix_ps.from_triplets(n, *Bt)
        res = session_product(nt, A, B, n, 1.0, 1e-8)
        assert_taken(res, side, "%s (nnz A %d, nnz B %d, 8 n %d)" % (name, len(At[2]), len(Bt[2]), 8 * n))
        assert_bits(res[0], oracle_product(fma, n, At, Bt, 1.0, 1e-8), name)


@pytest.mark.parametrize("alpha", tc.DENSE_ALPHAS)
def test_dense_rule_inside_a_session(nt, fma, alpha):
    """n = 48, min(nnz) > 0.1 n^2: the reference's dense branch thresholds the unscaled sum (DenseBranch.f90) -- the
    `dense_rule` arm of k_thin_slab_left and k_thin_slab_right, which no operand of 1003 rows or more can reach.  At least 100
    entries fare differently under the sparse rule for either alpha (tests/test_thin_cases_cpu.py), so a kernel that takes the
    wrong arm cannot pass."""
    case = tc.dense_rule_case()
    n, tt, bt, thr = case["n"], case["thin"], case["wide"], case["thr"]
    T, B = nt.Matrix_ps.from_triplets(n, *tt), nt.Matrix_ps.from_triplets(n, *bt)
    for (X, Y, Xt, Yt, side) in ((T, B, tt, bt, "left"), (B, T, bt, tt, "right")):
        what = "dense rule, thin %s, alpha %g" % (side, alpha)
        res = session_product(nt, X, Y, n, alpha, thr)
        assert_taken(res, side, what)
        assert_bits(res[0], oracle_product(fma, n, Xt, Yt, alpha, thr), what)


def test_gaps_inside_a_result_column(nt, fma):
    """thin_store: a 64-row chunk without a kept entry between two written chunks is zero-filled, the chunks before the first and
    after the last kept entry are never written.  Every column of the wide operand holds two clusters 200 rows apart; in at
    least 100 result columns two kept entries lie 129 or more rows apart (tests/test_thin_cases_cpu.py), inside windows of more
    than 192 rows.  The result is read back through its extents, so a chunk left unwritten shows as entries the oracle does not
    have.  The pool memory the result is written to is dirtied first by a product of the same shape with other values."""
    case = tc.gap_case()
    n, tt, bt, alpha, thr = case["n"], case["thin"], case["wide"], case["alpha"], case["thr"]
    T, B = nt.Matrix_ps.from_triplets(n, *tt), nt.Matrix_ps.from_triplets(n, *bt)
    dense = nt.Matrix_ps.from_triplets(n, *tc.wide_operand(n, 210))     # (a band that covers both clusters and the gap)
    for (X, Y, Xt, Yt, side) in ((T, B, tt, bt, "left"), (B, T, bt, tt, "right")):
        D = session_product(nt, *((T, dense) if side == "left" else (dense, T)), n, 1.0, 0.0)
        assert_taken(D, side, "gaps, the product that dirties the pool, thin " + side)
        del D
        res = session_product(nt, X, Y, n, alpha, thr)
        assert_taken(res, side, "gaps, thin " + side)
        assert_bits(res[0], oracle_product(fma, n, Xt, Yt, alpha, thr), "gaps, thin " + side)


def test_columns_whose_entries_are_all_pruned(nt, fma):
    """some columns of the wide operand are scaled by 1e-12 with a threshold of 1e-9: their result columns are computed and
    pruned whole -- thin_finish(..., 0, INT_MAX, -1) behind a live column, whole column groups of the left kernel among them.
    Empty in the oracle, empty here; and the extents (INT_MAX, -1) are consumable: C2 = C B (tile kernel, C on the left) and
    C3 = C T, C4 = T C (gather kernels) follow in the same session and are the oracle's bit for bit."""
    case = tc.pruned_case()
    n, tt, bt, alpha, thr = case["n"], case["thin"], case["wide"], case["alpha"], case["thr"]
    T, B = nt.Matrix_ps.from_triplets(n, *tt), nt.Matrix_ps.from_triplets(n, *bt)
    for (X, Y, Xt, Yt, side, dead) in ((T, B, tt, bt, "left", case["dead_left"]), (B, T, bt, tt, "right", case["dead_right"])):
        want = oracle_product(fma, n, Xt, Yt, alpha, thr)
        assert np.all(tc.per_column(want, n)[dead] == 0)
        C, C2, C3, C4 = (nt.Matrix_ps(n) for _ in range(4))
        c0, r0 = nt.thin_slab_counts(), nt.slab_algebra_counts()["refusals"]
        with nt.solver_session(False):
            C.Gemm(X, Y, None, alpha, 0.0, thr)
            c1 = nt.thin_slab_counts()
            C2.Gemm(C, B, None, 1.0, 0.0, thr)
            c2 = nt.thin_slab_counts()
            C3.Gemm(C, T, None, 1.0, 0.0, thr)
            c3 = nt.thin_slab_counts()
            C4.Gemm(T, C, None, 1.0, 0.0, thr)
            c4 = nt.thin_slab_counts()
        d = [delta(b, a) for a, b in ((c0, c1), (c1, c2), (c2, c3), (c3, c4))]
        print("pruned columns, thin", side, "counters", d)
        assert nt.slab_algebra_counts()["refusals"] == r0
        assert d[0]["real_" + side] == 1 and sum(d[0].values()) == 1, d[0]
        assert sum(d[1].values()) == 0, d[1]
        assert d[2]["real_right"] == 1 and sum(d[2].values()) == 1, d[2]
        assert d[3]["real_left"] == 1 and sum(d[3].values()) == 1, d[3]
        got = srt(C.triplets())
        assert_bits(got, want, "pruned columns, thin " + side)
        assert np.all(tc.per_column(got, n)[dead] == 0)
        assert_bits(srt(C2.triplets()), oracle_product(fma, n, want, bt, 1.0, thr), "C B behind it")
        assert_bits(srt(C3.triplets()), oracle_product(fma, n, want, tt, 1.0, thr), "C T behind it")
        assert_bits(srt(C4.triplets()), oracle_product(fma, n, tt, want, 1.0, thr), "T C behind it")


def test_unfused_arithmetic_takes_no_gather_kernel(nt):
    """spgemm_fma = 0: the session multiplies on the register-slab kernel (kernels.hip slab_multiply_loop); the gather kernels
    are FMA arithmetic only -- no thin counter moves, and the bits are the oracle's unfused product"""
    from oracle import oracle_py as O
    n, h = tc.BASE_SHAPES[0]
    alpha, thr = tc.BASE_SCALARS[0]
    case = tc.base_case(n, h)
    bt, tt = case["wide"], case["thin"]
    nt.set_option("spgemm_fma", 0)
    O.set_fma(False)
    B, T = nt.Matrix_ps.from_triplets(n, *bt), nt.Matrix_ps.from_triplets(n, *tt)
    for (X, Y, Xt, Yt, side) in ((T, B, tt, bt, "left"), (B, T, bt, tt, "right")):
        res = session_product(nt, X, Y, n, alpha, thr)
        print("unfused, thin", side, "-> thin", res[1], "slab", res[2], "counters", res[3], "refusals", res[4])
        assert sum(res[3].values()) == 0, res[3]
        assert res[2] == 1 and res[4] == 0, res[1:]
        assert_bits(res[0], oracle_product(O, n, Xt, Yt, alpha, thr), "unfused, thin " + side)
