"""Products with a thin left operand (ntpoly_amd/csrc/spgemm_thin.hip: identities, near-diagonal factors of the square-root
loops) against the oracle's multiply (MultiplyBlock.f90:9-36, PruneList.f90:8-38): BIT-EXACT in both arithmetic modes, real
and complex -- the kernel accumulates every entry over ascending k with the reference's own multiply-add."""
import numpy as np
import pytest

from gen import banded_triplets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture(params=["unfused", "fma"])
def arith(nt, request):
    from oracle import oracle_py as O
    fma = request.param == "fma"
    nt.set_option("spgemm_fma", 1 if fma else 0)
    O.set_fma(fma)
    yield request.param
    O.set_fma(False)
    nt.set_option("spgemm_fma", 0)


def srt(t):
    c, r, v = (np.asarray(x) for x in t)
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def exact(got, want, what):
    g, w = srt(got), srt(want)
    assert len(g[2]) == len(w[2]), "%s: %d vs %d entries" % (what, len(g[2]), len(w[2]))
    assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), what + ": pattern differs"
    assert np.array_equal(g[2], w[2]), "%s: values differ, max |d| = %g" % (what, np.abs(g[2] - w[2]).max())


def thin_triplets(n, reach, extra, cplx, seed, drop_diag=0.0):
    """diagonal (some of it missing) + `extra` entries per hundred rows within `reach` of the diagonal; 1-based (col, row, val)"""
    rng = np.random.default_rng(seed)
    d = np.arange(n)
    keep = rng.random(n) >= drop_diag
    rows = [d[keep]]
    cols = [d[keep]]
    ne = int(n * extra / 100)
    r = rng.integers(0, n, ne)
    c = np.clip(r + rng.integers(-reach, reach + 1, ne), 0, n - 1)
    rows.append(r)
    cols.append(c)
    row = np.concatenate(rows)
    col = np.concatenate(cols)
    key = col.astype(np.int64) * n + row
    _, first = np.unique(key, return_index=True)
    row, col = row[first], col[first]
    val = 1.0 + 0.25 * rng.standard_normal(len(row))
    if cplx:
        val = val + 0.3j * rng.standard_normal(len(row))
    return (col + 1).astype(np.int32), (row + 1).astype(np.int32), val


@pytest.mark.parametrize("n,h,holes,reach,extra,cplx,thr,alpha", [
    (6000, 120, 0.0, 0, 0, False, 1e-8, 1.0),          # identity-like (diagonal only)
    (6000, 120, 0.1, 40, 30, False, 1e-7, -0.5),       # near-diagonal factor
    (5003, 200, 0.3, 300, 150, False, 0.0, 2.0),       # several entries per row, far reach, threshold 0
    (6000, 60, 0.0, 0, 0, True, 1e-8, 1.0),
    (6000, 100, 0.2, 50, 60, True, 1e-7, 0.75),
    (4099, 240, 0.05, 200, 200, True, 1e-9, 1.0),
])
def test_thin_left_vs_oracle(nt, arith, n, h, holes, reach, extra, cplx, thr, alpha):
    from oracle import oracle_py as O
    rng = np.random.default_rng(n + h)
    col, row, val = banded_triplets(n, h, complex_=cplx)
    keep = (rng.random(len(val)) >= holes)
    keep &= ~np.isin(col, [7, 8, 9, n - 3])          # a few empty columns of B
    Bt = (col[keep], row[keep], val[keep])
    At = thin_triplets(n, reach, extra, cplx, seed=n + reach, drop_diag=0.02)
    A = nt.Matrix_ps.from_triplets(n, *At)
    B = nt.Matrix_ps.from_triplets(n, *Bt)
    C = nt.Matrix_ps(n)
    C.Gemm(A, B, None, alpha, 0.0, thr)
    # (real operands: a diagonal is run-like -- runs of one row -- and the slab session of the call multiplies it in slab form;
    # under FMA arithmetic the tile kernel's sessions take near-diagonal operands as well)
    if cplx or reach > 0:
        assert nt.last_spgemm_thin() == 1
    Ao = O.Mat.from_triplets(n, n, *At)
    Bo = O.Mat.from_triplets(n, n, *Bt)
    want = O.ps_multiply(Ao, Bo, None, alpha, 0.0, thr).triplets()
    exact(C.triplets(), want, "thin A * B n=%d cplx=%d %s" % (n, cplx, arith))
    # the same product with the kernel switched off: the general kernels agree bit for bit as well
    nt.set_option("thin_left", 0)
    try:
        C0 = nt.Matrix_ps(n)
        C0.Gemm(A, B, None, alpha, 0.0, thr)
        assert nt.last_spgemm_thin() == 0
    finally:
        nt.set_option("thin_left", 1)
    exact(C0.triplets(), want, "general kernels, thin A * B")
    # the thin operand on the right (real operands under FMA arithmetic: the slab session's gather kernel, spgemm_thin.hip
    # k_thin_slab_right; otherwise the column-driven kernels, which walk few entries per column there)
    C1 = nt.Matrix_ps(n)
    C1.Gemm(B, A, None, alpha, 0.0, thr)
    exact(C1.triplets(), O.ps_multiply(Bo, Ao, None, alpha, 0.0, thr).triplets(), "B * thin A")
    # thin * thin
    C2 = nt.Matrix_ps(n)
    C2.Gemm(A, A, None, alpha, 0.0, thr)
    exact(C2.triplets(), O.ps_multiply(Ao, Ao, None, alpha, 0.0, thr).triplets(), "thin A * A")


def test_thin_left_declines_far_entries(nt):
    """a left operand with entries far from its diagonal (a permuted identity) is not this kernel's: the general kernels take it"""
    from oracle import oracle_py as O
    n, h = 5000, 50
    rng = np.random.default_rng(3)
    perm = rng.permutation(n)
    At = ((np.arange(n) + 1).astype(np.int32), (perm + 1).astype(np.int32), np.ones(n))
    col, row, val = banded_triplets(n, h)
    A = nt.Matrix_ps.from_triplets(n, *At)
    B = nt.Matrix_ps.from_triplets(n, col, row, val)
    C = nt.Matrix_ps(n)
    C.Gemm(A, B, None, 1.0, 0.0, 1e-9)
    assert nt.last_spgemm_thin() == 0
    want = O.ps_multiply(O.Mat.from_triplets(n, n, *At), O.Mat.from_triplets(n, n, col, row, val), None, 1.0, 0.0, 1e-9).triplets()
    exact(C.triplets(), want, "permutation * B")


@pytest.fixture()
def compressed_columns(nt):
    """slab_algebra = 0: the one-call session of the C ABI would try real operands in slab form first (its own gather kernels,
    tests/test_gpu_thin_real_sessions.py); without it a product goes straight to spgemm() on compressed columns"""
    nt.set_option("slab_algebra", 0)
    yield
    nt.set_option("slab_algebra", 1)


def product(nt, n, At, Bt, alpha, thr):
    A, B, C = nt.Matrix_ps.from_triplets(n, *At), nt.Matrix_ps.from_triplets(n, *Bt), nt.Matrix_ps(n)
    C.Gemm(A, B, None, alpha, 0.0, thr)
    return C.triplets(), nt.last_spgemm_thin()


def oracle_product(n, At, Bt, alpha, thr):
    from oracle import oracle_py as O
    return O.ps_multiply(O.Mat.from_triplets(n, n, *At), O.Mat.from_triplets(n, n, *Bt), None, alpha, 0.0, thr).triplets()


@pytest.mark.parametrize("cplx", [False, True])
def test_dense_rule_of_the_thin_left_kernel(nt, arith, cplx):
    """n = 48 with min(nnz) > 0.1 n^2: the reference's dense branch thresholds the UNSCALED sum (DenseBranch.f90), the
    `dense_rule & 1` arm of k_spgemm_thin -- operands of thousands of rows with at most 8 n entries can never reach it.  At least
    100 entries fare differently under |alpha sum| > threshold (tests/test_thin_cases_cpu.py).  On compressed columns
    (slab_algebra = 0) thin x band is the thin-left kernel's; as a drop-in caller runs it the product may go to the call's own
    slab session first -- last_spgemm_thin() is printed and pinned to what the paths' rules give, the bits are the oracle's
    either way."""
    import thin_cases as tc
    case = tc.dense_rule_case(cplx)
    n, tt, bt, thr = case["n"], case["thin"], case["wide"], case["thr"]
    for alpha in case["alphas"]:
        for slab_algebra in (1, 0):
            nt.set_option("slab_algebra", slab_algebra)
            try:
                for (Xt, Yt, what) in ((tt, bt, "thin x band"), (bt, tt, "band x thin")):
                    got, thin = product(nt, n, Xt, Yt, alpha, thr)
                    print("dense rule n=48 cplx=%d %s alpha=%g slab_algebra=%d %s: last_spgemm_thin() = %d" % (cplx, arith, alpha, slab_algebra, what, thin))
                    exact(got, oracle_product(n, Xt, Yt, alpha, thr), "dense rule %s cplx=%d %s alpha=%g" % (what, cplx, arith, alpha))
                    if slab_algebra == 0 or cplx:
                        # (compressed columns -- the call's session takes no complex operand in slab form either: the thin-left
                        # kernel takes a thin LEFT operand, the column-driven kernels the other product)
                        assert thin == (1 if Xt is tt else 0), (what, thin)
                    else:
                        # (real operands in the call's own session: FMA arithmetic, the gather kernels on either side; unfused
                        # arithmetic, the register-slab kernel)
                        assert thin == (1 if arith == "fma" else 0), (what, thin)
            finally:
                nt.set_option("slab_algebra", 1)


def with_column(Bt, n, col, first, last, cplx):
    """column `col` of B replaced by entries in every row first .. last (1-based)"""
    c, r, v = Bt
    k = c != col
    rows = np.arange(first, last + 1)
    vals = 0.01 * (1.0 + (rows % 7)) * ((1.0 + 0.5j) if cplx else 1.0)
    c, r, v = np.concatenate([c[k], np.full(len(rows), col)]), np.concatenate([r[k], rows]), np.concatenate([v[k], vals])
    o = np.lexsort((r, c))
    return c[o].astype(np.int32), r[o].astype(np.int32), v[o]


def with_entry(At, col, row, val):
    c, r, v = At
    assert not np.any((c == col) & (r == row))
    c, r, v = np.append(c, col), np.append(r, row), np.append(v, val)
    o = np.lexsort((r, c))
    return c[o].astype(np.int32), r[o].astype(np.int32), v[o]


@pytest.mark.parametrize("cplx", [False, True])
def test_thin_left_gates(nt, arith, compressed_columns, cplx):
    """the refusal gates of spgemm_thin_left, each beside a case comfortably inside it (n = 2200, compressed columns):
    the LDS window -- 4 columns of the widest row extent of B must fit 64 KB (real: a column over rows 1 .. 2100 is 67200 bytes,
    over 1000 rows 32000; complex: 1100 rows 70400, 500 rows 32000); up + dn > 2048 -- one entry of A 2100 rows from its diagonal
    (real: B has a column over 1100 rows, so that 2 wmax + 64 = 2264 does not decide; complex: that window would not fit, and
    either rule may be the one that declines); up + dn > 2 wmax + 64 -- A of reach 300 against B of half-width 50 (101 rows:
    266), reach 100 is inside.  A declined product runs on the general kernels: last_spgemm_thin() == 0; every result is the
    oracle's bit for bit.  (A window of exactly 65536 bytes is left alone.)"""
    n, h, alpha, thr = 2200, 50, 0.75, 1e-8
    Bt = banded_triplets(n, h, complex_=cplx)
    near = thin_triplets(n, 40, 30, cplx, seed=n + 1, drop_diag=0.02)
    one = (1.0 + 0.5j) if cplx else 1.0
    long_rows, ok_rows = (1100, 500) if cplx else (2100, 1000)
    cases = [
        ("window past 64 KB", near, with_column(Bt, n, 1000, 1, long_rows, cplx), 0),
        ("window inside 64 KB", near, with_column(Bt, n, 1000, 1, ok_rows, cplx), 1),
        ("an entry 2100 rows from the diagonal", with_entry(near, 50, 2150, 0.5 * one),
         Bt if cplx else with_column(Bt, n, 1000, 1, 1100, cplx), 0),
        ("an entry 150 rows from the diagonal", with_entry(near, 50, 200, 0.5 * one), Bt, 1),
        ("reach 300 against half-width 50", thin_triplets(n, 300, 150, cplx, seed=n + 2, drop_diag=0.02), Bt, 0),
        ("reach 100 against half-width 50", thin_triplets(n, 100, 150, cplx, seed=n + 3, drop_diag=0.02), Bt, 1),
    ]
    for what, At, Bx, taken in cases:
        assert len(At[2]) <= 8 * n and len(Bx[2]) >= len(At[2])
        got, thin = product(nt, n, At, Bx, alpha, thr)
        print("gate:", what, "cplx", cplx, arith, "-> last_spgemm_thin()", thin)
        assert thin == taken, (what, thin)
        exact(got, oracle_product(n, At, Bx, alpha, thr), "%s cplx=%d %s" % (what, cplx, arith))


def test_kept_transposes_are_released_with_the_operand_caches(nt):
    """the transposes the thin-left path keeps per left operand (two slots) are device memory held between calls:
    ntpoly_amd_release_cache() returns it with the other operand caches (the engine's in-use figure goes back)"""
    n = 4096
    At = thin_triplets(n, 2, 3, True, seed=5, drop_diag=0.0)
    col, row, val = banded_triplets(n, 40, complex_=True)
    nt.set_option("spgemm_fma", 0)
    nt.release_cache()
    A = nt.Matrix_ps.from_triplets(n, *At)
    B = nt.Matrix_ps.from_triplets(n, col, row, val)
    C = nt.Matrix_ps(n)
    nt.synchronize()
    before = nt.memory()[0]
    C.Gemm(A, B, None, 1.0, 0.0, 1e-9)
    assert nt.last_spgemm_thin() == 1
    del C
    nt.synchronize()
    held = nt.memory()[0]
    assert held > before, "the product left nothing behind: the kept transpose is gone, update this test"
    nt.release_cache()
    nt.synchronize()
    assert nt.memory()[0] <= before, (before, held, nt.memory()[0])
