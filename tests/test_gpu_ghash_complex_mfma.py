"""GPU: complex products of the grouped LDS-hash kernel on the FP64 matrix cores (ntpoly_amd/csrc/spgemm_grouped.hip,
k_spgemm_ghash<double2, 8, 1, 2, MF>; option ghash_mfma_complex, table class 0) against the oracle's complex multiply
(MultiplyBlock.f90:9-36, PruneList.f90:8-38).

The kernel is a TOLERANCE mode (every part of an entry is the sum of two FMA chains over ascending k): it is compared by the
`close` rule of tests/test_gpu_complex_tile.py with that file's numbers -- entries within 1e-13 of the largest entry, the pattern
identical except where |C(i, j)| lies within that distance of the threshold.  Option 0 in the same arithmetic mode is the
reference's complex multiply-add on the vector units, bit for bit: both are run, and the per-path group counters say which
kernel finished the groups, so a silently unchanged kernel choice cannot pass.

Every product here is made with the grouped path's memory dropped (the table class a product starts in then does not depend on
the tests before it), the block path off and the grouped kernel forced."""
import functools

import numpy as np
import pytest

from gen import permuted_banded_triplets

pytestmark = pytest.mark.gpu
REL = 1e-13
OPTION = "ghash_mfma_complex"
SEED = 42
PF_WPC_WAVE = 3 * 2 * 64   # entries of a column of A the two waves that share it request a phase ahead (PF x WPC x 64)


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
    yield
    nt.set_option("complex_tile", 1)
    nt.set_option("spgemm_fma", 0)


def srt(t):
    c, r, v = (np.asarray(x) for x in t)
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def close(got, want, n, thr, what):
    """(the rule and the numbers of tests/test_gpu_complex_tile.py)"""
    import scipy.sparse as sp
    G = sp.csr_matrix((got[2], (got[1] - 1, got[0] - 1)), shape=(n, n))
    W = sp.csr_matrix((want[2], (want[1] - 1, want[0] - 1)), shape=(n, n))
    scale = max(1.0, np.abs(want[2]).max())
    D = (G - W).tocoo()
    bad = np.abs(D.data) > REL * scale
    # entries present on one side only must sit at the threshold
    assert np.all(np.abs(D.data[bad]) <= thr * (1 + 1e-9) + REL * scale), "%s: max |d| = %g" % (what, np.abs(D.data).max())
    assert abs(G.nnz - W.nnz) <= max(8, 1e-5 * W.nnz), "%s: %d vs %d entries" % (what, G.nnz, W.nnz)


def exact(got, want, what):
    assert len(got[2]) == len(want[2]), "%s: %d vs %d entries" % (what, len(got[2]), len(want[2]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what + ": pattern differs"
    assert np.array_equal(got[2], want[2]), "%s: values differ, max |d| = %g" % (what, np.abs(got[2] - want[2]).max())


@functools.lru_cache(maxsize=None)
def operand(n, h, holes, which):
    """permuted banded complex triplets under the seed-42 relabelling; `which` = 0 / 1: the left / right operand of a pair"""
    col, row, val = permuted_banded_triplets(n, h, SEED, shift=0.1 * which, complex_=True)
    if holes:
        keep = (np.random.default_rng(n + h + which).random(len(val)) >= holes) | (col == row)
        col, row, val = col[keep], row[keep], val[keep]
    for a in (col, row, val):
        a.setflags(write=False)
    return col, row, val


@functools.lru_cache(maxsize=None)
def oracle_product(n, ha, hb, holes, thr, alpha):
    """the oracle's complex product of a case, computed once and shared"""
    from oracle import oracle_py as O
    Ao = O.Mat.from_triplets(n, n, *operand(n, ha, holes, 0))
    Bo = Ao if hb is None else O.Mat.from_triplets(n, n, *operand(n, hb, holes, 1))
    want = srt(O.ps_multiply(Ao, Bo, None, alpha, 0.0, thr).triplets())
    for a in want:
        a.setflags(write=False)
    return want


def grouped_gemm(nt, C, A, B, alpha, beta, thr, opt):
    """C = alpha A B + beta C on the forced grouped kernel with option `opt`; returns (statistics of the product, of the grouped
    path, groups finished per path)"""
    nt.drop_grouped_caches()
    nt.set_option("block_path", 0)
    nt.set_option("spgemm_variant", 500)     # (the grouped kernel, forced)
    nt.set_option(OPTION, opt)
    try:
        c0 = nt.ghash_class_counts()
        C.Gemm(A, B, None, alpha, beta, thr)
        st, gs, c1 = nt.last_spgemm_stats(), nt.last_grouped_stats(), nt.ghash_class_counts()
    finally:
        nt.set_option(OPTION, 1)
        nt.set_option("spgemm_variant", -1)
        nt.set_option("block_path", 1)
    assert st["slab"] == 0 and gs["used"] == 1, (st, gs)
    return st, gs, {k: c1[k] - c0[k] for k in c0}


# h_A of the third case: a column of A (2 h_A + 1 entries) longer than what its two waves request ahead, the row union of a
# product group (2 (h_A + h_B) + 1 rows and up to 7 more for the 8 columns) within 409
LONG = 196
assert 2 * LONG + 1 > PF_WPC_WAVE and 2 * (LONG + 2) + 8 <= 409

CASES = [(4096, 50, None, 0.0, 1e-8, 1.0),     # row unions of ~210: every group in class 0
         (3001, 37, 41, 0.3, 0.0, -0.5),       # a group with absent columns, unions that are no multiples of four, threshold 0
         (4096, LONG, 2, 0.0, 1e-8, 0.5),      # the rest of a long column is scattered by the loop behind the requested chunks
         (4097, 160, None, 0.0, 1e-6, 1.0)]    # unions of ~650 rows overflow class 0 and finish on the vector class 1


@pytest.mark.parametrize("n,ha,hb,holes,thr,alpha", CASES)
def test_complex_grouped_hash_on_the_matrix_cores_vs_oracle(nt, fma, n, ha, hb, holes, thr, alpha):
    A = nt.Matrix_ps.from_triplets(n, *operand(n, ha, holes, 0))
    B = A if hb is None else nt.Matrix_ps.from_triplets(n, *operand(n, hb, holes, 1))
    want = oracle_product(n, ha, hb, holes, thr, alpha)
    what = "complex grouped hash n=%d h=%d/%s" % (n, ha, hb)
    res = {}
    for opt in (1, 0):
        C = nt.Matrix_ps(n)
        st, gs, d = grouped_gemm(nt, C, A, B, alpha, 0.0, thr, opt)
        res[opt] = (srt(C.triplets()), gs, d)
        print(what, "option", opt, "grouped", gs, "groups per path", d)
    got1, gs1, d1 = res[1]
    got0, gs0, d0 = res[0]
    # option 0: the reference's complex multiply-add on the vector units, no group on the matrix cores
    assert d0["complex_mfma"] == 0 and d0["complex_vector"] > 0 and d0["real_mfma"] == 0 and d0["real_vector"] == 0, d0
    exact(got0, want, what + ", vector units")
    # option 1: class 0 on the matrix cores
    assert d1["complex_mfma"] > 0 and d1["real_mfma"] == 0 and d1["real_vector"] == 0, d1
    close(got1, want, n, thr, what + ", matrix cores")
    if min(ha, hb or ha) >= 30 and len(got1[2]) == len(got0[2]):
        assert not np.array_equal(got1[2], got0[2]), "the two kernels returned identical bits: was the matrix-core kernel taken?"
    if 2 * (ha + (hb or ha)) + 8 <= 512:   # (the rows of every group of product columns fit 512 slots)
        assert gs1["level"] == 0 and gs1["failed_cols"] == 0, gs1
        assert d1["complex_mfma"] == gs1["groups"] and d1["complex_vector"] == 0, (d1, gs1)
    else:                   # the groups that outgrow class 0 finish on the vector class 1
        assert gs1["level"] >= 1 and d1["complex_vector"] > 0, (gs1, d1)
        assert gs1["failed_cols"] <= gs0["failed_cols"] + n // 50, (gs1, gs0)


def test_zero_imaginary_parts_give_the_real_fma_product_bit_for_bit(nt, fma):
    """The first operand with its imaginary parts set to zero, stored as complex: the real plane's chain is then the chain of
    fma() of the real product, the imaginary plane adds exact zeros -- the real parts are the oracle's FMA-mode product of the
    real matrix bit for bit, every imaginary part is zero, the pattern is equal.  This pins the operand and accumulator layout of
    the two matrix instructions exactly, not to a tolerance."""
    from oracle import oracle_py as O
    n, h, thr = 4096, 50, 1e-8
    col, row, val = operand(n, h, 0.0, 0)
    A = nt.Matrix_ps.from_triplets(n, col, row, val.real + 0j)
    assert A.IsComplex()
    C = nt.Matrix_ps(n)
    st, gs, d = grouped_gemm(nt, C, A, A, 1.0, 0.0, thr, 1)
    assert d["complex_mfma"] == gs["groups"] and d["complex_vector"] == 0, (d, gs)
    got = srt(C.triplets())
    O.set_fma(True)
    try:
        Ao = O.Mat.from_triplets(n, n, col, row, np.ascontiguousarray(val.real))
        want = srt(O.ps_multiply(Ao, Ao, None, 1.0, 0.0, thr).triplets())
    finally:
        O.set_fma(False)
    assert np.all(got[2].imag == 0.0)
    exact((got[0], got[1], got[2].real), want, "zero imaginary parts against the real FMA product")


@pytest.mark.parametrize("mode", ["unfused", "complex_tile=0"])
def test_option_is_ignored_where_complex_products_are_bit_for_bit(nt, mode):
    """Unfused arithmetic (the suite's baseline), and FMA arithmetic with complex_tile = 0: option 1 changes nothing -- the product
    is the oracle's bit for bit and no group runs on the matrix cores."""
    n, h, thr = 4096, 50, 1e-8
    A = nt.Matrix_ps.from_triplets(n, *operand(n, h, 0.0, 0))
    want = oracle_product(n, h, None, 0.0, thr, 1.0)
    if mode != "unfused":
        nt.set_option("spgemm_fma", 1)
        nt.set_option("complex_tile", 0)
    try:
        C = nt.Matrix_ps(n)
        st, gs, d = grouped_gemm(nt, C, A, A, 1.0, 0.0, thr, 1)
    finally:
        nt.set_option("complex_tile", 1)
        nt.set_option("spgemm_fma", 0)
    assert d["complex_mfma"] == 0 and d["complex_vector"] > 0, d
    exact(srt(C.triplets()), want, "option 1, " + mode)


def test_gemm_vocabulary_around_the_kernel(nt, fma):
    """A^2 = A A, then 0.25 A^2 A - 1.5 A (beta in play): the Gemm vocabulary around the kernel stays what it was."""
    from oracle import oracle_py as O
    n, h, thr = 4096, 30, 1e-9
    col, row, val = operand(n, h, 0.0, 0)
    A = nt.Matrix_ps.from_triplets(n, col, row, val)
    Ao = O.Mat.from_triplets(n, n, col, row, val)
    A2 = nt.Matrix_ps(n)
    st, gs, d = grouped_gemm(nt, A2, A, A, 1.0, 0.0, thr, 1)
    assert d["complex_mfma"] > 0, d
    A2o = O.ps_multiply(Ao, Ao, None, 1.0, 0.0, thr)
    close(srt(A2.triplets()), srt(A2o.triplets()), n, thr, "A^2")
    A3 = nt.Matrix_ps(A)
    st, gs, d = grouped_gemm(nt, A3, A2, A, 0.25, -1.5, thr, 1)
    assert d["complex_mfma"] > 0, d
    A3o = O.ps_multiply(A2o, Ao, Ao, 0.25, -1.5, thr)
    close(srt(A3.triplets()), srt(A3o.triplets()), n, thr, "0.25 A^2 A - 1.5 A")
