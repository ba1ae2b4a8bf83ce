"""GPU: the block path for COMPLEX operands without run structure (csrc/spgemm_block.hip k_bs_numeric_c): complex 16 x 16
tiles of the clustered index order on the FP64 matrix cores, two FMA chains per part of an entry (Re A against
[Re B | Im B], Im A against [-Im B | Re B]) added in the epilogue -- the scheme of the complex tile kernel.

Parity statement.
  (1) TOLERANCE, as for complex_tile: every entry within 1e-13 of the product's largest entry against the oracle's complex
      multiply, on the caller's labels and on the matrices relabelled by block_order(), mapped back; the patterns equal
      except entries whose modulus lies within that distance of the threshold.
  (2) BIT FOR BIT with the real block path: a complex operand whose imaginary parts are all zero gives the real block
      path's values, pattern and block order, with every imaginary part zero.
  (3) DETERMINISTIC: the same product twice gives the same bits.
"""
import numpy as np
import pytest

from gen import lattice_triplets, permuted_banded_triplets

pytestmark = pytest.mark.gpu
REL = 1e-13


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture()
def fma(nt):
    from oracle import oracle_py as O
    nt.set_option("spgemm_fma", 1)
    nt.set_option("complex_tile", 1)
    nt.set_option("block_complex", 1)
    nt.set_option("block_path", 2)      # (lattices up to 20^3 have row windows the automatic rule leaves to the LDS kernels)
    nt.set_option("slab_algebra", 0)
    nt.drop_block_caches()
    yield O
    nt.set_option("spgemm_fma", 0)
    nt.set_option("complex_tile", 1)
    nt.set_option("block_complex", 1)
    nt.set_option("block_path", 1)
    nt.set_option("slab_algebra", 1)


def hermitian(trip, phase=0.1):
    """a Hermitian complex operand with the pattern and |values| of a real symmetric one: H(r, c) = v exp(i phase (r - c))"""
    c, r, v = trip
    return c, r, v * np.exp(1j * phase * (r.astype(np.float64) - c.astype(np.float64)))


def srt(t):
    c, r, v = (np.asarray(x) for x in t)
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def close(got, want, n, thr, what):
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
    g, w = srt(got), srt(want)
    assert len(g[2]) == len(w[2]), "%s: %d vs %d entries" % (what, len(g[2]), len(w[2]))
    assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), what + ": pattern differs"
    assert np.array_equal(g[2], w[2]), what + ": values differ"


def relabel(trip, rank):
    c, r, v = trip
    return srt(((rank[c - 1] + 1).astype(np.int32), (rank[r - 1] + 1).astype(np.int32), v))


def operands(kind):
    if kind.startswith("lattice") and kind != "lattice_asym":
        L = int(kind[7:])
        ta = hermitian(lattice_triplets(L))
        return L ** 3, ta, ta
    if kind == "lattice_asym":           # A != B, patterns not symmetric, columns left empty
        L = 16
        c, r, v = hermitian(lattice_triplets(L))
        keep = ((r.astype(np.int64) * 7 + c.astype(np.int64) * 13) % 5 != 0) & (c % 97 != 0)
        ta = (c[keep], r[keep], v[keep] * (1.0 + 0.001 * (r[keep] % 11)))
        keep = ((r.astype(np.int64) * 3 + c.astype(np.int64) * 17) % 7 != 0) & (r % 89 != 0)
        tb = (c[keep], r[keep], v[keep] * (1.0 - 0.002j * (c[keep] % 5)))
        return L ** 3, ta, tb
    if kind == "permuted_band":
        n = 6000
        ta = permuted_banded_triplets(n, 40, 7, complex_=True)
        return n, ta, ta
    if kind == "mixed":                  # real A times complex B: promoted before the multiply
        L = 12
        c, r, v = lattice_triplets(L)
        return L ** 3, (c, r, v), hermitian((c, r, v * 0.5), phase=0.3)
    raise ValueError(kind)


def engine_product(nt, n, ta, tb, alpha, thr):
    A = nt.Matrix_ps.from_triplets(n, *ta)
    B = A if tb is ta else nt.Matrix_ps.from_triplets(n, *tb)
    C = nt.Matrix_ps(n)
    C.Gemm(A, B, None, alpha, 0.0, thr)
    return A, srt(C.triplets()), nt.last_block_stats()


CASES = [("lattice12", 0.0, -0.75), ("lattice16", 1e-8, 1.0), ("lattice20", 1e-6, 0.5), ("lattice16", 1e-6, 0.5),
         ("lattice_asym", 1e-9, 1.0), ("permuted_band", 1e-8, 1.0), ("mixed", 1e-8, 1.0)]


@pytest.mark.parametrize("kind,thr,alpha", CASES)
def test_complex_block_product_vs_oracle(nt, fma, kind, thr, alpha):
    O = fma
    n, ta, tb = operands(kind)
    A, got, bs = engine_product(nt, n, ta, tb, alpha, thr)
    assert bs["used"] == 1, (kind, bs)
    assert np.iscomplexobj(got[2])
    Ao = O.Mat.from_triplets(n, n, ta[0], ta[1], ta[2].astype(np.complex128))   # (the oracle multiplies like types)
    Bo = Ao if tb is ta else O.Mat.from_triplets(n, n, *tb)
    close(got, srt(O.ps_multiply(Ao, Bo, None, alpha, 0.0, thr).triplets()), n, thr, kind + " (caller's labels)")
    if kind in ("lattice12", "lattice_asym", "permuted_band"):
        # the oracle on the matrices relabelled by the engine's block order, mapped back
        pos = nt.block_order(A)
        assert pos is not None and len(np.unique(pos)) == n
        order = np.argsort(pos, kind="stable")
        rank = np.empty(n, dtype=np.int64)
        rank[order] = np.arange(n)
        Ar = O.Mat.from_triplets(n, n, *relabel(ta, rank))
        Br = Ar if tb is ta else O.Mat.from_triplets(n, n, *relabel(tb, rank))
        c, r, v = O.ps_multiply(Ar, Br, None, alpha, 0.0, thr).triplets()
        back = srt(((order[c - 1] + 1).astype(np.int32), (order[r - 1] + 1).astype(np.int32), v))
        close(got, back, n, thr, kind + " (engine order)")


@pytest.mark.parametrize("thr,alpha", [(1e-8, 1.0), (0.0, -0.75)])
def test_zero_imaginary_parts_give_the_real_block_path_bits(nt, fma, thr, alpha):
    """the Im A . B'' chains are exact zeros and the Re A . B' chain is the real kernel's: the same values, pattern and
    block order as the real block path (each product in a fresh cache: the order is made from the modulus of the complex
    operand, from |value| of the real one)"""
    L = 16
    n = L ** 3
    c, r, v = lattice_triplets(L)
    tc, tr = (c, r, v.astype(np.complex128)), (c, r, v)
    nt.drop_block_caches()
    Ac, gc, bsc = engine_product(nt, n, tc, tc, alpha, thr)
    pos_c = nt.block_order(Ac).copy()
    assert bsc["used"] == 1
    nt.drop_block_caches()
    Ar, gr, bsr = engine_product(nt, n, tr, tr, alpha, thr)
    pos_r = nt.block_order(Ar).copy()
    assert bsr["used"] == 1
    assert np.array_equal(pos_c, pos_r)
    assert bsc["tile_products"] == bsr["tile_products"] and bsc["candidates"] == bsr["candidates"]
    assert np.all(gc[2].imag == 0.0)
    exact((gc[0], gc[1], gc[2].real), gr, "zero-imaginary complex vs real block path")


def test_complex_block_product_is_deterministic(nt, fma):
    n, ta, tb = operands("lattice_asym")
    _, g1, b1 = engine_product(nt, n, ta, tb, 1.0, 1e-9)
    _, g2, b2 = engine_product(nt, n, ta, tb, 1.0, 1e-9)
    assert b1["used"] == 1 and b2["used"] == 1
    exact(g1, g2, "the same product twice")


@pytest.mark.parametrize("solver", ["sign", "inverse_square_root"])
def test_complex_solver_loop_on_the_block_path(nt, fma, solver):
    """SignFunction / InverseSquareRoot on a complex 16^3 lattice: every product of the loop on the block path; the
    iteration count of the oracle's loop, the result within 1e-10 of the scale"""
    import scipy.sparse as sp
    O = fma
    L, thr = 16, 1e-6
    n = L ** 3
    shift = 0.0 if solver == "sign" else 2.5
    col, row, val = hermitian(lattice_triplets(L, shift=shift))
    H = nt.Matrix_ps.from_triplets(n, col, row, val)
    p = nt.SolverParameters()
    p.SetThreshold(thr)
    p.SetConvergeDiff(1e-7)
    Out = nt.Matrix_ps(n)
    if solver == "sign":
        nt.SignSolvers.ComputeSign(H, Out, p)
    else:
        nt.SquareRootSolvers.InverseSquareRoot(H, Out, p)
    assert nt.last_block_stats()["used"] == 1
    it = nt.solver_trace()["iterations"]
    got = srt(Out.triplets())
    Ho = O.Mat.from_triplets(n, n, col, row, val)
    Oo, tro = O.matrix_function(solver, Ho, O.params(converge_diff=1e-7, threshold=thr))
    assert tro["iterations"] == it
    w = srt(Oo.triplets())
    G = sp.csr_matrix((got[2], (got[1] - 1, got[0] - 1)), shape=(n, n))
    W = sp.csr_matrix((w[2], (w[1] - 1, w[0] - 1)), shape=(n, n))
    assert abs(G - W).max() <= 1e-10 * max(1.0, abs(W).max())


def test_automatic_rule_takes_a_large_complex_lattice(nt, fma):
    """32^3 (row windows beyond the direct-mapped LDS kernels): the block path without block_path = 2; sampled columns
    against a host product"""
    import scipy.sparse as sp
    nt.set_option("block_path", 1)
    L, thr = 32, 1e-6
    n = L ** 3
    c, r, v = hermitian(lattice_triplets(L))
    ta = (c, r, v)
    A, got, bs = engine_product(nt, n, ta, ta, 1.0, thr)
    assert bs["used"] == 1, bs
    As = sp.csc_matrix((v, (r - 1, c - 1)), shape=(n, n))
    cols = np.random.default_rng(3).choice(n, 48, replace=False)
    W = (As @ As[:, cols]).tocsc()
    W.data[np.abs(W.data) <= thr] = 0
    W.eliminate_zeros()
    sel = np.isin(got[0] - 1, cols)
    G = sp.csc_matrix((got[2][sel], (got[1][sel] - 1, np.searchsorted(np.sort(cols), got[0][sel] - 1))), shape=(n, len(cols)))
    W = W[:, np.argsort(cols)]
    scale = max(1.0, np.abs(W.data).max())
    D = abs(G - W)
    assert D.max() <= thr * (1 + 1e-9) + REL * scale
    assert abs(G.nnz - W.nnz) <= max(8, 1e-5 * W.nnz)


@pytest.mark.parametrize("what", ["block_complex", "unfused", "complex_tile"])
def test_options_keep_complex_products_off_the_block_path(nt, fma, what):
    """block_complex = 0, unfused arithmetic and complex_tile = 0 keep their kernels: used == 0; the bit-for-bit modes
    (unfused, complex_tile = 0) give the oracle's bits, block_complex = 0 the FMA mode's tolerance"""
    O = fma
    n, ta, _ = operands("lattice12")
    if what == "block_complex":
        nt.set_option("block_complex", 0)
    elif what == "unfused":
        nt.set_option("spgemm_fma", 0)
    else:
        nt.set_option("complex_tile", 0)
    _, got, bs = engine_product(nt, n, ta, ta, 1.0, 1e-8)
    assert bs["used"] == 0, bs
    Ao = O.Mat.from_triplets(n, n, *ta)
    want = srt(O.ps_multiply(Ao, Ao, None, 1.0, 0.0, 1e-8).triplets())
    if what == "block_complex":
        close(got, want, n, 1e-8, what)
    else:
        exact(got, want, what)
