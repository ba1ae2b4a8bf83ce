"""GPU: complex iterates kept in block form (csrc/spgemm_block.hip, psmatrix.cpp complex_blocks_on).  Inside a session with
complex sessions and the complex block path allowed (one rank), complex products on the block path stay in block form
(DevMat::blk) and the loop's merges, scalings, copies, dots, traces and norms run on complex tiles (k_bs_merge<., true>,
k_bs_colabs_max<true>) instead of converting around every product.

Parity statement.
  (1) ELEMENT RULES BIT FOR BIT: Scale / Increment (complex, real and pruning) / Copy / the identity increment of a complex
      block-form matrix give the triplets the same calls give on a compressed-column copy of it (the complex merge on
      compressed columns: real scalars per part, the threshold on hypot(re, im)).  Dot, trace and norm to summation order.
  (2) SOLVER LOOPS: Sign, Invert, SquareRoot and InverseSquareRoot in block form take the iteration counts of the loops on
      compressed columns and of the oracle, their results within 1e-12 of each other and 1e-10 of the oracle.
  (3) DETERMINISTIC: the same loop twice gives the same bits.
"""
import numpy as np
import pytest

from gen import lattice_triplets, permuted_banded_triplets

pytestmark = pytest.mark.gpu
REL = 1e-13
L, THR = 16, 1e-6


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture()
def cs(nt):
    from oracle import oracle_py as O
    nt.set_option("spgemm_fma", 1)
    nt.set_option("complex_tile", 1)
    nt.set_option("block_complex", 1)
    nt.set_option("block_path", 2)      # (lattices up to 20^3 have row windows the automatic rule leaves to the LDS kernels)
    nt.set_option("slab_algebra", 1)
    nt.set_option("complex_sessions", 1)
    nt.drop_block_caches()
    yield O
    nt.set_option("spgemm_fma", 0)
    nt.set_option("complex_tile", 1)
    nt.set_option("block_complex", 1)
    nt.set_option("block_path", 1)
    nt.set_option("slab_algebra", 1)
    nt.set_option("complex_sessions", 1)


def hermitian(trip, phase=0.1):
    c, r, v = trip
    return c, r, v * np.exp(1j * phase * (r.astype(np.float64) - c.astype(np.float64)))


def srt(t):
    c, r, v = (np.asarray(x) for x in t)
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def exact(got, want, what):
    g, w = srt(got), srt(want)
    assert len(g[2]) == len(w[2]), "%s: %d vs %d entries" % (what, len(g[2]), len(w[2]))
    assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), what + ": pattern differs"
    assert np.array_equal(g[2], w[2]), what + ": values differ"


def csr(t, n):
    import scipy.sparse as sp
    return sp.csr_matrix((t[2], (t[1] - 1, t[0] - 1)), shape=(n, n))


def cdot(nt, A, B):
    """DotMatrix_psc_wrp straight (Matrix_ps.Dot asks IsComplex first, an entry point that packs its matrix)"""
    import ctypes as C
    re, im = C.c_double(), C.c_double()
    nt.lib.DotMatrix_psc_wrp(A.ih, B.ih, C.byref(re), C.byref(im))
    return complex(re.value, im.value)


def counts(nt):
    c = nt.block_algebra_counts()
    return c["operations"], c["fallbacks"]


def run_solver(nt, solver, H, n):
    p = nt.SolverParameters()
    p.SetThreshold(THR)
    p.SetConvergeDiff(1e-7)
    Out = nt.Matrix_ps(n)
    if solver == "sign":
        nt.SignSolvers.ComputeSign(H, Out, p)
    elif solver == "invert":
        nt.InverseSolvers.Invert(H, Out, p)
    elif solver == "square_root":
        nt.SquareRootSolvers.SquareRoot(H, Out, p)
    else:
        nt.SquareRootSolvers.InverseSquareRoot(H, Out, p)
    return srt(Out.triplets()), nt.solver_trace()["iterations"]


@pytest.mark.parametrize("solver", ["sign", "invert", "square_root", "inverse_square_root"])
def test_complex_solver_loops_in_block_form(nt, cs, solver):
    """with complex sessions on, the loop's vocabulary runs on complex tiles (at least two operations per iteration);
    with them off, none does; the two agree to roundoff (the products of the run off may take the LDS-hash kernels, whose
    chain runs over labels) and both take the oracle's iteration count"""
    O = cs
    n = L ** 3
    shift = 0.0 if solver == "sign" else 2.5
    col, row, val = hermitian(lattice_triplets(L, shift=shift))
    H = nt.Matrix_ps.from_triplets(n, col, row, val)
    res = {}
    for on in (0, 1):
        nt.set_option("complex_sessions", on)
        c0 = counts(nt)
        got, it = run_solver(nt, solver, H, n)
        c1 = counts(nt)
        res[on] = (got, it, c1[0] - c0[0])
    assert res[0][2] == 0, res[0][2]
    assert res[1][2] >= 2 * res[1][1], (res[1][2], res[1][1])
    assert res[0][1] == res[1][1]
    G, W = csr(res[1][0], n), csr(res[0][0], n)
    assert abs(G - W).max() <= 1e-12 * max(1.0, abs(W).max())
    Ho = O.Mat.from_triplets(n, n, col, row, val)
    Oo, tro = O.matrix_function(solver, Ho, O.params(converge_diff=1e-7, threshold=THR))
    assert tro["iterations"] == res[1][1]
    Wo = csr(srt(Oo.triplets()), n)
    for on in (0, 1):
        assert abs(csr(res[on][0], n) - Wo).max() <= 1e-10 * max(1.0, abs(Wo).max())


@pytest.mark.parametrize("kind", ["lattice", "permuted_band"])
def test_complex_products_stay_in_block_form_across_c_abi_calls(nt, cs, kind):
    """a caller's loop over MatrixMultiply_ps_wrp: the second product of the dimension stays in block form (a Scale on it is
    a block-algebra operation) and is multiplied as it is -- the same bits as the product of operands rebuilt from
    triplets, within 1e-13 of the oracle on the caller's labels"""
    O = cs
    if kind == "lattice":
        n = L ** 3
        ta = hermitian(lattice_triplets(L))
    else:
        n = 6000
        ta = permuted_banded_triplets(n, 40, 7, complex_=True)
    thr = 1e-7
    A = nt.Matrix_ps.from_triplets(n, *ta)
    C1 = nt.Matrix_ps(n)
    C1.Gemm(A, A, None, 1.0, 0.0, thr)
    assert nt.last_block_stats()["used"] == 1
    C2 = nt.Matrix_ps(n)
    C2.Gemm(A, A, None, 1.0, 0.0, thr)
    c0 = counts(nt)
    C2.Scale(1.0)
    c1 = counts(nt)
    assert c1[0] == c0[0] + 1 and c1[1] == c0[1], (c0, c1)
    C3 = nt.Matrix_ps(n)
    C3.Gemm(C2, A, None, 0.5, 0.0, thr)
    assert nt.last_block_stats()["used"] == 1
    got = srt(C3.triplets())
    assert np.iscomplexobj(got[2])
    nt.set_option("slab_algebra", 0)
    C2r = nt.Matrix_ps.from_triplets(n, *srt(C2.triplets()))
    Ar = nt.Matrix_ps.from_triplets(n, *ta)
    C3r = nt.Matrix_ps(n)
    C3r.Gemm(C2r, Ar, None, 0.5, 0.0, thr)
    assert nt.last_block_stats()["used"] == 1
    exact(got, C3r.triplets(), "block-form operand vs compressed columns")
    Ao = O.Mat.from_triplets(n, n, *ta)
    P2 = O.ps_multiply(Ao, Ao, None, 1.0, 0.0, thr)
    want = srt(O.ps_multiply(P2, Ao, None, 0.5, 0.0, thr).triplets())
    G, W = csr(got, n), csr(want, n)
    scale = max(1.0, np.abs(want[2]).max())
    D = (G - W).tocoo()
    bad = np.abs(D.data) > REL * scale
    assert np.all(np.abs(D.data[bad]) <= thr * (1 + 1e-9) + REL * scale), np.abs(D.data).max()
    assert abs(G.nnz - W.nnz) <= max(8, 1e-5 * W.nnz)


def test_complex_element_rules_bit_for_bit(nt, cs):
    """Scale, Increment (complex, real, pruning), the identity increment and Copy on a complex block-form matrix against the
    same calls on a compressed-column copy of it: identical triplets; dot, trace and norm to summation order"""
    n = L ** 3
    ta = hermitian(lattice_triplets(L))
    A = nt.Matrix_ps.from_triplets(n, *ta)

    def product():
        P = nt.Matrix_ps(n)
        P.Gemm(A, A, None, 1.0, 0.0, 1e-7)
        return P

    Q = nt.Matrix_ps.from_triplets(n, *srt(product().triplets()))
    P = product()
    Bc = nt.Matrix_ps.from_triplets(n, *hermitian(lattice_triplets(L, shift=0.5), phase=0.37))
    Br = nt.Matrix_ps.from_triplets(n, *lattice_triplets(L, shift=-1.0))
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    prune = float(np.median(np.abs(srt(product().triplets())[2])))
    P = product()
    c0 = counts(nt)
    steps = [("Scale", -0.75), ("Increment", Bc, 0.3, 0.0), ("Increment", Br, -1.25, 0.0), ("Increment", Bc, 1.0, prune),
             ("Increment", I, -1.0, 0.0)]
    for st in steps:
        if st[-1] == prune:
            tq, tb = srt(Q.triplets()), srt(Bc.triplets())
            union = len(set(zip(tq[0].tolist(), tq[1].tolist())) | set(zip(tb[0].tolist(), tb[1].tolist())))
        for M in (P, Q):
            getattr(M, st[0])(*st[1:])
        if st[-1] == prune:
            assert len(srt(Q.triplets())[2]) < union   # (the threshold dropped entries)
    c1 = counts(nt)
    assert c1[0] - c0[0] == len(steps) and c1[1] == c0[1], (c0, c1)
    # (reductions: the block form sums over its super-tiles, compressed columns over columns)
    for got, want in [(cdot(nt, P, Bc), cdot(nt, Q, Bc)), (cdot(nt, Bc, P), cdot(nt, Bc, Q)), (P.Trace(), Q.Trace()), (P.Norm(), Q.Norm())]:
        assert abs(got - want) <= REL * max(1.0, abs(want)), (got, want)
    c2 = counts(nt)
    assert c2[0] - c1[0] == 4 and c2[1] == c1[1], (c1, c2)
    P2 = nt.Matrix_ps(n)
    nt.lib.CopyMatrix_ps_wrp(P.ih, P2.ih)      # CopyMatrix of a block-form matrix
    assert counts(nt)[0] == c2[0] + 1
    want = srt(Q.triplets())
    exact(P.triplets(), want, "Scale / Increment / identity increment")
    exact(P2.triplets(), want, "Copy")


def test_complex_block_loop_is_deterministic(nt, cs):
    n = L ** 3
    H = nt.Matrix_ps.from_triplets(n, *hermitian(lattice_triplets(L, shift=2.5)))
    g1, i1 = run_solver(nt, "inverse_square_root", H, n)
    nt.drop_block_caches()
    g2, i2 = run_solver(nt, "inverse_square_root", H, n)
    assert i1 == i2
    exact(g1, g2, "the same loop twice")


@pytest.mark.parametrize("what", ["block_complex", "slab_algebra", "complex_sessions"])
def test_switches_keep_complex_loops_off_block_form(nt, cs, what):
    n = L ** 3
    H = nt.Matrix_ps.from_triplets(n, *hermitian(lattice_triplets(L)))
    nt.set_option(what, 0)
    c0 = counts(nt)
    _, it = run_solver(nt, "sign", H, n)
    c1 = counts(nt)
    assert it > 0 and c1 == c0, (c0, c1)
