"""GPU: the transpose of a slab form (option slab_transpose; csrc/slab_extra.hip k_tr_extents / k_tr_span / k_tr_values,
k_sa_conj) and PolarDecomposition in a slab session (solvers.cpp sign_core).

Transposition is data movement: the packed result of the slab pass equals the transpose on compressed columns in pattern and in
bits, with conjugation the conjugate transpose.  Real Polar with the option at 1 equals the option at 0 bit for bit (iterations,
convergence values, pattern and values of the unitary factor) -- the statement tests/test_gpu_slab_algebra.py makes for the sign
loop; complex Polar with the option at 2 agrees with 1 under the complex tile kernel's tolerance (close() of
tests/test_gpu_complex_tile.py) and to rtol 1e-8 in its convergence norms.

The operand: banded_triplets(n, max(hl, hu), shift=2.5) with the entries -hu <= row - col <= hl kept and those above the diagonal
halved -- not symmetric (|A - A^H| about 0.12), singular values in about [1.12, 3.62]; the loop's dense restatement converges in
7 iterations on it at (n, hl, hu) = (1037, 24, 9) and (777, 40, 3)."""
import numpy as np
import pytest

from gen import banded_triplets

pytestmark = pytest.mark.gpu
REL = 1e-13
OPTION = "slab_transpose"


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


def _arith(nt, mode):
    before = {k: nt.get_option(k) for k in ("spgemm_fma", "slab_algebra", OPTION)}
    nt.set_option("spgemm_fma", mode)
    nt.set_option("slab_algebra", 1)
    return before


def _restore(nt, before):
    for k, v in before.items():
        nt.set_option(k, v)


@pytest.fixture(params=[1, 0], ids=["fma", "unfused"])
def arith(nt, request):
    """both arithmetic modes: FMA (tile-kernel results, slots aligned to 32 rows) and unfused (runs packed back to back)"""
    before = _arith(nt, request.param)
    yield request.param
    _restore(nt, before)


@pytest.fixture()
def fma(nt):
    before = _arith(nt, 1)
    yield
    _restore(nt, before)


def srt(t):
    c, r, v = (np.asarray(x) for x in t)
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def same(a, b):
    """pattern and bits"""
    return len(a[2]) == len(b[2]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def swapped(t):
    """the triplets of the transpose: rows and columns swapped, sorted again"""
    return srt((t[1], t[0], t[2]))


def close(got, want, n, thr, what):
    """the rule of tests/test_gpu_complex_tile.py"""
    import scipy.sparse as sp
    G = sp.csr_matrix((got[2], (got[1] - 1, got[0] - 1)), shape=(n, n))
    W = sp.csr_matrix((want[2], (want[1] - 1, want[0] - 1)), shape=(n, n))
    scale = max(1.0, np.abs(want[2]).max())
    D = (G - W).tocoo()
    bad = np.abs(D.data) > REL * scale
    # entries present on one side only must sit at the threshold
    assert np.all(np.abs(D.data[bad]) <= thr * (1 + 1e-9) + REL * scale), "%s: max |d| = %g" % (what, np.abs(D.data).max())
    assert abs(G.nnz - W.nnz) <= max(8, 1e-5 * W.nnz), "%s: %d vs %d entries" % (what, G.nnz, W.nnz)


def operand(n, hl, hu, complex_=False, holes=0.0, emptied=(), seed=1):
    col, row, val = banded_triplets(n, max(hl, hu), shift=2.5, complex_=complex_)
    d = row.astype(np.int64) - col
    keep = (d >= -hu) & (d <= hl)
    val = np.where(d < 0, 0.5 * val, val)
    if holes:
        keep &= (np.random.default_rng(seed).random(len(val)) >= holes) | (d == 0)
    if len(emptied):
        e = np.asarray(emptied) + 1
        keep &= ~np.isin(col, e) & ~np.isin(row, e)
    return col[keep], row[keep], val[keep]


def to_sp(t, n):
    import scipy.sparse as sp
    return sp.csc_matrix((t[2], (t[1] - 1, t[0] - 1)), shape=(n, n))


def norm1(M):
    return float(abs(M).sum(axis=0).max()) if M.nnz else 0.0


KERNEL_CASES = {"band3001": (3001, 24, 9, 0.3, ()), "emptied3001": (3001, 24, 9, 0.3, (0, 1500, 3000)), "narrow777": (777, 3, 3, 0.0, ())}


def _product_and_transpose(nt, trip, n, option):
    """P = X X (in a session of the call's own: left in slab form), T = P^T through the C ABI; what test 2 reads from both"""
    nt.set_option(OPTION, option)
    X = nt.Matrix_ps.from_triplets(n, *trip)
    P, T, T2, G = nt.Matrix_ps(n), nt.Matrix_ps(n), nt.Matrix_ps(n), nt.Matrix_ps(n)
    P.Gemm(X, X, None, 1.0, 0.0, 1e-8)
    c0 = nt.slab_transpose_counts()
    T.Transpose(P)
    c1 = nt.slab_transpose_counts()
    T2.Transpose(T)
    G.Gemm(T, P, None, 1.0, 0.0, 1e-8)
    nrm = T.Norm()
    back = srt(T2.triplets())
    g = srt(G.triplets())
    t = srt(T.triplets())
    p = srt(P.triplets())
    T.Increment(P, 0.75, 0.0)
    return dict(P=p, T=t, back=back, G=g, norm=nrm, inc=srt(T.triplets()), d=c1["transposes"] - c0["transposes"],
                refused=c1["refused"] - c0["refused"])


@pytest.fixture(scope="module")
def cache():
    return {}


def _runs(nt, cache, case, mode):
    key = (case, mode)
    if key not in cache:
        n, hl, hu, holes, emptied = KERNEL_CASES[case]
        trip = operand(n, hl, hu, holes=holes, emptied=emptied)
        cache[key] = (_product_and_transpose(nt, trip, n, 1), _product_and_transpose(nt, trip, n, 0))
    return cache[key]


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_transpose_of_a_product_through_the_c_abi(nt, arith, cache, case):
    """the product of an earlier call, still in slab form, is transposed there: counted, and the packed result is the product's
    triplets with rows and columns swapped -- exactly, and exactly what the option at 0 gives"""
    on, off = _runs(nt, cache, case, arith)
    assert on["d"] == 1 and on["refused"] == 0, on["d"]
    assert off["d"] == 0
    assert same(on["P"], off["P"])
    assert same(on["T"], swapped(on["P"]))
    assert same(on["T"], off["T"])


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_transposed_slab_form_is_a_valid_operand(nt, arith, cache, case):
    """a product with it, its norm and a merge into it give the bits of the option at 0; its transpose is the product again"""
    on, off = _runs(nt, cache, case, arith)
    assert same(on["G"], off["G"])
    assert on["norm"] == off["norm"]
    assert same(on["inc"], off["inc"])
    assert same(on["back"], on["P"]) and same(off["back"], off["P"])


@pytest.mark.parametrize("n", [3001, 1037])
@pytest.mark.parametrize("conj", [False, True], ids=["transpose", "conjugate_transpose"])
def test_complex_transpose_through_the_diagnostic_entry(nt, fma, n, conj):
    trip = operand(n, 24, 9, complex_=True, holes=0.3)
    A = nt.Matrix_ps.from_triplets(n, *trip)
    AT, W = nt.Matrix_ps(n), nt.Matrix_ps(n)
    c0 = nt.slab_transpose_counts()
    assert nt.slab_transpose(A, AT, conjugate=conj) is True
    c1 = nt.slab_transpose_counts()
    assert c1["transposes"] - c0["transposes"] == 1
    nt.set_option(OPTION, 0)   # compressed columns
    W.Transpose(A)
    if conj:
        W.Conjugate()
    got, want = srt(AT.triplets()), srt(W.triplets())
    assert same(got, want)
    assert np.array_equal(np.signbit(got[2].imag), np.signbit(want[2].imag)) and np.array_equal(np.signbit(got[2].real), np.signbit(want[2].real))
    assert same(srt(A.triplets()), srt(trip))   # (the operand is what it was)


def _count_deltas(nt, fn):
    c0, s0 = nt.slab_transpose_counts(), nt.slab_algebra_counts()
    out = fn()
    c1, s1 = nt.slab_transpose_counts(), nt.slab_algebra_counts()
    return out, {k: c1[k] - c0[k] for k in c1}, s1["refusals"] - s0["refusals"]


def test_transpose_with_extents_far_apart_is_refused_not_overflowed(nt, arith):
    """a narrow band with full columns 0 and n - 1: the transpose has full rows, every column of it would span all n rows (about n^2
    slots against 4 slots + 4 row_pad n).  The product X X of this operand never reaches the vocabulary call in slab form --
    slab_multiply declines it (a window of 3008 rows for the blocks of the full columns), so P arrives in compressed columns and
    TransposeMatrix is gated, not refused -- hence the diagnostic entry: it enters P itself, the pass refuses (return value 0, counted,
    the result handle untouched), and the transpose through the C ABI equals the option at 0"""
    n, h = 3001, 3
    col, row, val = operand(n, h, h)
    rest = (col != 1) & (col != n)
    i = np.arange(1, n + 1, dtype=np.int32)
    full = 0.01 + 0.001 * np.cos(i.astype(np.float64))
    col = np.concatenate([col[rest], np.full(n, 1, np.int32), np.full(n, n, np.int32)])
    row = np.concatenate([row[rest], i, i])
    val = np.concatenate([val[rest], full, full])
    res = []
    for option in (1, 0):
        nt.set_option(OPTION, option)
        X = nt.Matrix_ps.from_triplets(n, col, row, val)
        P, T, D = nt.Matrix_ps(n), nt.Matrix_ps(n), nt.Matrix_ps(n)
        P.Gemm(X, X, None, 1.0, 0.0, 1e-8)
        _, dt, _ = _count_deltas(nt, lambda: T.Transpose(P))
        assert dt == dict(transposes=0, conjugates=0, refused=0, polar_sessions=0)   # (gated: P is in compressed columns)
        if option == 1:
            took, dd, _ = _count_deltas(nt, lambda: nt.slab_transpose(P, D))
            assert took is None and dd["refused"] == 1 and dd["transposes"] == 0
            assert D.GetSize() == 0   # (the result handle is as it was)
        res.append((srt(T.triplets()), srt(P.triplets())))
    on, off = res
    assert same(on[0], off[0]) and same(on[0], swapped(on[1]))


def test_refused_transpose_inside_a_session_runs_on_compressed_columns(nt, arith):
    """an operand whose product DOES stay in slab form while its transpose does not fit: columns below 1504 hold a narrow run around
    their diagonal, columns from 1504 on the same run 1504 rows higher -- every column is narrow (the split sits on a block
    boundary), but row i < 1497 holds entries near columns i and i + 1504, so a transposed column spans about 1510 rows: about 2.3e6
    slots against a bound of at most 1.2e6.  TransposeMatrix of the product is refused past the gates: counted there and in the
    session's books, P keeps its slab form, and the result is the transpose on compressed columns"""
    n, h, split = 3001, 3, 1504
    col, row, val = operand(n, h, h)
    row = np.where(col > split, row - split, row)
    keep = row >= 1
    trip = (col[keep], row[keep], val[keep])
    res = []
    for option in (1, 0):
        nt.set_option(OPTION, option)
        X = nt.Matrix_ps.from_triplets(n, *trip)
        P, T, Q = nt.Matrix_ps(n), nt.Matrix_ps(n), nt.Matrix_ps(n)
        P.Gemm(X, X, None, 1.0, 0.0, 1e-8)
        _, dt, ds = _count_deltas(nt, lambda: T.Transpose(P))
        _, _, _ = _count_deltas(nt, lambda: Q.Gemm(P, T, None, 1.0, 0.0, 1e-8))   # (P is still a valid operand)
        res.append((srt(T.triplets()), srt(P.triplets()), srt(Q.triplets()), dt, ds))
    on, off = res
    assert on[3] == dict(transposes=0, conjugates=0, refused=1, polar_sessions=0) and on[4] == 1, (on[3], on[4])
    assert off[3] == dict(transposes=0, conjugates=0, refused=0, polar_sessions=0) and off[4] == 0
    assert same(on[0], off[0]) and same(on[0], swapped(on[1])) and same(on[2], off[2])


def _polar(nt, A, n, thr, conv):
    p = nt.SolverParameters()
    p.SetThreshold(thr)
    p.SetConvergeDiff(conv)
    U, Hm = nt.Matrix_ps(n), nt.Matrix_ps(n)
    s0, c0 = nt.slab_algebra_counts(), nt.slab_transpose_counts()
    nt.SignSolvers.ComputePolarDecomposition(A, U, Hm, p)
    tr = nt.solver_trace()
    s1, c1 = nt.slab_algebra_counts(), nt.slab_transpose_counts()
    return dict(U=srt(U.triplets()), Hm=srt(Hm.triplets()), it=int(tr["iterations"]), value=np.asarray(tr["value"]),
                slab={k: s1[k] - s0[k] for k in s1}, tr={k: c1[k] - c0[k] for k in c1})


def test_real_polar_in_a_session_equals_compressed_columns(nt, arith):
    """option 1 against option 0 at n = 3001, (hl, hu) = (24, 9): iterations, convergence values, pattern and bits of U (and Hm), the
    session's counts, U^T U = I, U Hm = A.

    Measured on one MI355X: 12 iterations in both modes, every result bit for bit in both, 24 products and 11 transposes in slab form
    and no refusal in both.  In unfused arithmetic that needs the Polar session's rule (engine.hpp slab_keep_sparse_runs): from the
    seventh iteration on 3 I - a^2 U^T U is sparse inside wide extents, where ps_multiply would otherwise hand the product to the
    general kernels, book a refusal and pack U -- the next transpose would then start from compressed columns again (17 products,
    6 transposes and 5 refusals without the rule)."""
    n, thr = 3001, 1e-8
    trip = operand(n, 24, 9)
    A = nt.Matrix_ps.from_triplets(n, *trip)
    nt.set_option(OPTION, 0)
    off = _polar(nt, A, n, thr, 1e-8)
    nt.set_option(OPTION, 1)
    on = _polar(nt, A, n, thr, 1e-8)
    print("iterations", off["it"], on["it"], "slab", on["slab"], "transpose counts", on["tr"])
    assert off["tr"] == dict(transposes=0, conjugates=0, refused=0, polar_sessions=0) and off["slab"]["products"] == 0
    assert on["it"] == off["it"] and on["it"] >= 5
    assert np.array_equal(on["value"], off["value"])
    assert same(on["U"], off["U"]), "max |d| = %g" % (np.abs(on["U"][2] - off["U"][2]).max() if len(on["U"][2]) == len(off["U"][2]) else -1)
    assert same(on["Hm"], off["Hm"])
    assert on["tr"]["polar_sessions"] == 1
    if arith == 1:
        assert on["slab"]["refusals"] <= 1
    import scipy.sparse as sp
    U, Hm, Ad = to_sp(on["U"], n), to_sp(on["Hm"], n), to_sp(trip, n)
    assert norm1(U.T @ U - sp.identity(n, format="csc")) <= 1e-5
    assert abs(U @ Hm - Ad).max() <= 1e-6
    assert on["slab"]["products"] >= 2 * (on["it"] - 1), on["slab"]
    assert on["tr"]["transposes"] >= on["it"] - 1, on["tr"]


def test_complex_polar_in_a_complex_session(nt, fma):
    n, thr = 1037, 1e-8
    trip = operand(n, 24, 9, complex_=True)
    A = nt.Matrix_ps.from_triplets(n, *trip)
    nt.set_option(OPTION, 1)
    one = _polar(nt, A, n, thr, 1e-8)
    nt.set_option(OPTION, 2)
    two = _polar(nt, A, n, thr, 1e-8)
    print("iterations", one["it"], two["it"], "slab", two["slab"], "transpose counts", two["tr"])
    assert one["slab"]["products"] == 0 and one["tr"]["polar_sessions"] == 0   # (option 1: the complex loop on compressed columns, as ever)
    assert two["tr"]["polar_sessions"] == 1 and two["slab"]["products"] >= 2 * (two["it"] - 1)
    assert two["tr"]["transposes"] >= two["it"] - 1 and two["tr"]["conjugates"] >= two["it"] - 1
    assert two["it"] == one["it"] and two["it"] >= 5
    close(two["U"], one["U"], n, thr, "complex polar U")
    assert np.allclose(two["value"], one["value"], rtol=1e-8, atol=0.0)
    import scipy.sparse as sp
    U = to_sp(two["U"], n)
    assert norm1(U.conj().T @ U - sp.identity(n, format="csc")) <= 1e-5
