"""GPU, one rank: the engine's four operand caches against operands that change IN PLACE between two calls.

Between calls the engine keeps a derivative of an operand: the transposes of the thin-left path (spgemm_thin.hip, two slots), the
block forms of the block path (spgemm_block.hip operand_form), the expanded D of the fused TRS2 step (kernels.hip dot_operand)
and the relabelled D (relabel_key_matches).  All are keyed on (value pointer, allocation serial, value epoch, nnz); every function
that rewrites values in place must bump the epoch.  One that forgets returns the PREVIOUS operand's product -- finite and
plausible.  Every case here: a call that fills the cache, the operand changed in place through the vocabulary (ScaleMatrix,
ConjugateMatrix, MatrixDiagonalScale, IncrementMatrix(Identity) on a stored diagonal, a matrix deleted and rebuilt with the same
pattern), the same call again, and the second result compared with the reference computed from the CHANGED operand -- and shown to
differ from the first, so that no case is vacuous.  Products: the oracle, bit for bit.  Energies of trs2_step: a dense numpy
evaluation, relative 1e-11 (README, "energies 1e-11"); a stale cache is wrong by a factor of 3 there."""
import time

import numpy as np
import pytest

import thin_cases as tc
from gen import banded_triplets, lattice_triplets, permuted_banded_triplets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    t0 = time.perf_counter()
    yield nt
    print("\n[wall time] tests/test_gpu_operand_caches.py: %.1f s" % (time.perf_counter() - t0))


@pytest.fixture()
def clean(nt):
    """every case starts from and leaves empty caches and the options it found"""
    from oracle import oracle_py as O
    nt.release_cache()
    yield O
    nt.release_cache()
    O.set_fma(False)
    nt.set_option("spgemm_fma", 0)
    nt.set_option("slab_algebra", 1)
    nt.set_option("block_path", 1)


def srt(t):
    c, r, v = (np.asarray(x) for x in t)
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def exact(got, want, what):
    g, w = srt(got), srt(want)
    assert len(g[2]) == len(w[2]), "%s: %d vs %d entries" % (what, len(g[2]), len(w[2]))
    assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), what + ": pattern differs"
    assert np.array_equal(g[2], w[2]), "%s: values differ, max |d| = %g" % (what, np.abs(g[2] - w[2]).max())


def differs(a, b):
    a, b = srt(a), srt(b)
    return len(a[2]) != len(b[2]) or not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]))


# ------------------------------------------------------------------ the mutators: (matrix, its triplets) -> (matrix, its triplets now)
def m_scale(nt, A, t, n):
    A.Scale(-2.5)
    return A, (t[0], t[1], t[2] * -2.5)


def m_conjugate(nt, A, t, n):
    A.Conjugate()
    return A, (t[0], t[1], np.conj(t[2]))


def m_diagonal_scale(nt, A, t, n):
    """column c times the factor of its triplet (real factors, also for complex matrices: exact in either arithmetic)"""
    cplx = np.iscomplexobj(t[2])
    cols = np.arange(1, n + 1, 3, dtype=np.int32)
    f = 1.5 + (cols % 5)
    tl = nt.TripletList_c() if cplx else nt.TripletList_r()
    tl.set_arrays(cols, cols, f.astype(np.complex128) if cplx else f)
    getattr(nt.lib, "MatrixDiagonalScale_ps%s_wrp" % ("c" if cplx else "r"))(A.ih, tl.ih)
    factor = np.ones(n + 1)
    factor[cols] = f
    return A, (t[0], t[1], t[2] * factor[t[0]])


def m_increment_identity(nt, A, t, n):
    """IncrementMatrix(Identity, A, 0.75) as the solver loops call it; A stores its whole diagonal, so on compressed columns one
    value per column changes in place (column_fused.hip add_identity_inplace)"""
    assert (t[0] == t[1]).sum() == n
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    nt.increment_identity(I, A, 0.75)
    return A, (t[0], t[1], np.where(t[0] == t[1], 0.75 + t[2], t[2]))


def m_rebuild(nt, A, t, n):
    """the matrix deleted, another one built with the same pattern and other values (the allocator may hand out the same buffer)"""
    A.__del__()   # (DestructMatrix now, not when the caller's name goes away)
    v = t[2] * (1.0 + 0.25 * np.cos(t[0] + 2.0 * t[1]))
    return nt.Matrix_ps.from_triplets(n, t[0], t[1], v), (t[0], t[1], v)


MUTATORS = [m_scale, m_conjugate, m_diagonal_scale, m_increment_identity, m_rebuild]


def mutators_for(cplx):
    return [m for m in MUTATORS if cplx or m is not m_conjugate]


def oracle_product(O, n, At, Bt, alpha, thr):
    return O.ps_multiply(O.Mat.from_triplets(n, n, *At), O.Mat.from_triplets(n, n, *Bt), None, alpha, 0.0, thr).triplets()


def gemm(nt, A, B, n, alpha, thr):
    C = nt.Matrix_ps(n)
    C.Gemm(A, B, None, alpha, 0.0, thr)
    return C.triplets(), nt.last_spgemm_thin()


# ------------------------------------------------------------------ kept transposes of the thin-left path
@pytest.mark.parametrize("kind", ["real_unfused", "real_fma", "complex"])
@pytest.mark.parametrize("slab_algebra", [0, 1])
def test_kept_transpose_of_an_operand_changed_in_place(nt, clean, kind, slab_algebra):
    """thin A x wide B outside a session, n = 1003, twice with A changed in between.  slab_algebra = 0: compressed columns, the
    thin-left kernel and its kept transposes; 1: as a drop-in caller runs it (real operands may go through the call's own slab
    session, where the mutators act on the slab form)."""
    O = clean
    n, alpha, thr = 1003, -0.5, 1e-7
    cplx, fma = kind == "complex", kind == "real_fma"
    nt.set_option("spgemm_fma", 1 if fma else 0)
    nt.set_option("slab_algebra", slab_algebra)
    O.set_fma(fma)
    Bt = tc.wide_operand(n, 20, cplx=cplx)
    B = nt.Matrix_ps.from_triplets(n, *Bt)
    for mutate in mutators_for(cplx):
        At = tc.thin_operand(n, 31, full_diagonal=True, cplx=cplx)
        A = nt.Matrix_ps.from_triplets(n, *At)
        first, thin1 = gemm(nt, A, B, n, alpha, thr)
        exact(first, oracle_product(O, n, At, Bt, alpha, thr), "%s %s: first product" % (kind, mutate.__name__))
        inplace0 = nt.column_fused_counts()["identity_in_place"]
        A, At2 = mutate(nt, A, At, n)
        if mutate is m_increment_identity:
            assert nt.column_fused_counts()["identity_in_place"] - inplace0 == 1
        second, thin2 = gemm(nt, A, B, n, alpha, thr)
        print(kind, "slab_algebra", slab_algebra, mutate.__name__, "last_spgemm_thin()", thin1, thin2)
        if slab_algebra == 0:
            assert thin1 == 1 and thin2 == 1     # (the thin-left kernel: its kept transpose is what the second product may find)
        assert differs(second, first), mutate.__name__
        exact(A.triplets(), At2, "%s %s: the operand after the change" % (kind, mutate.__name__))
        exact(second, oracle_product(O, n, At2, Bt, alpha, thr), "%s %s: product of the changed operand" % (kind, mutate.__name__))
        nt.release_cache()


@pytest.mark.parametrize("kind", ["real_fma", "complex"])
def test_kept_transposes_slot_eviction(nt, clean, kind):
    """two slots: A1 and A2 fill them, A3 evicts the one used longest ago (A1's); then A1 and A2 change in place and are used again
    -- A1 through a fresh transpose, A2 against its kept one -- and A3, unchanged, against its own"""
    O = clean
    n, alpha, thr = 1003, 1.0, 1e-8
    cplx, fma = kind == "complex", kind == "real_fma"
    nt.set_option("spgemm_fma", 1 if fma else 0)
    nt.set_option("slab_algebra", 0)
    O.set_fma(fma)
    Bt = tc.wide_operand(n, 20, cplx=cplx)
    B = nt.Matrix_ps.from_triplets(n, *Bt)
    ts = [tc.thin_operand(n, seed, full_diagonal=True, cplx=cplx) for seed in (41, 42, 43)]
    As = [nt.Matrix_ps.from_triplets(n, *t) for t in ts]
    firsts = []
    for A, t in zip(As, ts):
        got, thin = gemm(nt, A, B, n, alpha, thr)
        assert thin == 1
        exact(got, oracle_product(O, n, t, Bt, alpha, thr), kind + ": first products")
        firsts.append(got)
    As[0], t0 = m_scale(nt, As[0], ts[0], n)
    As[1], t1 = m_diagonal_scale(nt, As[1], ts[1], n)
    for k, t in ((0, t0), (1, t1), (2, ts[2]), (0, t0)):
        got, thin = gemm(nt, As[k], B, n, alpha, thr)
        assert thin == 1
        assert differs(got, firsts[k]) == (k != 2), k
        exact(got, oracle_product(O, n, t, Bt, alpha, thr), "%s: operand %d after the eviction" % (kind, k + 1))
    nt.release_cache()


# ------------------------------------------------------------------ block forms of the block path
@pytest.mark.parametrize("mutate", mutators_for(False), ids=lambda m: m.__name__)
def test_block_form_of_an_operand_changed_in_place(nt, clean, mutate):
    """A A for a 12^3 lattice operand (n = 1728, no runs) on the block path, twice with A changed in between; the block path's
    contract for real operands (tests/test_gpu_block.py): bit for bit the oracle in FMA mode on the matrices relabelled by the
    engine's positions"""
    from test_gpu_block import oracle_product_in_engine_order
    O = clean
    L, alpha, thr = 12, 1.0, 1e-8
    n = L ** 3
    nt.set_option("spgemm_fma", 1)
    nt.set_option("block_path", 2)
    nt.set_option("slab_algebra", 0)
    O.set_fma(True)
    nt.drop_block_caches()
    At = lattice_triplets(L, shift=0.3701)
    assert np.all(At[2] != 0)
    A = nt.Matrix_ps.from_triplets(n, *At)

    def square(A, t, what):
        C = nt.Matrix_ps(n)
        C.Gemm(A, A, None, alpha, 0.0, thr)
        assert nt.last_block_stats()["used"] == 1, (what, nt.last_block_stats(), nt.last_spgemm_stats())
        got = C.triplets()
        pos = nt.block_order(A)
        assert pos is not None and len(np.unique(pos)) == n
        exact(got, oracle_product_in_engine_order(O, n, t, t, pos, alpha, thr), what)
        return got

    first = square(A, At, "first product")
    A, At2 = mutate(nt, A, At, n)
    second = square(A, At2, mutate.__name__ + ": product of the changed operand")
    assert differs(second, first)
    exact(A.triplets(), At2, mutate.__name__ + ": the operand after the change")
    nt.drop_block_caches()
    nt.release_cache()


# ------------------------------------------------------------------ the operands of the fused TRS2 step
def dense(t, n):
    M = np.zeros((n, n))
    M[t[1] - 1, t[0] - 1] = t[2]
    return M


@pytest.mark.parametrize("relabelled", [False, True], ids=["dot_operand", "relabelled_operand"])
def test_trs2_step_operand_scaled_between_two_steps(nt, clean, relabelled):
    """two fused TRS2 steps (nt.trs2_step) with WH.Scale(3.0) between them, n = 4096, half-width 40: the banded operand (the
    expanded D of the step's energy, kernels.hip dot_operand) and the same band under a seeded symmetric permutation (the
    relabelled D).  The second energy is dot(X_new, 3 WH) evaluated densely in numpy from the iterate read back, relative 1e-11
    -- a stale operand gives a third of it."""
    n, h, thr = 4096, 40, 1e-7
    nt.set_option("spgemm_fma", 1)
    ht = permuted_banded_triplets(n, h, 7) if relabelled else banded_triplets(n, h)
    WH = nt.Matrix_ps.from_triplets(n, *ht)
    e_min, e_max = nt.EigenBounds.GershgorinBounds(WH)
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    X = nt.Matrix_ps(WH)
    X.Scale(-1.0)
    X.Increment(I, e_max, 0.0)
    X.Scale(1.0 / (e_max - e_min))
    X2 = nt.Matrix_ps(n)

    def fused():
        f = nt.fusion_counts()
        return f["square"] + f["update"]

    f0 = fused()
    _, energy1, tr = nt.trs2_step(X, X2, WH, n / 2.0, thr, None)
    f1 = fused()
    WH.Scale(3.0)
    _, energy2, tr = nt.trs2_step(X, X2, WH, n / 2.0, thr, tr)
    f2 = fused()
    print("relabelled", relabelled, "energies", energy1, energy2, "fused steps", f1 - f0, f2 - f1)
    # the first step ran inside the SpGEMM kernel and left the cached operand behind.  The second finds the key changed: the
    # banded operand is expanded again and the step is fused as before; the relabelled form of the iterate has lost its partner
    # and that one step runs on compressed columns (relabel_enter takes the next one) -- either way on the operand as it is now
    assert f1 - f0 == 1 and (relabelled or f2 - f1 == 1), (f0, f1, f2)
    wt = WH.triplets()
    assert np.array_equal(srt(wt)[2], srt(ht)[2] * 3.0)
    Wd = dense(wt, n).ravel()
    want = float(np.dot(dense(X.triplets(), n).ravel(), Wd))
    assert energy2 != energy1
    assert abs(energy2 - want) <= 1e-11 * abs(want), (energy2, want, energy2 / want)
    # a third step, the operand unchanged: whatever the second one cached is the operand
    _, energy3, tr = nt.trs2_step(X, X2, WH, n / 2.0, thr, None)
    print("third step: energy", energy3, "fused steps", fused() - f2)
    want3 = float(np.dot(dense(X.triplets(), n).ravel(), Wd))
    assert abs(energy3 - want3) <= 1e-11 * abs(want3), (energy3, want3, energy3 / want3)
    nt.release_cache()
