"""GPU, FMA arithmetic: read-only slab views of operands that STORE zeros (option stored_zero_views; kernels.hip slab_enter /
slab_enter_c keep the compressed columns in SlabForm::origin and the row of each column's last stored zero in SlabForm::zlast).

A zero inside a run reads as "no entry", so a matrix that stores one cannot live in slab form alone.  As a view it can still be
READ there: products, norms and dots see a zero of the run, and a merge is exact wherever no stored zero of one operand lies
beyond the other operand's last row (k_sa_axpby) -- otherwise that one merge runs on compressed columns and the view stays.

1. products with a view equal the products of the filtered twin bit for bit, and the oracle within the complex tile kernel's
   tolerance; 2. merges on views equal the compressed-column merge bit for bit, taken or declined as the zlast rule says, real
   and complex; 3. copies and scalings keep the view; 4. the polynomial and function families take an input with stored zeros
   as they take its filtered twin; 5. the complex sign loop; 6. real sign and inverse loops; 7. the option at 0."""
import numpy as np
import pytest

from gen import banded_triplets
from test_gpu_complex_poly_sessions import (HERMITE, POLY, assert_bits, delta, dense_chebyshev_factorized, dense_cosine, dense_exponential,
                                            dense_of, dense_power_series, dense_three_term, routines)
from test_gpu_complex_poly_sessions import counts as slab_counts
from test_gpu_complex_tile import close, srt

pytestmark = pytest.mark.gpu
VIEW = ("built", "products", "taken", "declined")


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
    O.set_fma(True)
    yield O
    O.set_fma(False)
    for name, value in (("stored_zero_views", 1), ("complex_poly_sessions", 2), ("complex_sessions", 1), ("slab_algebra", 1), ("spgemm_fma", 0)):
        nt.set_option(name, value)


def vdelta(v1, v0):
    return {k: v1[k] - v0[k] for k in VIEW}


def scaled(c, r, v, radius):
    g = np.zeros(int(c.max()))
    np.add.at(g, c - 1, np.abs(v))
    return c, r, v * (radius / g.max())


def filtered(t):
    k = t[2] != 0
    return t[0][k], t[1][k], t[2][k]


def z1():
    """Z1: the generator's complex band, n = 2048, h = 24, Gershgorin radius 0.9 -- stored zeros at (500, 500) and (1500, 1500)"""
    t = scaled(*banded_triplets(2048, 24, complex_=True), 0.9)
    z = t[2] == 0
    assert z.sum() == 2 and list(t[0][z]) == [500, 1500] and list(t[1][z]) == [500, 1500]
    return t


Z2_N, Z2_H = 1000, 40


def z2(zero_column=True):
    """Z2: a zero-free complex band, n = 1000 (no multiple of 16 or 64), h = 40 (runs of 81 rows: more than one pass of a wave),
    with stored zeros planted (1-based column, row): the first-row entry of column 100, the last-row entry of column 200, both
    of column 300, an interior off-diagonal of column 400, the diagonal of column 500, all of column 600, entries of columns
    1 and n"""
    n, h = Z2_N, Z2_H
    c, r, v = scaled(*banded_triplets(n, h, complex_=True, shift=1e-3), 0.9)
    assert (v != 0).all()
    v = v.copy()
    plant = (c == 600) if zero_column else np.zeros(len(c), dtype=bool)
    for col, row in ((100, 100 - h), (200, 200 + h), (300, 300 - h), (300, 300 + h), (400, 410), (500, 500), (1, 2), (1, 1 + h), (n, n - 1), (n, n)):
        hit = (c == col) & (r == row)
        assert hit.sum() == 1, (col, row)
        plant |= hit
    v[plant] = 0.0
    return c, r, v


def rz(plant_last_row=False):
    """RZ: the generator's real band, n = 2000, h = 24 (zeros at (500, 500) and (1500, 1500)); optionally a zero planted at the
    last row of column 700"""
    c, r, v = banded_triplets(2000, 24)
    assert ((v == 0) & (c == r)).sum() == 2
    if plant_last_row:
        v = v.copy()
        hit = (c == 700) & (r == 724)
        assert hit.sum() == 1
        v[hit] = 0.0
    return c, r, v


def copy_of(nt, M, n):
    """CopyMatrix into a fresh matrix of the known dimension (Matrix_ps(M) asks M for its dimension first, an entry point that
    sees compressed columns: it would pack a view before copying it)"""
    out = nt.Matrix_ps(n)
    nt.lib.CopyMatrix_ps_wrp(M.ih, out.ih)
    return out


def bits(got, want, what):
    got, want = srt(got), srt(want)
    assert len(got[2]) == len(want[2]) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what + ": pattern"
    gv, wv = np.asarray(got[2]), np.asarray(want[2])
    assert np.array_equal(gv.real, wv.real) and np.array_equal(gv.imag, wv.imag), what + ": values"


# ------------------------------------------------------------------ 1. products
@pytest.mark.parametrize("operand", ["Z2", "Z1"])
def test_products_with_a_view_equal_the_filtered_twin_bit_for_bit(nt, fma, operand):
    O = fma
    zt = z2() if operand == "Z2" else z1()
    n = Z2_N if operand == "Z2" else 2048
    ft = filtered(zt)
    Z, F = nt.Matrix_ps.from_triplets(n, *zt), nt.Matrix_ps.from_triplets(n, *ft)
    assert Z.GetSize() == len(zt[2]) > len(ft[2]) == F.GetSize()   # (the stored zeros are entries)
    with nt.solver_session(True):
        for thr in (0.0, 1e-9):
            FF = nt.Matrix_ps(n)
            FF.Gemm(F, F, None, 1.0, 0.0, thr)
            want = srt(FF.triplets())
            for (A, B, tag) in ((Z, Z, "Z*Z"), (Z, F, "Z*F"), (F, Z, "F*Z")):
                v0, s0 = nt.slab_view_counts(), slab_counts(nt)
                Cm = nt.Matrix_ps(n)
                Cm.Gemm(A, B, None, 1.0, 0.0, thr)
                dv, ds = vdelta(nt.slab_view_counts(), v0), delta(slab_counts(nt), s0)
                print(operand, tag, "threshold", thr, "views", dv, "slab algebra", ds)
                assert dv["products"] == 1 and dv["built"] <= 2 and ds["products"] == 1 and ds["refusals"] == 0, (tag, thr, dv, ds)
                got = srt(Cm.triplets())
                bits(got, want, "%s %s threshold %g against F*F" % (operand, tag, thr))
                if tag == "Z*Z" and operand == "Z2":
                    Zo = O.Mat.from_triplets(n, n, *zt)
                    close(got, srt(O.ps_multiply(Zo, Zo, None, 1.0, 0.0, thr).triplets()), n, thr, "Z2*Z2 against the oracle")
            assert nt.slab_view_counts()["built"] >= 1
    assert Z.GetSize() == len(zt[2])
    bits(Z.triplets(), zt, operand + " after the session: its stored zeros are back")


# ------------------------------------------------------------------ 2. merges
def merge_cases(nt, n, zt, dt):
    """IncrementMatrix inside a session, every alpha and threshold, each against the same call with slab_algebra = 0 bit for bit
    (pattern and values, stored zeros of the result included).  Z (triplets zt): every stored zero lies at or below the last row
    of P = Z*Z and of a view copy's other operand -- (A = Z view, B = P) and (A = P, B = a view copy of Z) must be TAKEN.  D
    (triplets dt, possibly Z itself): stored zeros beyond the identity's one row -- (A = D, B = identity) must be DECLINED, be
    correct all the same, and leave the view standing for the next product; where D has an all-zero column, column of D*D is
    empty and (A = D, B = D*D) is declined too."""
    Z = nt.Matrix_ps.from_triplets(n, *zt)
    D = Z if dt is zt else nt.Matrix_ps.from_triplets(n, *dt)
    # (an identity of the operands' kind: IncrementMatrix of a complex matrix into a REAL one is the mixed-kind path, which no
    # slab session takes)
    eye = np.arange(1, n + 1, dtype=np.int32)
    Ident = nt.Matrix_ps.from_triplets(n, eye, eye, np.ones(n, dtype=np.asarray(zt[2]).dtype))
    kept = {}
    P, PD = nt.Matrix_ps(n), nt.Matrix_ps(n)
    for alpha in (1.0, -1.0, 0.37):
        for thr in (0.0, 1e-9):
            # (a session of its own per case: a declined merge is a refusal in the session's books, and a session that has
            # counted five of them goes back to compressed columns)
            with nt.solver_session(True):
                if not kept:
                    P.Gemm(Z, Z, None, 1.0, 0.0, 0.0)
                    PD.Gemm(D, D, None, 1.0, 0.0, 0.0)
                B1 = copy_of(nt, P, n)
                v0 = nt.slab_view_counts()
                B1.Increment(Z, alpha, thr)                     # A = Z (view), B = P: wider extents
                d1 = vdelta(nt.slab_view_counts(), v0)
                ZC = copy_of(nt, Z, n)                            # (a view copy)
                v0 = nt.slab_view_counts()
                ZC.Increment(P, alpha, thr)                     # A = P, B = the view copy
                d2 = vdelta(nt.slab_view_counts(), v0)
                B3 = copy_of(nt, Ident, n)
                v0, s0 = nt.slab_view_counts(), slab_counts(nt)
                B3.Increment(D, alpha, thr)                     # A = D, B = identity
                d3, s3 = vdelta(nt.slab_view_counts(), v0), delta(slab_counts(nt), s0)
                B4 = copy_of(nt, PD, n)
                v0 = nt.slab_view_counts()
                B4.Increment(D, alpha, thr)                     # A = D, B = D*D
                d4 = vdelta(nt.slab_view_counts(), v0)
                v0 = nt.slab_view_counts()
                Q = nt.Matrix_ps(n)
                Q.Gemm(D, D, None, 1.0, 0.0, 0.0)              # the view is still there
                d5 = vdelta(nt.slab_view_counts(), v0)
            print("alpha", alpha, "threshold", thr, "Z into P", d1, "P into a copy of Z", d2, "D into I", d3, s3, "D into D*D", d4,
                  "next product", d5)
            assert d1["taken"] == 1 and d1["declined"] == 0, (alpha, thr, d1)
            assert d2["taken"] == 1 and d2["declined"] == 0, (alpha, thr, d2)
            assert d3["declined"] == 1 and d3["taken"] == 0 and s3["refusals"] == 1, (alpha, thr, d3, s3)
            assert (d4["declined"], d4["taken"]) == ((1, 0) if D is not Z else (0, 1)), (alpha, thr, d4)
            assert d5["built"] == 0 and d5["products"] == 1, (alpha, thr, d5)
            kept[(alpha, thr)] = (B1, ZC, B3, B4)
    pt, pdt = P.triplets(), PD.triplets()
    results = {key: [m.triplets() for m in mats] for key, mats in kept.items()}
    bits(Z.triplets(), zt, "Z after the sessions")
    bits(D.triplets(), dt, "D after the sessions")
    nt.set_option("slab_algebra", 0)
    try:
        Zc, Dc = nt.Matrix_ps.from_triplets(n, *zt), nt.Matrix_ps.from_triplets(n, *dt)
        for (alpha, thr), got in results.items():
            W1 = nt.Matrix_ps.from_triplets(n, *pt)
            W1.Increment(Zc, alpha, thr)
            W2 = nt.Matrix_ps(Zc)
            W2.Increment(nt.Matrix_ps.from_triplets(n, *pt), alpha, thr)
            W3 = copy_of(nt, Ident, n)
            W3.Increment(Dc, alpha, thr)
            W4 = nt.Matrix_ps.from_triplets(n, *pdt)
            W4.Increment(Dc, alpha, thr)
            for g, W, tag in zip(got, (W1, W2, W3, W4), ("Z into P", "P into a copy of Z", "D into I", "D into D*D")):
                assert W.GetSize() == len(g[2]), (tag, alpha, thr, W.GetSize(), len(g[2]))
                bits(g, W.triplets(), "%s, alpha %g threshold %g" % (tag, alpha, thr))
            # (the declined merge's result keeps the stored zeros that lie beyond the identity's one row)
            assert (np.asarray(got[2][2]) == 0).sum() > 0
    finally:
        nt.set_option("slab_algebra", 1)


def test_merges_on_complex_views(nt, fma):
    """Z2 as planted, all-zero column included, is the operand of the declined pairs.  The taken pairs use Z2 WITHOUT the all-zero
    column: column 600 of Z2*Z2 is empty, so every stored zero of that column lies beyond it and IncrementMatrix(Z2, Z2*Z2) has
    to store zeros -- by the zlast rule itself that pair is declined, and it is checked here as such (D into D*D)."""
    merge_cases(nt, Z2_N, z2(zero_column=False), z2())


def test_merges_on_real_views(nt, fma):
    t = rz(plant_last_row=True)
    merge_cases(nt, 2000, t, t)


# ------------------------------------------------------------------ 3. copy and scale
def test_copy_and_scale_keep_the_view(nt, fma):
    zt = z2()
    ft = filtered(zt)
    n = Z2_N
    Z, F = nt.Matrix_ps.from_triplets(n, *zt), nt.Matrix_ps.from_triplets(n, *ft)
    with nt.solver_session(True):
        P = nt.Matrix_ps(n)
        P.Gemm(Z, Z, None, 1.0, 0.0, 0.0)
        v0 = nt.slab_view_counts()
        ZC = copy_of(nt, Z, n)
        Z.Scale(2.0)
        F.Scale(2.0)
        d = vdelta(nt.slab_view_counts(), v0)
        assert d["taken"] == 2 and d["built"] == 0, d
        PZ, PF = nt.Matrix_ps(n), nt.Matrix_ps(n)
        PZ.Gemm(Z, Z, None, 1.0, 0.0, 0.0)
        PF.Gemm(F, F, None, 1.0, 0.0, 0.0)
        d = vdelta(nt.slab_view_counts(), v0)
        assert d["built"] == 0 and d["products"] == 1, d
        bits(PZ.triplets(), PF.triplets(), "product of the scaled view against the product of the scaled twin")
    bits(ZC.triplets(), zt, "CopyMatrix of a view")
    bits(Z.triplets(), (zt[0], zt[1], 2.0 * zt[2]), "the scaled view after the session")


# ------------------------------------------------------------------ 4. the polynomial and function families
@pytest.fixture(scope="module")
def routine_operands():
    zt = z1()
    wide = scaled(zt[0], zt[1], -zt[2], 6.0)   # (negated, Gershgorin radius 6: test_gpu_complex_poly_sessions.wide_band)
    return {False: zt, True: wide}


class Banded(np.ndarray):
    """a dense complex128 matrix whose products go through scipy.sparse while both operands are mostly zero (the powers of a band
    at n = 2048): the same sums of the same products, a fraction of the host time"""

    def __matmul__(self, other):
        a, b = np.asarray(self), np.asarray(other)
        if a.ndim == 2 and b.ndim == 2 and np.count_nonzero(a) < 0.2 * a.size and np.count_nonzero(b) < 0.2 * b.size:
            import scipy.sparse as sp
            return (sp.csr_matrix(a) @ sp.csr_matrix(b)).toarray().view(Banded)
        return (a @ b).view(Banded)


def dense_want(name, X):
    X = X.view(Banded)
    if name in ("horner", "ps"):
        return dense_power_series(X, POLY)
    if name == "cheby":
        return dense_three_term(X, POLY, False)
    if name == "chebyfact":
        return dense_chebyshev_factorized(X, POLY)
    if name == "hermite":
        return dense_three_term(X, HERMITE, True)
    return dense_exponential(X) if name == "exp" else dense_cosine(X)


def run_routine(nt, name, A, n):
    fn = routines(nt)[name][0]
    p = nt.SolverParameters()
    p.SetThreshold(0.0)
    Out = nt.Matrix_ps(n)
    c0, v0 = slab_counts(nt), nt.slab_view_counts()
    fn(A, Out, p)
    return Out, delta(slab_counts(nt), c0), vdelta(nt.slab_view_counts(), v0)


@pytest.mark.parametrize("name", ["horner", "ps", "cheby", "chebyfact", "hermite", "exp", "cos"])
def test_routines_take_an_input_with_stored_zeros(nt, fma, routine_operands, name):
    """threshold 0; values bounded by 4 x the deviation of the complex_poly_sessions = 0 path from the same dense complex128
    evaluation, floored at 1e-12 max|want| (the rule of test_gpu_complex_poly_sessions.py)"""
    n = 2048
    wide = routines(nt)[name][3]
    zt = routine_operands[wide]
    ft = filtered(zt)
    Z, F = nt.Matrix_ps.from_triplets(n, *zt), nt.Matrix_ps.from_triplets(n, *ft)
    nt.set_option("complex_poly_sessions", 2)
    OutZ, dz, vz = run_routine(nt, name, Z, n)
    OutF, df, vf = run_routine(nt, name, F, n)
    print(name, "Z1:", dz, vz, "F1:", df, vf)
    assert dz["products"] == df["products"] > 0, (name, dz, df)
    assert dz["refusals"] <= df["refusals"], (name, dz, df)
    view_steps = 1 if df["fused"] else 0   # (the one step whose Tkm2 is the input's copy, T1)
    assert dz["fused"] >= df["fused"] - view_steps, (name, dz, df)
    assert 1 <= vz["built"] <= 2 and vz["products"] >= 1, (name, vz)
    assert all(v == 0 for v in vf.values()), (name, vf)
    bits(Z.triplets(), zt, name + ": the caller's input")
    nt.set_option("complex_poly_sessions", 0)
    Out0, d0, v0 = run_routine(nt, name, Z, n)
    nt.set_option("complex_poly_sessions", 2)
    assert d0["products"] == 0 and all(v == 0 for v in v0.values()), (name, d0, v0)
    want = dense_want(name, dense_of(n, zt))
    dev0 = float(np.abs(dense_of(n, Out0.triplets()) - want).max())
    dev2 = float(np.abs(dense_of(n, OutZ.triplets()) - want).max())
    bound = max(4.0 * dev0, 1e-12 * float(np.abs(want).max()))
    print("%s: max|want| %.3g, deviation from the dense evaluation: option 0 %.3g, option 2 on the view %.3g, bound %.3g" % (
        name, np.abs(want).max(), dev0, dev2, bound))
    assert dev2 <= bound, (name, dev0, dev2, bound)


# ------------------------------------------------------------------ 5. the complex sign loop
def test_complex_sign_loop_on_an_input_with_stored_zeros(nt, fma):
    n, h, thr = 2048, 24, 1e-8
    zt = banded_triplets(n, h, complex_=True)
    assert (zt[2] == 0).sum() == 2
    ft = filtered(zt)

    def sign(t, sessions):
        nt.set_option("complex_sessions", sessions)
        try:
            H = nt.Matrix_ps.from_triplets(n, *t)
            p = nt.SolverParameters()
            p.SetThreshold(thr)
            p.SetConvergeDiff(1e-9)
            S = nt.Matrix_ps(n)
            c0, v0 = slab_counts(nt), nt.slab_view_counts()
            nt.SignSolvers.ComputeSign(H, S, p)
            return srt(S.triplets()), nt.solver_trace()["iterations"], delta(slab_counts(nt), c0), vdelta(nt.slab_view_counts(), v0)
        finally:
            nt.set_option("complex_sessions", 1)

    got, it, d, v = sign(zt, 1)
    want, it0, d0, _ = sign(zt, 0)
    _, itf, df, vf = sign(ft, 1)
    print("sign: iterations", it, it0, itf, "with stored zeros", d, v, "filtered", df, vf)
    assert it == it0 and it >= 5
    assert d0["products"] == 0 and d["products"] == 2 * it, (d, it)
    close(got, want, n, thr, "sign with / without the complex session")
    assert d["refusals"] <= df["refusals"], (d, df)
    assert v["built"] >= 1 and v["products"] >= 2, v


# ------------------------------------------------------------------ 6. real loops
def test_real_sign_and_inverse_loops_on_views(nt, fma):
    from test_gpu_slab_algebra import run, same_pattern
    n = 2000
    zt = rz()
    H = nt.Matrix_ps.from_triplets(n, *zt)
    taken = 0
    for solver, iters in (("sign", None), ("invert", 12)):
        nt.set_option("slab_algebra", 0)
        want, tr0, _ = run(nt, solver, H, n, 1e-8, 1e-8, iters)
        nt.set_option("slab_algebra", 1)
        c0, v0 = slab_counts(nt), nt.slab_view_counts()
        got, tr1, _ = run(nt, solver, H, n, 1e-8, 1e-8, iters)
        d, v = delta(slab_counts(nt), c0), vdelta(nt.slab_view_counts(), v0)
        print(solver, "iterations", tr1["iterations"], "slab algebra", d, "views", v)
        assert tr0["iterations"] == tr1["iterations"]
        assert same_pattern(got, want) and np.array_equal(got[2], want[2]), solver
        assert d["refusals"] == 0 and d["products"] >= 2 * (tr1["iterations"] - 1), (solver, d)
        assert v["built"] >= 1 and v["products"] >= 1 and v["declined"] == 0, (solver, v)
        taken += v["taken"]
    assert taken >= 1
    bits(H.triplets(), zt, "the caller's input")


# ------------------------------------------------------------------ 7. the option at 0
def test_option_zero_is_the_behaviour_without_views(nt, fma, routine_operands):
    n = 2048
    zt = routine_operands[False]
    Z = nt.Matrix_ps.from_triplets(n, *zt)
    nt.set_option("stored_zero_views", 0)
    try:
        Out, d, v = run_routine(nt, "cheby", Z, n)
    finally:
        nt.set_option("stored_zero_views", 1)
    print("stored_zero_views = 0:", d, v)
    assert d["products"] == 0 and d["fused"] == 0, d
    assert all(x == 0 for x in v.values()), v
    Out1, d1, v1 = run_routine(nt, "cheby", Z, n)
    assert d1["products"] == 7 and v1["products"] >= 1, (d1, v1)
    close(srt(Out.triplets()), srt(Out1.triplets()), n, 0.0, "Chebyshev with the option at 0 and at 1")
