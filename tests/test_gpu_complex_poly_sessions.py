"""GPU, FMA arithmetic: complex slab sessions of the polynomial and function families (option complex_poly_sessions;
solvers_poly.cpp, solvers_func.cpp) and the fused recurrence step of the Chebyshev / Hermite loops (slab_extra.hip
slab_recurrence_step_c: Tk = P + a Tkm2 and R <- R + c Tk in one pass).

1. the complex cases of the reference's own polynomial and function fixtures with the option at 2;
2. the session is taken (counters of the slab algebra) and left (results and inputs back in compressed columns);
3. values against a dense complex128 evaluation, bounded by 4 x the deviation of the option-0 path (the behaviour before the
   option existed) from the same evaluation;
4. option 2 against option 1, bit for bit: the fused kernel is the two merges;
5. two ranks against one, bit for bit."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from gen import banded_triplets
from golden_util import Golden, to_dense
from test_gpu_complex_tile import close, srt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "complex_poly_session_worker.py")
OPTION = "complex_poly_sessions"
COUNTERS = ("products", "merges", "others", "refusals", "fused")

POLY = [0.9, -0.5, 0.35, 0.3, -0.25, 0.2, 0.15, -0.1, 0.05]        # 9 coefficients: degree 8
HERMITE = [0.5, 0.2, -0.05, 0.01, 0.002, -0.0004, 0.00005]         # degree 6
CHEBY16 = [0.8 / (1 + k) * (-1) ** k for k in range(17)]           # degree 16


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture()
def fma(nt):
    """FMA arithmetic (what the complex sessions need); the option back at its default and the suite's unfused baseline after"""
    nt.set_option("spgemm_fma", 1)
    yield
    nt.set_option(OPTION, 2)
    nt.set_option("spgemm_fma", 0)


def with_option(nt, value, fn):
    nt.set_option(OPTION, value)
    try:
        return fn()
    finally:
        nt.set_option(OPTION, 2)


def counts(nt):
    """the slab algebra's counters and, as "fused", the fused recurrence steps taken: the one figure that only the fused kernel's
    path moves (a fused step and the two merges it replaces add the same 2 to "merges")"""
    return dict(nt.slab_algebra_counts(), fused=nt.recurrence_step_count())


def delta(c1, c0):
    return {k: c1[k] - c0[k] for k in COUNTERS}


def band(n, h, radius, holes=0.0, seed=0, thin_edge=0):
    """complex Hermitian band of gen.banded_triplets without stored zeros, scaled so that its Gershgorin radius is `radius`;
    holes: that share of the off-diagonal entries dropped; thin_edge: the first and last so many columns keep their diagonal only"""
    c, r, v = banded_triplets(n, h, complex_=True, shift=1e-3)
    k = v != 0
    if holes:
        k &= (np.random.default_rng(seed).random(len(v)) >= holes) | (c == r)
    if thin_edge:
        k &= (c == r) | ((c > thin_edge) & (c <= n - thin_edge))
    c, r, v = c[k], r[k], v[k]
    g = np.zeros(n)
    np.add.at(g, c - 1, np.abs(v))
    return c, r, v * (radius / g.max())


def wide_band(n, h):
    """the band of Gershgorin radius 6 for the exponential and the cosine, negated.  The band's own dominant eigenvalue is negative
    (spectrum about -4.2 .. 2.9): PowerBounds' ten steps from e_1 with Aitken's extrapolation end on a negative estimate, and
    ComputeExponential -- as the reference's -- then scales by 1 and squares nothing.  The negated band's estimate is 11.5:
    sigma = 16, four squarings.  (The cosine scales by the Gershgorin radius, the same for both signs.)"""
    c, r, v = band(n, h, 6.0)
    return c, r, -v


def poly_object(nt, cls, coef):
    poly = cls(len(coef))
    for k, x in enumerate(coef):
        poly.SetCoefficient(k, x)
    return poly


def routines(nt):
    """name -> (run(A, Out, p), products of the evaluation, fused recurrence steps with the option at 2, wants radius ~ 6)"""
    P, C, Hm = nt.Polynomial, nt.ChebyshevPolynomial, nt.HermitePolynomial
    return {
        # Horner, 9 coefficients: one product per II = 7 .. 1
        "horner": (lambda A, O, p: poly_object(nt, P, POLY).HornerCompute(A, O, p), 7, 0, False),
        # Paterson-Stockmeyer, m = 8, s = 2, r = 4: 2 powers, 1 leading block, 3 steps
        "ps": (lambda A, O, p: poly_object(nt, P, POLY).PatersonStockmeyerCompute(A, O, p), 6, 0, False),
        # Chebyshev, degree 8: T2 .. T8
        "cheby": (lambda A, O, p: poly_object(nt, C, POLY).Compute(A, O, p), 7, 7, False),
        # factorized, 9 coefficients: T2, T4 and four recombinations
        "chebyfact": (lambda A, O, p: poly_object(nt, C, POLY).ComputeFactorized(A, O, p), 6, 0, False),
        # Hermite, degree 6: H2 .. H6
        "hermite": (lambda A, O, p: poly_object(nt, Hm, HERMITE).Compute(A, O, p), 5, 5, False),
        # exponential: the degree-15 Chebyshev fit (T2 .. T15) and at least two squarings (wide_band: four)
        "exp": (lambda A, O, p: nt.ExponentialSolvers.ComputeExponential(A, O, p), 16, 14, True),
        # cosine: T2, T4, T6, T8, one block product, three squarings (Gershgorin radius 6: sigma = 8)
        "cos": (lambda A, O, p: nt.TrigonometrySolvers.Cosine(A, O, p), 8, 0, True),
    }


def run(nt, name, A, n, thr=0.0):
    fn = routines(nt)[name][0]
    p = nt.SolverParameters()
    p.SetThreshold(thr)
    Out = nt.Matrix_ps(n)
    c0 = counts(nt)
    fn(A, Out, p)
    return Out, delta(counts(nt), c0)


def assert_bits(got, want, what):
    assert len(got[2]) == len(want[2]) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what + ": pattern"
    assert np.array_equal(got[2].real, want[2].real) and np.array_equal(got[2].imag, want[2].imag), what + ": values"


# ------------------------------------------------------------------ 1. against the real reference
def pmat(nt, t):
    return nt.Matrix_ps.from_triplets(t[0], t[2], t[3], t[4])


def test_polynomial_fixture_complex_cases(nt, fma):
    """tests/golden/polynomials.npz, complex cases (n = 160), option 2: the tolerances of tests/test_gpu_extras.py"""
    g = Golden("polynomials")
    A = pmat(nt, g.tri(None, "A1"))
    n = A.GetActualDimension()
    nt.set_option(OPTION, 2)
    ran = 0
    for i, c in enumerate(g.cases):
        if not c["complex"]:
            continue
        p = nt.SolverParameters()
        p.SetThreshold(c["thr"])
        cls, fn = {"horner": (nt.Polynomial, "HornerCompute"), "ps": (nt.Polynomial, "PatersonStockmeyerCompute"),
                   "cheby": (nt.ChebyshevPolynomial, "Compute"), "chebyfact": (nt.ChebyshevPolynomial, "ComputeFactorized"),
                   "hermite": (nt.HermitePolynomial, "Compute")}[c["kind"]]
        Out = nt.Matrix_ps(n)
        getattr(poly_object(nt, cls, c["coef"]), fn)(A, Out, p)
        want = g.tri(i, "K")
        gd = to_dense((want[0], want[1]) + tuple(Out.triplets()))
        wd = to_dense(want)
        tol = max(100 * c["thr"], 1e-12) * max(1.0, np.abs(wd).max())
        assert np.abs(gd - wd).max() <= tol, (i, c["kind"], len(c["coef"]), np.abs(gd - wd).max())
        if c["thr"] == 0.0:
            assert abs(Out.GetSize() - c["nnz"]) <= 0.002 * c["nnz"] + 2, (i, c["kind"], Out.GetSize(), c["nnz"])
        ran += 1
    assert ran > 0


def test_function_fixture_csym_cases(nt, fma):
    """tests/golden/functions.npz, the csym cases (n = 96; the fixture holds exp and cos for this matrix, its sine is of the real
    one), option 2"""
    g = Golden("functions")
    A = pmat(nt, g.tri(None, "M_csym"))
    n = A.GetActualDimension()
    nt.set_option(OPTION, 2)
    kinds = set()
    for i, c in enumerate(g.cases):
        if c["matrix"] != "csym" or c["kind"] not in ("exp", "cos", "sin"):
            continue
        p = nt.SolverParameters()
        p.SetThreshold(c["thr"])
        p.SetConvergeDiff(c["conv"])
        Out = nt.Matrix_ps(n)
        {"exp": nt.ExponentialSolvers.ComputeExponential, "sin": nt.TrigonometrySolvers.Sine,
         "cos": nt.TrigonometrySolvers.Cosine}[c["kind"]](A, Out, p)
        want = g.tri(i, "K")
        gd = to_dense((want[0], want[1]) + tuple(Out.triplets()))
        wd = to_dense(want)
        tol = max(1000 * c["thr"], 1e-11) * max(1.0, np.abs(wd).max())
        assert np.abs(gd - wd).max() <= tol, (i, c["kind"], np.abs(gd - wd).max())
        kinds.add(c["kind"])
    assert kinds >= {"exp", "cos"}, kinds


# ------------------------------------------------------------------ 2. the session is taken, and left
@pytest.fixture(scope="module")
def bands2048(nt):
    n, h = 2048, 24
    small, large = band(n, h, 0.9), wide_band(n, h)
    return n, {False: (small, nt.Matrix_ps.from_triplets(n, *small)), True: (large, nt.Matrix_ps.from_triplets(n, *large))}


@pytest.mark.parametrize("name", ["horner", "ps", "cheby", "chebyfact", "hermite", "exp", "cos"])
def test_session_is_taken_and_left(nt, fma, bands2048, name):
    from oracle import oracle_py as O
    n, mats = bands2048
    _, products, fused, wide = routines(nt)[name]
    tri, A = mats[wide]
    thr = 1e-9 if wide else 0.0   # (the squarings of exp and cos fill the matrix: a threshold keeps the case small)
    Out, d = with_option(nt, 2, lambda: run(nt, name, A, n, thr))
    print(name, "option 2: slab operations", d)
    assert d["products"] >= products and d["merges"] >= max(products, 2 * fused), (name, d)
    assert d["fused"] == fused, (name, d)   # (every recurrence step of the evaluation was the fused kernel; none elsewhere)
    assert d["refusals"] <= 1, (name, d)
    _, d0 = with_option(nt, 0, lambda: run(nt, name, A, n, thr))
    print(name, "option 0: slab operations", d0)
    assert all(v == 0 for v in d0.values()), (name, d0)
    # the result and the caller's input are back in compressed columns: they read back, the input unchanged, and multiply
    got_in = srt(A.triplets())
    assert_bits(got_in, srt(tri), name + ": the caller's input")
    res = srt(Out.triplets())
    assert len(res[2]) > 0 and np.isfinite(res[2].real).all() and np.isfinite(res[2].imag).all()
    C = nt.Matrix_ps(n)
    C.Gemm(A, Out, None, 1.0, 0.0, 1e-6)
    O.set_fma(True)
    try:
        want = srt(O.ps_multiply(O.Mat.from_triplets(n, n, *got_in), O.Mat.from_triplets(n, n, *res), None, 1.0, 0.0, 1e-6).triplets())
    finally:
        O.set_fma(False)
    close(srt(C.triplets()), want, n, 1e-6, name + ": product after the session")


# ------------------------------------------------------------------ 3. values against an independent dense evaluation
def dense_of(n, t):
    D = np.zeros((n, n), dtype=np.complex128)
    D[t[1] - 1, t[0] - 1] = t[2]
    return D


def dense_power_series(X, c):
    R = c[-1] * np.eye(len(X), dtype=np.complex128)
    for x in c[-2::-1]:
        R = X @ R + x * np.eye(len(X))
    return R


def dense_three_term(X, c, hermite):
    """sum c_k T_k(X) (T_{k+1} = 2 X T_k - T_{k-1}) or sum c_k H_k(X) (H_1 = 2 X, H_{k+1} = 2 X H_k - 2 k H_{k-1})"""
    I = np.eye(len(X), dtype=np.complex128)
    Pm, Pk = I, (2.0 * X if hermite else X.copy())
    R = c[0] * I + c[1] * Pk
    for k in range(1, len(c) - 1):
        Pn = 2.0 * (X @ Pk) - (2.0 * k if hermite else 1.0) * Pm
        R = R + c[k + 1] * Pn
        Pm, Pk = Pk, Pn
    return R


def dense_chebyshev_factorized(X, c):
    """ChebyshevPolynomial::ComputeFactorized's divide and conquer over T_1, T_2, T_4, ... (written for 2^k coefficients; with
    9 it is not sum c_k T_k, and the dense evaluation follows the same recursion)"""
    I = np.eye(len(X), dtype=np.complex128)
    levels = 1
    while (1 << levels) <= len(c):
        levels += 1
    T = [I, X]
    for _ in range(3, levels + 1):
        T.append(2.0 * (T[-1] @ T[-1]) - I)

    def rec(c, depth):
        n = len(c)
        if n <= 2:
            return sum(x * T[k] for k, x in enumerate(c))
        left, right = list(c[:n // 2]), list(c[n // 2:])
        for k in range(1, len(left)):
            left[k] -= c[n - k]
        mid = T[len(T) - depth]
        return 2.0 * (mid @ rec(right, depth + 1)) + rec(left, depth + 1) - right[0] * mid
    return rec(list(c), 1)


def dense_cosine(X):
    """TrigonometrySolvers::Cosine's own evaluation: X / sigma with sigma the power of two at or above the Gershgorin radius, the
    even Chebyshev terms up to T16 through T2, T4, T6, T8 and one product T8 (...), then cos 2x = 2 cos^2 x - 1 per halving"""
    I = np.eye(len(X), dtype=np.complex128)
    d = X.diagonal().real
    off = np.abs(X).sum(axis=0) - np.abs(X.diagonal())
    radius = max(abs((d - off).min()), abs((d + off).max()))
    sigma, squarings = 1.0, 0
    while radius / sigma > 1.0:
        sigma, squarings = 2.0 * sigma, squarings + 1
    S = X / sigma
    c = {1: 7.651976865579664e-01, 3: -2.298069698638004e-01, 5: 4.953277928219409e-03, 7: -4.187667600472235e-05,
         9: 1.884468822397086e-07, 11: -5.261224549346905e-10, 13: 9.999906645345580e-13, 15: -2.083597362700025e-15,
         17: 9.181480886537484e-17}
    T2 = 2.0 * (S @ S) - I
    T4 = 2.0 * (T2 @ T2) - I
    T6 = 2.0 * (T4 @ T2) - T2
    T8 = 2.0 * (T6 @ T2) - T4
    R = T8 @ (0.5 * c[17] * T8 + 0.5 * c[15] * T6 + 0.5 * c[13] * T4 + 0.5 * c[11] * T2)
    R = R + c[9] * T8 + (c[7] + 0.5 * c[11]) * T6 + (c[5] + 0.5 * c[13]) * T4 + (c[3] + 0.5 * c[15]) * T2 + (c[1] + 0.5 * c[17]) * I
    for _ in range(squarings):
        R = 2.0 * (R @ R) - I
    return R


EXP_COEF = [1.266065877752007e+00, 1.130318207984970e+00, 2.714953395340771e-01, 4.433684984866504e-02, 5.474240442092110e-03,
            5.429263119148932e-04, 4.497732295351912e-05, 3.198436462630565e-06, 1.992124801999838e-07, 1.103677287249654e-08,
            5.505891628277851e-10, 2.498021534339559e-11, 1.038827668772902e-12, 4.032447357431817e-14, 2.127980007794583e-15,
            -1.629151584468762e-16]   # (Chebyshev coefficients of exp on [-1, 1]: I_0(1), 2 I_k(1))


def dense_exponential(X):
    """ExponentialSolvers::ComputeExponential's own evaluation: PowerBounds' estimate (ten power steps from e_1, Aitken's
    extrapolation of the last three Ritz values), sigma the power of two at or above it, the degree-15 Chebyshev fit of X / sigma
    by the three-term recurrence, one squaring per halving"""
    v = np.zeros(len(X), dtype=np.complex128)
    v[0] = 1.0
    ritz, estimate = [], 0.0
    for _ in range(10):
        w = X @ v
        ritz.append((np.vdot(v, w) / np.vdot(v, v)).real)
        v = w / np.linalg.norm(w)
        estimate = ritz[-1]
        if len(ritz) >= 3:
            num, den = ritz[-1] * ritz[-3] - ritz[-2] ** 2, ritz[-1] - 2.0 * ritz[-2] + ritz[-3]
            if abs(den) > 1e-14:
                estimate = num / den
    sigma, squarings = 1.0, 0
    while estimate / sigma > 1.0:
        sigma, squarings = 2.0 * sigma, squarings + 1
    assert squarings >= 2, (estimate, squarings)
    R = dense_three_term(X / sigma, EXP_COEF, False)
    for _ in range(squarings):
        R = R @ R
    return R


@pytest.fixture(scope="module")
def dense_references():
    """n = 1024 (a dense complex product of n = 2048 takes seconds on the host; every path the n = 2048 cases take is taken here too);
    each evaluation computed once, read-only afterwards"""
    n, h = 1024, 24
    small, large = band(n, h, 0.9), wide_band(n, h)
    Xs, Xl = dense_of(n, small), dense_of(n, large)
    want = {"horner": dense_power_series(Xs, POLY), "cheby": dense_three_term(Xs, POLY, False),
            "chebyfact": dense_chebyshev_factorized(Xs, POLY), "hermite": dense_three_term(Xs, HERMITE, True),
            "exp": dense_exponential(Xl), "cos": dense_cosine(Xl)}
    want["ps"] = want["horner"]
    for w in want.values():
        w.setflags(write=False)
    return n, {False: small, True: large}, want


@pytest.mark.parametrize("name", ["horner", "ps", "cheby", "chebyfact", "hermite", "exp", "cos"])
def test_values_against_dense_evaluation(nt, fma, dense_references, name):
    """threshold 0.  The bound is 4 x the deviation of the option-0 path -- compressed columns between the operations, the
    behaviour before the option existed -- from the same dense evaluation, floored at 1e-12 max|want|: the factor covers the complex
    tile kernel's 1e-13-per-product tolerance mode compounded over at most 16 products."""
    n, tris, want = dense_references
    wide = routines(nt)[name][3]
    A = nt.Matrix_ps.from_triplets(n, *tris[wide])
    w = want[name]
    dev = {}
    for opt in (0, 2):
        Out, d = with_option(nt, opt, lambda: run(nt, name, A, n, 0.0))
        dev[opt] = float(np.abs(dense_of(n, Out.triplets()) - w).max())
        assert (d["products"] > 0) == (opt == 2), (name, opt, d)
    bound = max(4.0 * dev[0], 1e-12 * float(np.abs(w).max()))
    print("%s: max|want| %.3g, deviation from the dense evaluation: option 0 %.3g, option 2 %.3g, bound %.3g" % (
        name, np.abs(w).max(), dev[0], dev[2], bound))
    assert dev[2] <= bound, (name, dev, bound)


# ------------------------------------------------------------------ 4. the fused kernel, bit for bit
def edge_operands():
    return {"holes": (1003, band(1003, 20, 0.9, holes=0.15, seed=3)),        # n no multiple of 16, ragged column extents
            "thin_edge": (1200, band(1200, 20, 0.9, thin_edge=40)),         # T_{k-2} much narrower than P at the edges
            "band": (2048, band(2048, 24, 0.9))}


@pytest.mark.parametrize("operand", ["holes", "thin_edge", "band"])
def test_fused_step_is_the_two_merges_bit_for_bit(nt, fma, operand):
    n, tri = edge_operands()[operand]
    A = nt.Matrix_ps.from_triplets(n, *tri)
    cases = [("cheby", CHEBY16[:d + 1], d - 1) for d in (3, 4, 9, 16)] + [("hermite", HERMITE, 5)]
    for kind, coef, steps in cases:
        cls = nt.ChebyshevPolynomial if kind == "cheby" else nt.HermitePolynomial
        res = {}
        for opt in (1, 2):
            def go():
                p = nt.SolverParameters()
                p.SetThreshold(0.0)
                Out = nt.Matrix_ps(n)
                c0 = counts(nt)
                poly_object(nt, cls, coef).Compute(A, Out, p)
                return srt(Out.triplets()), delta(counts(nt), c0)
            res[opt] = with_option(nt, opt, go)
        (t1, d1), (t2, d2) = res[1], res[2]
        print(operand, kind, "degree", len(coef) - 1, "option 1", d1, "option 2", d2)
        # the same products; the fused steps are counted as the two merges they replace, and leave no refusal behind
        assert d2["products"] == d1["products"] >= steps and d2["merges"] == d1["merges"] >= 2 * steps, (kind, d1, d2)
        assert d2["refusals"] == d1["refusals"] <= 1, (kind, d1, d2)
        assert d2["fused"] == steps and d1["fused"] == 0, (kind, d1, d2)   # (the fused kernel ran for every step, with 2 only)
        assert_bits(t2, t1, "%s %s degree %d" % (operand, kind, len(coef) - 1))


def test_fused_step_hook_takes_and_declines(nt, fma):
    """the kernel's entry point on operands of the test's own, inside a diagnostic session: with a = 0 (ScaleMatrix by zero would
    store zeros) it declines and every operand is as it was; with a = -1 it is taken and leaves what the two IncrementMatrix calls
    leave on compressed columns, bit for bit"""
    n, tri = edge_operands()["holes"]
    nt.set_option(OPTION, 2)
    A = nt.Matrix_ps.from_triplets(n, *tri)
    wide = nt.Matrix_ps.from_triplets(n, *band(n, 31, 0.7, holes=0.1, seed=5))

    def products():
        P, R = nt.Matrix_ps(n), nt.Matrix_ps(n)
        P.Gemm(A, A, None, 2.0, 0.0, 0.0)
        R.Gemm(wide, A, None, 0.3, 0.0, 0.0)
        return P, R

    Tk = nt.Matrix_ps(n)
    with nt.solver_session(True):
        Pa, Ra = products()
        Pb, Rb = products()
        pre = srt(Pa.triplets()), srt(Ra.triplets())   # (reading packs Pa and Ra; Pb and Rb stay in slab form for the step)
        c0 = counts(nt)
        taken = nt.recurrence_step(Pb, A, Tk, Rb, 0.0, 0.25)
        mid = delta(counts(nt), c0)
        post = srt(Pb.triplets()), srt(A.triplets()), srt(Rb.triplets())
    assert not taken and mid["merges"] == 0 and mid["fused"] == 0, (taken, mid)
    assert Tk.GetSize() == 0
    assert_bits(post[0], pre[0], "P after the declined step")
    assert_bits(post[1], srt(tri), "Tkm2 after the declined step")
    assert_bits(post[2], pre[1], "R after the declined step")
    with nt.solver_session(True):
        P2, R2 = products()
        c1 = counts(nt)
        taken = nt.recurrence_step(P2, A, Tk, R2, -1.0, 0.25)
        d = delta(counts(nt), c1)
        got = srt(Tk.triplets()), srt(R2.triplets())
    assert taken and d["merges"] == 2 and d["fused"] == 1 and d["refusals"] == 0, (taken, d)
    # the two merges on compressed columns, outside any solver session: the IncrementMatrix rules themselves
    P3, R3 = nt.Matrix_ps.from_triplets(n, *pre[0]), nt.Matrix_ps.from_triplets(n, *pre[1])
    P3.Increment(A, -1.0, 0.0)
    R3.Increment(P3, 0.25, 0.0)
    assert_bits(got[0], srt(P3.triplets()), "Tk")
    assert_bits(got[1], srt(R3.triplets()), "R")


# ------------------------------------------------------------------ 5. two ranks
def run_world(world, tmp_path):
    out = str(tmp_path / ("cpoly%d_%s" % (world, uuid.uuid4().hex[:6])))
    name = "q%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name, NTPOLY_AMD_SHM_MB="64")
        procs.append(subprocess.Popen([sys.executable, WORKER, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=180)   # (two small evaluations and the start of a process: seconds)
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


def test_two_ranks_equal_one_rank_bit_for_bit(tmp_path):
    """Chebyshev degree 8 and ComputeExponential on the n = 2048 band, option 2, ranks sharing the GPU over the test transport: the
    gathered result is the one-rank result bit for bit (a column's products and merges have the same bits whoever owns it), and the
    products were complex panel products"""
    one = run_world(1, tmp_path)[0]
    two = run_world(2, tmp_path)
    for tag in ("cheby", "exp"):
        got = tuple(np.concatenate([p[tag + s] for p in two]) for s in ("_col", "_row", "_val"))
        assert_bits(got, tuple(one[tag + s] for s in ("_col", "_row", "_val")), tag + " on two ranks")
        for r, p in enumerate(two):
            print(tag, "rank", r, "panel products (slab, declined)", p[tag + "_panel"], "slab operations", p[tag + "_slab"])
            assert p[tag + "_panel"][0] > 0, (tag, r, p[tag + "_panel"])
        assert one[tag + "_panel"][0] == 0 and one[tag + "_slab"][0] > 0, (tag, one[tag + "_panel"], one[tag + "_slab"])
        # every recurrence step (T2 .. T8; T2 .. T15) was the fused kernel, on each rank's panel as on one rank
        steps = {"cheby": 7, "exp": 14}[tag]
        assert [int(p[tag + "_fused"]) for p in [one] + two] == [steps] * 3, (tag, [int(p[tag + "_fused"]) for p in [one] + two])
    assert one["exp_slab"][0] >= 16, one["exp_slab"]   # (T2 .. T15 and squarings)
