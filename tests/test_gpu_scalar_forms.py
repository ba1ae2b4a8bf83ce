"""GPU: the scalar reductions in every storage form against exact sums (operands and references: tests/scalar_reference.py).

Dot (both parts), Trace, Norm, Sigma, GershgorinBounds and MeasureAsymmetry decide every solver's step size and stopping
iteration, and the fused passes state their own correctness as "the bits of DotMatrix / MatrixTrace / MatrixNorm".  Here they
are compared with references that owe nothing to the engine: int64 arithmetic on the integer family (EQUALITY, no tolerance),
the correctly rounded exact sum on the real family with |error| <= 1.01 (k + 1) 2^-53 sum |term| (one dropped, doubled or
mis-paired entry exceeds it: tests/test_scalar_reference_cpu.py), a cancelling pair whose exact sum is 0, and for the
Gershgorin ends 2^-52 (|d| + R) on the matrix and on a randomly relabelled copy.

Shapes, from the constants of csrc/kernels.hip quoted in scalar_reference.py -- k_dot: LDS window W = 1024 rows, LDS row-id
search up to 1024 entries, global search beyond, 5 x 64 entries preloaded, a second column per wave beyond 32 768 columns; the
two-level sums and the min / max reduction: one stage up to 8192 partials, chunks of 2048 above; k_trace and the min / max
reduction: a strided pass beyond 262 144 columns:
  mixed     n = 1500     every column kind on the A side and the B side independently, diagonal first / last / absent
  long      n = 33 000   tridiagonal, the wide kinds beyond column 32 768
  partials  n = 10 500   band of half width 40, extreme columns at 0, 8191, 8192, n - 1 in separate operands; disjoint runs
  strided   n = 262 444  tridiagonal, integer family, extremes and a missing diagonal beyond column 262 144

Reachable (form, scalar) pairs -- every case prints the form it ran in, proved by the counters:
  compressed columns   Dot (real, complex, mixed in both orders), Trace, Norm, Gershgorin, MeasureAsymmetry, Sigma (the ABI
                       has no MatrixSigma: read from the trace of one Invert iteration, which records 1 / (N N))
  real slab form       (slab_algebra = 1, FMA arithmetic, one-call sessions; operands enter through a product X I or a copy)
                       Dot, Trace, Norm.  GershgorinBounds and MeasureAsymmetry pack their operand at the ABI; the only call of
                       slab_gershgorin is the first step of the order-2 inverse square root, which exposes
                       lambda = 1 / max(|lo|, |hi|) in its trace: asserted through that.  For a real matrix
                       max(|d - r|, |d + r|) = |d| + r is the column's whole sum whichever entry is taken for the diagonal.
  read-only view       (an operand with a stored zero, stored_zero_views) Dot, Trace, Norm
  complex slab form    (inside a solver session that takes complex operands) Norm; Trace under option complex_scale_fold
                       (without it Trace packs the operand); Re Dot through the energy pass of complex TRS4 (option complex_trs4),
                       against a slab-form and a compressed second operand.  DotMatrix packs (the real slab_dot declines
                       complex operands) and is still right
  block form           (12^3 lattice, block_path = 2 / block_complex) Dot(block, compressed), Dot(compressed, block) with
                       a non-zero imaginary part, Trace, Norm
  not reachable        the grand sum (kernels.hip grand_sum has no caller and no ABI entry); Sigma, Gershgorin and
                       MeasureAsymmetry of a matrix in slab or block form (the entry points pack first).
Norm of a complex PRODUCT sums moduli of general Gaussian integers, which are not integers: that one is held to the real
family's bound.  The ranks are tests/scalar_forms_worker.py, run from here."""
import ctypes as C
import os
import subprocess
import sys
import time
import uuid

import numpy as np
import pytest

import scalar_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


OPTIONS = (("spgemm_fma", 0), ("slab_algebra", 1), ("block_path", 1), ("block_complex", 1), ("complex_tile", 1), ("complex_sessions", 1),
           ("stored_zero_views", 1), ("complex_scale_fold", 0), ("complex_trs4", 0))


@pytest.fixture(params=["fma", "unfused"])
def arith(nt, request):
    nt.set_option("spgemm_fma", 1 if request.param == "fma" else 0)
    yield request.param      # (test_compressed_columns switches slab_algebra off: everything back to its default)
    for name, value in OPTIONS:
        nt.set_option(name, value)


@pytest.fixture()
def fma(nt):
    for name, value in OPTIONS:
        nt.set_option(name, value)
    nt.set_option("spgemm_fma", 1)
    yield
    for name, value in OPTIONS:
        nt.set_option(name, value)


def ident(key):
    return "%s-%s-%s" % (key[0], key[1], "c" if key[2] else "r")


# ------------------------------------------------------------------ engine calls (straight at the ABI: Matrix_ps.Dot asks
# IsComplex first, an entry point that packs its matrix)
def mat(nt, n, t):
    return nt.Matrix_ps.from_triplets(n, *t)


def dot(nt, A, B, cplx):
    if cplx:
        re, im = C.c_double(), C.c_double()
        nt.lib.DotMatrix_psc_wrp(A.ih, B.ih, C.byref(re), C.byref(im))
        return re.value, im.value
    v = C.c_double()
    nt.lib.DotMatrix_psr_wrp(A.ih, B.ih, C.byref(v))
    return v.value, 0.0


def identity(nt, n, cplx):
    if not cplx:
        I = nt.Matrix_ps(n)
        I.FillIdentity()
        return I
    j = np.arange(1, n + 1, dtype=np.int32)
    return mat(nt, n, (j, j, np.ones(n, dtype=complex)))


def one_step(nt, solver, A, n):
    """the `sigma` the first iteration of a solver records: Invert -> 1 / (N N); order-2 inverse square root -> 1 / max(|lo|, |hi|)
    of the Gershgorin bounds of A I, taken in the loop's own session"""
    p = nt.SolverParameters()
    p.SetThreshold(0.0)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(1)
    Out = nt.Matrix_ps(n)
    if solver == "invert":
        nt.InverseSolvers.Invert(A, Out, p)
    else:
        nt.SquareRootSolvers.with_order(A, Out, p, True, 2)
    return float(nt.solver_trace()["sigma"][0])


def slab(nt):
    return nt.slab_algebra_counts()


def moved(c1, c0):
    return {k: c1[k] - c0[k] for k in c0}


# ------------------------------------------------------------------ references (made once per case, shared, left unchanged)
_EXPECTED = {}


def want_dot(c, a, b):
    key = (c["id"], "dot", a, b)
    if key not in _EXPECTED:
        ta, tb = c["ops"][a], c["ops"][b]
        _EXPECTED[key] = (R.dot_int(ta, tb, c["n"]), (0.0, 0.0)) if c["family"] == "int" else R.dot_real(ta, tb, c["n"])
    return _EXPECTED[key]


def want_single(c, name, what, t=None):
    """(value, tolerance) -- Gershgorin: ((lo, hi), (tol, tol))"""
    key = (c["id"], what, name)
    if key in _EXPECTED:
        return _EXPECTED[key]
    t = c["ops"][name] if t is None else t
    n, exact = c["n"], c["family"] == "int"
    if what == "trace":
        v = (R.trace_int(t), 0.0) if exact else R.trace_real(t)
    elif what == "norm":
        v = (R.norm_int(t, n), 0.0) if exact else R.norm_real(t, n)
    elif what == "gershgorin":
        v = (R.gershgorin_int(t, n), (0.0, 0.0)) if exact else R.gershgorin_real(t, n)
    elif what == "sigma":
        v = (R.sigma_int(t, n), 0.0) if exact else R.sigma_real(t, n)
    elif what == "asymmetry":
        # (the differences of Gaussian integers have no integer moduli: a complex operand is held to the bound in either family)
        d = R.asymmetry_operand(t, n)
        v = (R.norm_int(d, n), 0.0) if exact and not c["cplx"] else R.norm_real(d, n)
    elif what == "lambda":
        (lo, hi), (tl, th) = want_single(c, name, "gershgorin", t)
        m = max(abs(lo), abs(hi))
        # (1 / m: the relative tolerance of the end that gives m, and the rounding of the quotient on either side)
        v = (1.0 / m, 0.0 if exact else (1.0 / m) * 1.01 * (max(tl, th) / m + 2.0 * R.U))
    _EXPECTED[key] = v
    return v


def check(what, form, got, want, tol):
    err = abs(got - want)
    print("  %-34s [%s] got %.17g want %.17g |d| %.3g allowed %.3g" % (what, form, got, want, err, tol))
    assert err <= tol, "%s in %s: got %.17g, want %.17g, |d| = %.3g > %.3g" % (what, form, got, want, err, tol)


def check_dot(nt, c, form, M, a, b):
    cplx = np.iscomplexobj(c["ops"][a][2]) or np.iscomplexobj(c["ops"][b][2])
    got = dot(nt, M[a], M[b], cplx)
    (re, im), (tre, tim) = want_dot(c, a, b)
    check("%s Re Dot(%s, %s)" % (c["id"], a, b), form, got[0], re, tre)
    check("%s Im Dot(%s, %s)" % (c["id"], a, b), form, got[1], im, tim)


def check_singles(nt, c, form, M, name, which=("trace", "norm")):
    for what in which:
        got = M[name].Trace() if what == "trace" else M[name].Norm()
        v, tol = want_single(c, name, what)
        check("%s %s(%s)" % (c["id"], what, name), form, got, v, tol)


# ------------------------------------------------------------------ compressed columns
RELABEL_MISMATCHES = []


@pytest.mark.parametrize("key", R.CASE_TABLE, ids=ident)
def test_compressed_columns(nt, arith, key):
    t0 = time.time()
    c = R.case(*key)
    n, form = c["n"], "compressed columns, " + arith
    nt.set_option("slab_algebra", 0)
    M = {name: mat(nt, n, t) for name, t in c["ops"].items()}
    s0, b0 = slab(nt), nt.block_algebra_counts()
    for a, b in c["dots"]:
        check_dot(nt, c, form, M, a, b)
    for name in c["singles"]:
        check_singles(nt, c, form, M, name)
        (lo, hi), (tl, th) = want_single(c, name, "gershgorin")
        g = nt.EigenBounds.GershgorinBounds(M[name])
        check("%s Gershgorin lower(%s)" % (c["id"], name), form, g[0], lo, tl)
        check("%s Gershgorin upper(%s)" % (c["id"], name), form, g[1], hi, th)
        if c["family"] == "real" and name in ("A", "P0"):
            # the same contract on a randomly relabelled copy; how many of the two ends differ in their bits is MEASURED
            perm = np.random.default_rng(77).permutation(n)
            g2 = nt.EigenBounds.GershgorinBounds(mat(nt, n, R.relabelled(c["ops"][name], n, perm)))
            check("%s Gershgorin lower(relabelled %s)" % (c["id"], name), form, g2[0], lo, tl)
            check("%s Gershgorin upper(relabelled %s)" % (c["id"], name), form, g2[1], hi, th)
            RELABEL_MISMATCHES.append((c["id"], arith, int(g[0] != g2[0]) + int(g[1] != g2[1])))
            print("  GERSHGORIN-RELABEL %s %s: %d of 2 ends differ in their bits (so far %d of %d)" % (
                c["id"], arith, RELABEL_MISMATCHES[-1][2], sum(m[2] for m in RELABEL_MISMATCHES), 2 * len(RELABEL_MISMATCHES)))
    if c["shape"] == "mixed":
        v, tol = want_single(c, "A", "asymmetry")
        check("%s MeasureAsymmetry(A)" % c["id"], form, M["A"].MeasureAsymmetry(), v, tol)
        v, tol = want_single(c, "A", "sigma")
        check("%s Sigma(A)" % c["id"], form, one_step(nt, "invert", M["A"], n), v, tol)
    assert slab(nt) == s0 and nt.block_algebra_counts() == b0      # nothing left compressed columns
    print("%s in %s: %.2f s" % (c["id"], form, time.time() - t0))


def test_hypot_is_exact_on_pythagorean_pairs(nt):
    """the probe behind the integer family's modulus-based scalars: one column per pair, Norm must be the integer modulus"""
    pairs = [(3, 4), (4, 3), (5, 12), (12, 5), (8, 15), (15, 8), (-3, 4), (5, -12), (-8, -15), (0, 7), (-6, 0)]
    inexact = []
    for x, y in pairs:
        A = mat(nt, 4, (np.array([2], dtype=np.int32), np.array([3], dtype=np.int32), np.array([complex(x, y)])))
        got, want = A.Norm(), float(round(np.hypot(x, y)))
        print("  hypot(%d, %d) on the device: %.17g (%s)" % (x, y, got, "exact" if got == want else "INEXACT"))
        if got != want:
            inexact.append((x, y, got))
    assert not inexact, inexact


# ------------------------------------------------------------------ real slab form and read-only views (FMA arithmetic)
def into_slab(nt, X, n, I, must=True):
    """X I in a one-call session: the product stays in slab form and X is converted where it is.  Returns (product, in slab form)"""
    c0 = slab(nt)
    T = nt.Matrix_ps(n)
    T.Gemm(X, I, None, 1.0, 0.0, 0.0)
    d = moved(slab(nt), c0)
    ok = d["products"] == 1 and d["refusals"] == 0
    assert ok or not must, "the product X I did not stay in slab form: %s" % d
    if not ok:
        print("  the product X I did not stay in slab form (operations in slab form moved by %s): compressed columns from here" % d)
    return T, ok


def counted(nt, fn, expect, form):
    """run one scalar call; `expect` operations in slab form (None: whatever) and no refusal"""
    c0 = slab(nt)
    out = fn()
    d = moved(slab(nt), c0)
    if expect is not None:
        assert d["others"] == expect and d["refusals"] == 0, "%s: the counter of operations in slab form moved by %s" % (form, d)
    return out, d


SLAB_CASES = [k for k in R.CASE_TABLE if not k[2]]


@pytest.mark.parametrize("key", SLAB_CASES, ids=ident)
def test_real_slab_form(nt, fma, key):
    t0 = time.time()
    c = R.case(*key)
    n = c["n"]
    I = identity(nt, n, False)
    X = {name: mat(nt, n, t) for name, t in c["ops"].items() if not np.iscomplexobj(t[2])}
    # the mixed case holds columns no slab form is made for: packs or refuses, and is still right
    must = c["shape"] != "mixed"
    S, in_slab = {}, True
    for name in X:
        S[name], ok = into_slab(nt, X[name], n, I, must)
        in_slab = in_slab and ok
    first = c["singles"][0]
    Cp = nt.Matrix_ps(n)
    c0 = slab(nt)
    nt.lib.CopyMatrix_ps_wrp(S[first].ih, Cp.ih)
    if in_slab:
        assert moved(slab(nt), c0)["merges"] == 1, moved(slab(nt), c0)
    for form, M in (("slab form (product)", S), ("slab form (operand converted in place)", X), ("slab form (copy)", {first: Cp})):
        form = form if in_slab else "slab form refused, compressed columns"
        expect = 1 if in_slab else None
        for a, b in c["dots"]:
            if a in M and b in M and not np.iscomplexobj(c["ops"][a][2]) and not np.iscomplexobj(c["ops"][b][2]):
                counted(nt, lambda: check_dot(nt, c, form, M, a, b), expect, form)
        for name in c["singles"]:
            if name in M:
                for what in ("trace", "norm"):
                    counted(nt, lambda: check_singles(nt, c, form, M, name, (what,)), expect, form)
    if c["shape"] in ("partials", "strided"):
        # the Gershgorin bounds of a slab-form matrix: the first step of the order-2 inverse square root takes them of A I
        for name in c["singles"]:
            if name == "Q":
                continue
            v, tol = want_single(c, name, "lambda")
            c0 = slab(nt)
            got = one_step(nt, "isr2", mat(nt, n, c["ops"][name]), n)
            d = moved(slab(nt), c0)
            assert d["products"] >= 1 and d["others"] >= 1 and d["refusals"] == 0, d
            check("%s 1 / max |Gershgorin end|(%s)" % (c["id"], name), "slab form (solver loop)", got, v, tol)
    print("%s in real slab form: %.2f s" % (c["id"], time.time() - t0))


@pytest.mark.parametrize("family", ["int", "real"])
def test_read_only_view(nt, fma, family):
    """P1 of the partials case with stored zeros planted -- an interior entry, a diagonal entry, one inside the extreme column
    and the first entry of a column: the operand enters slab form as a read-only view that keeps its compressed columns"""
    t0 = time.time()
    c = R.case("partials", family, False)
    n = c["n"]
    col, row, val = c["ops"]["P1"]
    val = val.copy()
    ext = R.PARTIALS_EXTREME[1] + 1
    for cc, rr in ((100, 110), (200, 200), (ext, ext + 3), (300, 260)):
        hit = np.flatnonzero((col == cc) & (row == rr))
        assert len(hit) == 1
        val[hit[0]] = 0.0
    zc = dict(c, id=c["id"] + "-zeros", ops=dict(c["ops"], Z=(col, row, val)))
    I = identity(nt, n, False)
    Z, P0 = mat(nt, n, zc["ops"]["Z"]), mat(nt, n, c["ops"]["P0"])
    assert Z.GetSize() == len(val)
    v0 = nt.slab_view_counts()
    into_slab(nt, Z, n, I)
    S0, _ = into_slab(nt, P0, n, I)
    assert nt.slab_view_counts()["built"] == v0["built"] + 1
    form = "read-only view"
    M = {"Z": Z, "P0": S0}
    for a, b in (("Z", "P0"), ("P0", "Z"), ("Z", "Z")):
        counted(nt, lambda: check_dot(nt, zc, form, M, a, b), 1, form)
    for what in ("trace", "norm"):
        counted(nt, lambda: check_singles(nt, zc, form, M, "Z", (what,)), 1, form)
    assert Z.GetSize() == len(val)          # (the stored zeros are still entries)
    print("%s as a read-only view: %.2f s" % (zc["id"], time.time() - t0))


COMPLEX_SLAB_CASES = [k for k in R.CASE_TABLE if k[2] and k[0] in ("partials", "long")]


@pytest.mark.parametrize("key", COMPLEX_SLAB_CASES, ids=ident)
def test_complex_slab_form(nt, fma, key):
    """inside a session that takes complex operands a complex product stays in slab form.  Norm reads its runs (slab_norm_c).
    Trace reads them under option complex_scale_fold (slab_dot_trace_c) and packs the operand without it.  The real part of
    Dot(X, W) comes from one pass over the runs of X under option complex_trs4 (the energy pass of the complex TRS4 loop,
    slab_dot_trace_c with W in slab form and with W in compressed columns).  DotMatrix itself packs complex operands (the real
    slab_dot declines them) and is still right"""
    t0 = time.time()
    c = R.case(*key)
    n = c["n"]
    I = identity(nt, n, True)
    a, b = [x for x in c["singles"] if x != "Q"][:2]
    X = {name: mat(nt, n, c["ops"][name]) for name in (a, b)}
    form = "complex slab form"
    with nt.solver_session(True):
        S = {name: into_slab(nt, X[name], n, I)[0] for name in (a, b)}
        for name in (a, b):
            counted(nt, lambda: check_singles(nt, c, form, S, name, ("norm",)), 1, form)
        nt.set_option("complex_scale_fold", 1)
        for name in (a, b):
            counted(nt, lambda: check_singles(nt, c, form, S, name, ("trace",)), 1, form)
        nt.set_option("complex_scale_fold", 0)
        nt.set_option("complex_trs4", 1)
        (re, _), (tre, _) = want_dot(c, a, b)
        W = mat(nt, n, c["ops"][b])
        for other, wform in ((S[b], form + ", both operands"), (W, form + ", second operand in compressed columns")):
            (got, d) = counted(nt, lambda: nt.trs4_energy(S[a], other), 1, wform)
            assert got is not None, "the energy pass was refused"
            check("%s Re Dot(%s, %s)" % (c["id"], a, b), wform, got, re, tre)
        nt.set_option("complex_trs4", 0)
        _, d = counted(nt, lambda: check_singles(nt, c, "complex slab form operand, packed by Trace", S, a, ("trace",)), None, form)
        assert d["others"] == 0, d
        _, d = counted(nt, lambda: check_dot(nt, c, "complex slab form operand, packed by Dot", S, b, a), None, form)
        assert d["others"] == 0, d
    print("%s in complex slab form: %.2f s" % (c["id"], time.time() - t0))


# ------------------------------------------------------------------ block form
LATTICE = 12


def lattice_operands(cplx):
    """the lattice operand of tests/test_gpu_block.py (its pattern) with integer values, a second one on a thinner stencil,
    and their exact products"""
    key = ("lattice", cplx)
    if key not in _EXPECTED:
        from gen import lattice_triplets
        n = LATTICE ** 3
        col, row, _ = lattice_triplets(LATTICE)
        A = (col, row, R.lattice_values(0, len(col), cplx))
        col, row, _ = lattice_triplets(LATTICE, r2=6)
        B = (col, row, R.lattice_values(1, len(col), cplx))
        Ad = R.dense(A, n)
        AA = Ad @ Ad                      # (integers far below 2^53: exact in any order)
        assert np.array_equal(AA, np.rint(AA.real) + 1j * np.rint(AA.imag) if cplx else np.rint(AA))
        _EXPECTED[key] = (n, A, B, R.from_dense(AA), AA)
    return _EXPECTED[key]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_block_form(nt, fma, cplx):
    t0 = time.time()
    n, A, B, AA, AAd = lattice_operands(cplx)
    c = {"id": "lattice12-int-%s" % ("c" if cplx else "r"), "n": n, "family": "int", "cplx": cplx, "ops": {"AA": AA, "B": B}}
    nt.set_option("block_path", 2)
    nt.set_option("block_complex", 1)
    nt.set_option("complex_tile", 1)
    nt.set_option("complex_sessions", 1)
    nt.set_option("slab_algebra", 1)
    nt.drop_block_caches()
    Am, Bm = mat(nt, n, A), mat(nt, n, B)
    C1 = nt.Matrix_ps(n)
    C1.Gemm(Am, Am, None, 1.0, 0.0, 0.0)        # (the first product of the dimension comes back in compressed columns)
    assert nt.last_block_stats()["used"] == 1
    P = nt.Matrix_ps(n)
    P.Gemm(Am, Am, None, 1.0, 0.0, 0.0)         # block form from here on
    M = {"AA": P, "B": Bm}
    form = "block form"

    def on_tiles(fn):
        b0 = nt.block_algebra_counts()
        fn()
        b1 = nt.block_algebra_counts()
        assert b1["operations"] == b0["operations"] + 1 and b1["fallbacks"] == b0["fallbacks"], "%s: the block algebra's counters moved by %s" % (
            form, moved(b1, b0))

    (re, im), _ = want_dot(c, "AA", "B")
    if cplx:
        assert im != 0 and re != 0          # (a flipped or dropped imaginary part shows)
    on_tiles(lambda: check_dot(nt, c, form + ", Dot(block, compressed)", M, "AA", "B"))
    on_tiles(lambda: check_dot(nt, c, form + ", Dot(compressed, block)", M, "B", "AA"))
    on_tiles(lambda: check_singles(nt, c, form, M, "AA", ("trace",)))
    if cplx:
        # (moduli of general Gaussian integers: the real family's bound, with the two roundings of a 1 ulp hypot)
        _EXPECTED[(c["id"], "norm", "AA")] = R.norm_real(AA, n)
    on_tiles(lambda: check_singles(nt, c, form, M, "AA", ("norm",)))
    assert np.array_equal(R.dense(P.triplets(), n), AAd)      # (the block-form operand itself is the exact product)
    print("%s in block form: %.2f s" % (c["id"], time.time() - t0))


# ------------------------------------------------------------------ ranks
# Measured on an MI355X: a run of this worker (all ranks) takes 0.6 s on two ranks and 0.8 s on three, where the worker of
# tests/test_gpu_multirank_vocabulary.py takes 1.2 s and 1.9 s.  The limit is that file's: five times its longest run, which is
# more than ten times the longest of this one
RUN_TIMEOUT = 15


def run_world(world, tmp_path):
    out = str(tmp_path / ("sf%d" % world))
    name = "s%s" % uuid.uuid4().hex[:12]
    assert world <= 3
    procs = []
    t0 = time.time()
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name,
                   NTPOLY_AMD_SHM_MB="16", NTPOLY_AMD_SPGEMM_FMA="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "scalar_forms_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=RUN_TIMEOUT)
            logs.append(o)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        try:
            os.unlink("/dev/shm/ntpoly_amd_" + name)
        except OSError:
            pass
    print("scalar forms run: world %d: %.1f s" % (world, time.time() - t0))
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d of %d failed:\n%s" % (r, world, logs[r][-3000:])
    return [dict(np.load(out + ".%d.npz" % r)) for r in range(world)]


@pytest.mark.parametrize("world", [2, 3])
def test_column_panels_across_ranks(world, tmp_path):
    """the mixed case, both families, as column panels: Trace, Gershgorin, Dot and Norm on every rank against the references of
    the one-rank tests.  Banded operands whose extreme column and missing diagonal lie in a panel with col_offset != 0: Trace,
    Norm and both Gershgorin ends on compressed column panels, and 1 / max |Gershgorin end| from the slab-form panels of a solver
    session (panel_sessions; one-call sessions do not open across ranks, so no vocabulary call sees a slab-form panel)"""
    parts = run_world(world, tmp_path)
    form = "compressed column panels, %d ranks" % world
    for family in ("int", "real"):
        for cplx in (False, True):
            c = R.case("mixed", family, cplx)
            for r in range(world):
                p = parts[r]
                for a, b in c["dots"]:
                    got = p["%s.dot.%s.%s" % (c["id"], a, b)]
                    (re, im), (tre, tim) = want_dot(c, a, b)
                    check("%s Re Dot(%s, %s) rank %d" % (c["id"], a, b, r), form, got[0], re, tre)
                    check("%s Im Dot(%s, %s) rank %d" % (c["id"], a, b, r), form, got[1], im, tim)
                for name in c["singles"]:
                    for what in ("trace", "norm"):
                        v, tol = want_single(c, name, what)
                        check("%s %s(%s) rank %d" % (c["id"], what, name, r), form, float(p["%s.%s.%s" % (c["id"], what, name)][0]), v, tol)
                    (lo, hi), (tl, th) = want_single(c, name, "gershgorin")
                    g = p["%s.gershgorin.%s" % (c["id"], name)]
                    check("%s Gershgorin lower(%s) rank %d" % (c["id"], name, r), form, g[0], lo, tl)
                    check("%s Gershgorin upper(%s) rank %d" % (c["id"], name, r), form, g[1], hi, th)
    form = "slab-form column panels, %d ranks" % world
    for name, (t, ext, gone) in R.panel_operands(world).items():
        lo, hi = R.gershgorin_int(t, R.N_MIXED)
        for r in range(world):
            got = parts[r]["panel.%s.compressed" % name]
            for what, g, w in (("trace", got[0], R.trace_int(t)), ("norm", got[1], R.norm_int(t, R.N_MIXED)), ("Gershgorin lower", got[2], lo),
                               ("Gershgorin upper", got[3], hi)):
                check("panel operand '%s' %s rank %d" % (name, what, r), "compressed column panels, %d ranks" % world, float(g), w, 0.0)
            d = parts[r]["panel.%s.counts" % name]      # products, others, refusals in slab form; panel products in slab form
            assert d[0] >= 1 and d[1] >= 1 and d[2] == 0 and d[3] >= 1, "rank %d: the loop's panels were not in slab form: %s" % (r, d)
            check("panel operand '%s' 1 / max |Gershgorin end| rank %d" % (name, r), form, float(parts[r]["panel.%s.lambda" % name][0]),
                  1.0 / max(abs(lo), abs(hi)), 0.0)
