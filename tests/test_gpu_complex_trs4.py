"""GPU: complex TRS4 in a complex slab session (option complex_trs4; csrc/slab_extra.hip k_sa_trs4<double2, .>, engine.hpp ps_trs4_traces /
ps_trs4_operand / ps_trs4_energy).  Behind its product X X -> X2 an iteration builds, with the vocabulary at threshold 0,
Fx = 4 X - 3 X2 and Gx = I - 2 X + X2, takes dot(X2, Fx) and dot(X2, Gx), and multiplies X2 by Fx + sigma Gx; the fused passes read
the runs of X and X2 twice and never build Fx and Gx, and the energy Re dot(X, WH) comes from one pass over X's runs.

The kernel is reached with crafted operands through nt.trs4_chain_step / nt.trs4_energy and compared with (i) the same chain
spelled with the vocabulary on compressed columns (slab_algebra = 0) and (ii) a numpy restatement written here, componentwise --
never with the fused code itself.  numpy's float64 products and sums are the correctly rounded ones the kernel spells as
__dmul_rn / __dadd_rn, so patterns are compared for equality and values with np.array_equal; the traces, summed in another
order, within the worst-case bound of a reordered sum of rounded terms.  The solver is compared with option 0, with the CPU
oracle in FMA mode on an occupation that takes all three branches of the loop, with the real solve where every imaginary part
is zero, and bit for bit outside the option's gates."""
import math

import numpy as np
import pytest

from gen import banded_triplets, lattice_triplets

pytestmark = pytest.mark.gpu
N = 259   # (not a multiple of the 4 waves of a workgroup)
SIGMAS = (0.5, 3.0, 5.75)   # short binary fractions, which the planted cancellations need
KEYS = ("traces", "operands", "energies", "refused")
NONE = dict(traces=0, operands=0, energies=0, refused=0)
OPTIONS = ("spgemm_fma", "complex_tile", "complex_sessions", "complex_trs4", "slab_algebra", "block_path", "block_complex")


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


def _set_fma(nt):
    nt.set_option("spgemm_fma", 1)   # (set explicitly: the in-process baseline is unfused)
    nt.set_option("complex_tile", 1)
    nt.set_option("complex_sessions", 1)
    nt.set_option("slab_algebra", 1)


@pytest.fixture()
def fma(nt):
    from oracle import oracle_py as O
    keep = {k: nt.get_option(k) for k in OPTIONS}
    _set_fma(nt)
    nt.set_option("complex_trs4", 1)
    O.set_fma(True)
    yield O
    for k, v in keep.items():
        nt.set_option(k, v)
    O.set_fma(False)


def srt(t):
    c, r, v = (np.asarray(x) for x in t)
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def same(a, b):
    """sorted triplets: equal patterns, equal values"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def delta(c1, c0):
    return {k: c1[k] - c0[k] for k in c1}


# ------------------------------------------------------------------ crafted operands
# a column is (rows, complex values)
EMPTY = {"X": {7, 40}, "X2": {8, 40}}   # empty in X, empty in X2, column 40 empty in both
DIAG_ONLY = {13}
BELOW, ABOVE = 60, 150    # columns whose runs lie wholly below / above the diagonal row: the hull must reach the diagonal
NO_DIAG = 110             # a column whose X and X2 have a hole on the diagonal inside their runs
CANCEL, CANCEL_RE, ONE_SIDED = 30, 29, 31   # row 33: fx + sigma gx == 0 in both parts; in the real part only; the same x without an X2 entry
ROW = 33


def _runs(rng, n, empty):
    """{column: (rows, values)}: a run around the diagonal with half-widths 6..90 drawn per side, ~12 % holes inside, real and
    imaginary parts drawn independently, log-uniform in [1e-6, 1] with a random sign each"""
    cols = {}
    for j in range(n):
        if j in empty:
            continue
        if j in DIAG_ONLY:
            rows = np.array([j])
        else:
            if j == BELOW:
                f, l = j + 3, j + int(rng.integers(30, 60))
            elif j == ABOVE:
                f, l = j - int(rng.integers(30, 60)), j - 3
            else:
                f, l = max(0, j - int(rng.integers(6, 91))), min(n - 1, j + int(rng.integers(6, 91)))
            rows = np.arange(f, l + 1)
            keep = rng.random(len(rows)) > 0.12
            keep[0] = keep[-1] = True
            rows = rows[keep]
        part = lambda: 10.0 ** rng.uniform(-6.0, 0.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
        re = part()
        cols[j] = (rows, re + 1j * part())
    return cols


def _set(cols, j, r, v):
    rows, vals = cols[j]
    if v == 0:
        cols[j] = (rows[rows != r], vals[rows != r])   # (no entry: the matrices of the loop store no zeros)
    elif r in rows:
        vals[rows == r] = v
    else:
        k = int(np.searchsorted(rows, r))
        cols[j] = (np.insert(rows, k, r), np.insert(vals, k, v))


def _part(x, x2, d, sigma):
    """one part of an entry through the chain, every operation rounded on its own (DensityMatrixSolversModule.F90:590-627)"""
    fx = 4.0 * x + (-3.0 * x2)
    gx = x2 + ((-2.0 * x) + d)
    return fx, gx, fx + sigma * gx


def _plant(X, X2, sigma):
    """cancellations, exact by construction and checked here: x (4 - 2 sigma) + x2 (sigma - 3) == 0 with x = k (3 - sigma),
    x2 = k (4 - 2 sigma) -- at sigma = 3 that x is zero, no entry"""
    k = 0.25
    x, x2 = k * (3.0 - sigma), k * (4.0 - 2.0 * sigma)
    assert _part(x, x2, 0.0, sigma)[2] == 0.0 and x2 != 0.0
    xi, x2i = 0.3125, 0.1875   # an imaginary part that does not cancel
    assert _part(xi, x2i, 0.0, sigma)[2] != 0.0
    _set(X, CANCEL, ROW, complex(x, 2.0 * x))
    _set(X2, CANCEL, ROW, complex(x2, 2.0 * x2))
    _set(X, CANCEL_RE, ROW, complex(x, xi))
    _set(X2, CANCEL_RE, ROW, complex(x2, x2i))
    _set(X, ONE_SIDED, ROW, complex(x, 2.0 * x))
    _set(X2, ONE_SIDED, ROW, 0)
    for M in (X, X2):
        _set(M, NO_DIAG, NO_DIAG, 0)


@pytest.fixture(scope="module")
def operands():
    out = {}
    for sigma in SIGMAS:
        rng = np.random.default_rng(20261019)
        X, X2 = (_runs(rng, N, EMPTY[k]) for k in ("X", "X2"))
        _plant(X, X2, sigma)
        out[sigma] = (X, X2)
    return out


def _triplets(cols, real=False):
    c, r, v = [], [], []
    for j in sorted(cols):
        rows, vals = cols[j]
        c.append(np.full(len(rows), j + 1))
        r.append(rows + 1)
        v.append(vals.real.copy() if real else vals)
    if not c:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64 if real else np.complex128)
    return np.concatenate(c).astype(np.int32), np.concatenate(r).astype(np.int32), np.concatenate(v)


def _matrix(nt, cols, n=N, real=False):
    c, r, v = _triplets(cols, real)
    M = nt.Matrix_ps.from_triplets(n, c, r, v)
    assert len(M.triplets()[2]) == len(v)
    return M


def _dense(cols, j, n=N):
    v = np.zeros(n, dtype=np.complex128)
    if j in cols:
        v[cols[j][0]] = cols[j][1]
    return v


def restated(X, X2, sigma, n=N):
    """P column by column and the terms of the two traces: an absent entry enters as (0, 0), the identity adds (1, 0) on the
    diagonal row, an entry of P exists where either part is not zero"""
    P, tf, tg = {}, [], []
    for j in range(n):
        x, x2 = _dense(X, j, n), _dense(X2, j, n)
        d = np.zeros(n)
        d[j] = 1.0
        fr, gr, pr = _part(x.real, x2.real, d, sigma)
        fi, gi, pi = _part(x.imag, x2.imag, np.zeros(n), sigma)
        rows = np.nonzero((pr != 0.0) | (pi != 0.0))[0]
        if len(rows):
            P[j] = (rows, pr[rows] + 1j * pi[rows])
        has = np.nonzero(x2 != 0.0)[0]
        tf += [x2.real[has] * fr[has], x2.imag[has] * fi[has]]
        tg += [x2.real[has] * gr[has], x2.imag[has] * gi[has]]
    return P, np.concatenate(tf), np.concatenate(tg)


@pytest.fixture(scope="module")
def references(operands):
    return {sigma: restated(*operands[sigma], sigma) for sigma in SIGMAS}


def _sum_bound(terms):
    """any summation order of m rounded terms is within m 2^-52 sum |t| of their exact sum (u = 2^-53 per addition, the pair
    sums x2.re f.re + x2.im f.im inside an entry included, with room for the second-order part): a derived bound"""
    return math.fsum(terms), len(terms) * 2.0 ** -52 * math.fsum(np.abs(terms))


def test_the_inputs_reach_every_branch(operands, references):
    """from the operands and the numpy restatement alone"""
    for sigma in SIGMAS:
        X, X2 = operands[sigma]
        P, tf, tg = references[sigma]
        assert 7 not in X and 7 in X2 and 8 not in X2 and 8 in X and 40 not in X and 40 not in X2
        for M in (X, X2):
            assert 0 in M and N - 1 in M and M[BELOW][0][0] > BELOW and M[ABOVE][0][-1] < ABOVE and list(M[13][0]) == [13]
            assert NO_DIAG not in M[NO_DIAG][0] and M[NO_DIAG][0][0] < NO_DIAG < M[NO_DIAG][0][-1]
            assert np.all(M[5][1].real != 0.0) and np.all(M[5][1].imag != 0.0) and not np.array_equal(M[5][1].real, M[5][1].imag)
        # the identity alone where both are empty; the diagonal joins the hull of runs that do not hold it
        assert list(P[40][0]) == [40] and P[40][1][0] == sigma
        for j in (BELOW, ABOVE, NO_DIAG):
            assert P[j][1][P[j][0] == j][0] == sigma
        assert P[BELOW][0][0] == BELOW and P[ABOVE][0][-1] == ABOVE
        # the cancellations
        assert ROW in X2[CANCEL][0] and ROW not in P[CANCEL][0] and P[CANCEL][0][0] < ROW < P[CANCEL][0][-1]
        v = P[CANCEL_RE][1][P[CANCEL_RE][0] == ROW]
        assert len(v) == 1 and v[0].real == 0.0 and v[0].imag != 0.0
        assert ROW not in X2[ONE_SIDED][0]
        if sigma != 3.0:
            assert ROW in X[CANCEL][0] and ROW in X[ONE_SIDED][0] and P[ONE_SIDED][1][P[ONE_SIDED][0] == ROW][0] != 0.0
        assert len(tf) == len(tg) > 2000


def _vocabulary(nt, MX, MX2, sigma):
    """the calls of solvers.cpp solver_trs4 behind its first product, through the C ABI"""
    Fx = nt.Matrix_ps(MX2)
    Fx.Scale(-3.0)
    Fx.Increment(MX, 4.0, 0.0)
    Gx = nt.Matrix_ps(N)
    Gx.FillIdentity()
    Gx.Increment(MX, -2.0, 0.0)
    Gx.Increment(MX2, 1.0, 0.0)
    tf, tg = MX2.Dot(Fx), MX2.Dot(Gx)
    Gx.Scale(sigma)
    Gx.Increment(Fx, 1.0, 0.0)
    return Gx, tf, tg


@pytest.mark.parametrize("sigma", SIGMAS)
def test_chain_bit_for_bit(nt, fma, operands, references, sigma):
    X, X2 = operands[sigma]
    P, tf, tg = references[sigma]
    want = srt(_triplets(P))
    MX, MX2 = _matrix(nt, X), _matrix(nt, X2)
    before = [srt(m.triplets()) for m in (MX, MX2)]
    # (i) the vocabulary on compressed columns against (ii) the restatement
    nt.set_option("slab_algebra", 0)
    V, vf, vg = _vocabulary(nt, MX, MX2, sigma)
    nt.set_option("slab_algebra", 1)
    assert same(srt(V.triplets()), want), "compressed columns against the restatement"
    O = nt.Matrix_ps(N)
    c0, s0 = nt.complex_trs4_counts(), nt.slab_algebra_counts()
    with nt.solver_session():
        got = nt.trs4_chain_step(MX, MX2, sigma, O)
    c1, s1 = nt.complex_trs4_counts(), nt.slab_algebra_counts()
    print(sigma, "counts", c0, c1, "slab algebra", s0, s1)
    assert got is not None
    assert delta(c1, c0) == dict(traces=1, operands=1, energies=0, refused=0)
    assert s1["merges"] - s0["merges"] == 1 and s1["others"] - s0["others"] == 1 and s1["refusals"] == s0["refusals"]
    for m, bf in zip((MX, MX2), before):
        assert same(srt(m.triplets()), bf), "the operands are as they were"
    g = srt(O.triplets())
    print(sigma, "entries", len(want[2]))
    assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]), "pattern"
    assert same(g, want), "values against the restatement"
    assert same(g, srt(V.triplets())), "values against compressed columns"
    for name, t, terms, v in (("fx", got[0], tf, vf), ("gx", got[1], tg, vg)):
        exact, bound = _sum_bound(terms)
        print(sigma, "trace", name, t, "exact", exact, "|difference|", abs(t - exact), "bound", bound, "compressed columns", v)
        assert abs(t - exact) <= bound
        assert abs(complex(v).real - exact) <= bound


def test_sigma_zero_is_declined_without_a_refusal(nt, fma, operands):
    X, X2 = operands[SIGMAS[0]]
    MX, MX2, O = _matrix(nt, X), _matrix(nt, X2), nt.Matrix_ps(N)
    c0 = nt.complex_trs4_counts()
    with nt.solver_session():
        got = nt.trs4_chain_step(MX, MX2, 0.0, O)
    assert got is None and nt.complex_trs4_counts() == c0
    assert len(O.triplets()[2]) == 0


def test_gates_of_the_diagnostic(nt, fma, operands):
    """the option at 0 and a session that does not take complex operands: declined, nothing counted"""
    X, X2 = operands[SIGMAS[0]]
    MX, MX2, O = _matrix(nt, X), _matrix(nt, X2), nt.Matrix_ps(N)
    c0 = nt.complex_trs4_counts()
    nt.set_option("complex_trs4", 0)
    with nt.solver_session():
        assert nt.trs4_chain_step(MX, MX2, 0.5, O) is None and nt.trs4_energy(MX, MX2) is None
    nt.set_option("complex_trs4", 1)
    with nt.solver_session(False):
        assert nt.trs4_chain_step(MX, MX2, 0.5, O) is None and nt.trs4_energy(MX, MX2) is None
    assert nt.complex_trs4_counts() == c0


def test_zero_imaginary_parts_give_the_real_kernel(nt, fma, operands):
    """the same entry point on real matrices runs the real kernel: its P bit for bit in the real parts, every imaginary part 0"""
    sigma = SIGMAS[2]
    X, X2 = operands[sigma]
    Xr = {j: (rows, vals.real + 0j) for j, (rows, vals) in X.items()}
    X2r = {j: (rows, vals.real + 0j) for j, (rows, vals) in X2.items()}
    Oc, Or = nt.Matrix_ps(N), nt.Matrix_ps(N)
    c0 = nt.complex_trs4_counts()
    with nt.solver_session():
        gc = nt.trs4_chain_step(_matrix(nt, Xr), _matrix(nt, X2r), sigma, Oc)
        c1 = nt.complex_trs4_counts()
        gr = nt.trs4_chain_step(_matrix(nt, Xr, real=True), _matrix(nt, X2r, real=True), sigma, Or)
    assert gc is not None and gr is not None
    assert delta(c1, c0) == dict(traces=1, operands=1, energies=0, refused=0)
    assert nt.complex_trs4_counts() == c1, "real operands never count"
    assert Oc.IsComplex() and not Or.IsComplex()
    c, r = srt(Oc.triplets()), srt(Or.triplets())
    assert np.array_equal(c[0], r[0]) and np.array_equal(c[1], r[1]), "pattern"
    assert np.array_equal(c[2].real, r[2]) and np.all(c[2].imag == 0.0)
    assert len(r[2]) > 1000


def test_refusal_leaves_everything_as_it_was(nt, fma):
    """every column: X's run in rows 0-5, X2's in rows 250-255 -- the hulls (256 rows and more per column) exceed the output's bound
    (the operands' slots and four alignments per column)"""
    rng = np.random.default_rng(7)
    val = lambda: rng.uniform(0.1, 0.9, 6) + 1j * rng.uniform(0.1, 0.9, 6)
    X = {j: (np.arange(0, 6), val()) for j in range(N)}
    X2 = {j: (np.arange(250, 256), val()) for j in range(N)}
    MX, MX2, O = _matrix(nt, X), _matrix(nt, X2), nt.Matrix_ps(N)
    before = [srt(m.triplets()) for m in (MX, MX2)]
    c0, s0 = nt.complex_trs4_counts(), nt.slab_algebra_counts()
    with nt.solver_session():
        got = nt.trs4_chain_step(MX, MX2, 0.5, O)
    c1, s1 = nt.complex_trs4_counts(), nt.slab_algebra_counts()
    assert got is None
    assert c1 == dict(c0, refused=c0["refused"] + 1), (c0, c1)
    assert s1 == s0, (s0, s1)   # (a refused pass is no operation and no refusal of the session)
    for m, bf in zip((MX, MX2), before):
        assert same(srt(m.triplets()), bf)
    assert len(O.triplets()[2]) == 0


def _dot_terms(X, W):
    t = []
    for j in X:
        if j in W:
            both = np.intersect1d(X[j][0], W[j][0])
            x, w = X[j][1][np.isin(X[j][0], both)], W[j][1][np.isin(W[j][0], both)]
            t += [x.real * w.real, x.imag * w.imag]
    return np.concatenate(t)


def test_energy_pass(nt, fma, operands):
    """Re sum conj(X) WH for a WH in slab form, in compressed columns, and one that stores a zero"""
    X, W = operands[SIGMAS[0]]
    Wz = {j: (rows.copy(), vals.copy()) for j, (rows, vals) in W.items()}
    shared = np.intersect1d(X[ONE_SIDED][0], W[ONE_SIDED][0])
    Wz[ONE_SIDED][1][Wz[ONE_SIDED][0] == shared[len(shared) // 2]] = 0.0   # (a stored zero inside a run, on a row X holds too)
    exact, bound = _sum_bound(_dot_terms(X, W))
    exact_z, bound_z = _sum_bound(_dot_terms(X, Wz))
    assert exact_z != exact
    MX, MW, MWs, MWz, O = _matrix(nt, X), _matrix(nt, W), _matrix(nt, W), _matrix(nt, Wz), nt.Matrix_ps(N)
    assert np.any(MWz.triplets()[2] == 0.0)
    c0 = nt.complex_trs4_counts()
    with nt.solver_session():
        e_cols = nt.trs4_energy(MX, MW)
        assert nt.trs4_chain_step(MWs, MX, 0.5, O) is not None   # (leaves MWs in complex slab form)
        c1 = nt.complex_trs4_counts()
        e_slab = nt.trs4_energy(MX, MWs)
        e_zero = nt.trs4_energy(MX, MWz)
    c2 = nt.complex_trs4_counts()
    print("energy", e_cols, e_slab, e_zero, "exact", exact, exact_z, "bound", bound, "terms", len(_dot_terms(X, W)))
    assert delta(c1, c0) == dict(traces=1, operands=1, energies=1, refused=0) and delta(c2, c1) == dict(NONE, energies=2)
    assert abs(e_cols - exact) <= bound and abs(e_slab - exact) <= bound and abs(e_zero - exact_z) <= bound_z
    assert abs(complex(MX.Dot(MW)).real - exact) <= bound
    assert same(srt(MWz.triplets()), srt(_triplets(Wz)))


# ------------------------------------------------------------------ the solver
SOLVE = (1536, 16, 1e-7, 10)


def close(got, want, n, thr, what, rel=1e-10):
    """the rule of tests/test_gpu_complex_density.py: larger differences only at the threshold, entry counts nearly equal"""
    import scipy.sparse as sp
    G = sp.csr_matrix((got[2], (got[1] - 1, got[0] - 1)), shape=(n, n))
    W = sp.csr_matrix((want[2], (want[1] - 1, want[0] - 1)), shape=(n, n))
    scale = max(1.0, np.abs(want[2]).max())
    D = (G - W).tocoo()
    bad = np.abs(D.data) > rel * scale
    print(what, "max |difference|", np.abs(D.data).max() if D.nnz else 0.0, "beyond", rel * scale, ":", int(bad.sum()), "entries", G.nnz, W.nnz)
    assert np.all(np.abs(D.data[bad]) <= thr * (1 + 1e-9) + rel * scale), "%s: max |d| = %g" % (what, np.abs(D.data).max())
    assert abs(G.nnz - W.nnz) <= max(8, 1e-5 * W.nnz), "%s: %d vs %d entries" % (what, G.nnz, W.nnz)


def trs4(nt, n, trip, opt, nel, iters=SOLVE[3], thr=SOLVE[2]):
    nt.set_option("complex_trs4", opt)
    Hm = nt.Matrix_ps.from_triplets(n, *trip)
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    p = nt.SolverParameters()
    p.SetThreshold(thr)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(iters)
    p.SetMonitorConvergence(False)
    K = nt.Matrix_ps(n)
    c0, b0, s0 = nt.complex_trs4_counts(), nt.block_algebra_counts(), nt.slab_algebra_counts()
    energy, mu = nt.DensityMatrixSolvers.TRS4(Hm, I, nel, K, p)
    c1, b1, s1 = nt.complex_trs4_counts(), nt.block_algebra_counts(), nt.slab_algebra_counts()
    tr = nt.solver_trace()
    return dict(K=srt(K.triplets()), energy=energy, mu=mu, it=tr["iterations"], sigma=np.asarray(tr["sigma"]).copy(),
                e=np.asarray(tr["energy"]).copy(), nnz=np.asarray(tr["nnz"]).copy(), counts=delta(c1, c0), block=delta(b1, b0), slab=delta(s1, s0))


def agree(a, b, n, thr, what):
    """the numbers the real TRS4 session is held to (tests/test_gpu_slab_algebra.py)"""
    print(what, "iterations", a["it"], b["it"], "max |d sigma|", float(np.max(np.abs(a["sigma"] - b["sigma"]))), "max relative energy difference",
          float(np.max(np.abs(a["e"] - b["e"]) / np.abs(b["e"]))), "entry counts equal", bool(np.array_equal(a["nnz"], b["nnz"])))
    assert a["it"] == b["it"]
    assert np.allclose(a["sigma"], b["sigma"], rtol=1e-6, atol=1e-8)
    assert np.allclose(a["e"], b["e"], rtol=1e-10, atol=0.0)
    assert abs(a["energy"] - b["energy"]) <= 1e-10 * abs(b["energy"])
    close(a["K"], b["K"], n, thr, what)


def fused_counts_ok(r):
    mid = int(np.sum((r["sigma"] >= 0.0) & (r["sigma"] <= 6.0)))
    c = r["counts"]
    assert c["traces"] >= r["it"] - 1 and c["energies"] >= r["it"] - 1 and c["operands"] >= mid - 1 and c["refused"] <= 1, (c, mid)


@pytest.fixture(scope="module")
def banded():
    return banded_triplets(SOLVE[0], SOLVE[1], complex_=True)


def test_solver_option_1_against_option_0(nt, fma, banded):
    n = SOLVE[0]
    on = trs4(nt, n, banded, 1, n / 2.0)
    off = trs4(nt, n, banded, 0, n / 2.0)
    print("counts", on["counts"], "slab algebra", on["slab"], off["slab"], "sigma", on["sigma"].tolist())
    assert on["it"] == SOLVE[3]
    agree(on, off, n, SOLVE[2], "density, option 1 against option 0")
    fused_counts_ok(on)
    assert on["slab"]["products"] >= on["it"] - 1, "the loop's products ran in complex slab form"
    assert off["counts"] == NONE


def test_all_three_branches_against_the_oracle(nt, fma, banded):
    O = fma
    n, h, thr, iters = SOLVE
    nel = 0.1 * n
    Ho = O.Mat.from_triplets(n, n, *banded)
    po = O.params(converge_diff=1e-30, threshold=thr, max_iterations=iters, monitor_convergence=False)
    Ko, e_o, mu_o, tro = O.density("trs4", Ho, O.Mat.identity(n), nel, po)
    so, eo = np.asarray(tro["sigma"]), np.asarray(tro["energy"])
    cls = lambda s: np.where(s < 0.0, -1, np.where(s > 6.0, 1, 0))
    print("oracle sigma", so.tolist())
    assert set(cls(so).tolist()) == {-1, 0, 1}, "the oracle's run takes all three branches"
    on = trs4(nt, n, banded, 1, nel)
    print("engine sigma", on["sigma"].tolist(), "counts", on["counts"])
    print("max |d sigma|", float(np.max(np.abs(on["sigma"] - so))), "max relative energy difference", float(np.max(np.abs(on["e"] - eo) / np.abs(eo))))
    assert on["it"] == tro["iterations"] == iters
    assert np.array_equal(cls(on["sigma"]), cls(so)), "the same branch in every iteration"
    assert np.allclose(on["e"], eo, rtol=1e-10, atol=0.0)
    assert np.allclose(on["sigma"], so, rtol=1e-6, atol=1e-8)
    assert abs(on["energy"] - e_o) <= 1e-10 * abs(e_o)
    import scipy.sparse as sp
    w = srt(Ko.triplets())
    G = sp.csr_matrix((on["K"][2], (on["K"][1] - 1, on["K"][0] - 1)), shape=(n, n))
    W = sp.csr_matrix((w[2], (w[1] - 1, w[0] - 1)), shape=(n, n))
    print("max |K - oracle|", abs(G - W).max())
    assert abs(G - W).max() <= 1e-6
    fused_counts_ok(on)


def test_zero_imaginary_parts(nt, fma):
    """a real H stored as complex: the real solve's iterations, sigma and energies; every imaginary part of K exactly zero"""
    n, h, thr, iters = SOLVE
    c, r, v = banded_triplets(n, h)
    cplx = trs4(nt, n, (c, r, v.astype(np.complex128)), 1, n / 2.0)
    real = trs4(nt, n, (c, r, v), 1, n / 2.0)
    print("sigma", cplx["sigma"].tolist(), real["sigma"].tolist())
    assert cplx["it"] == real["it"] == iters
    assert np.allclose(cplx["sigma"], real["sigma"], rtol=1e-6, atol=1e-8)
    assert np.allclose(cplx["e"], real["e"], rtol=1e-10, atol=0.0)
    assert np.iscomplexobj(cplx["K"][2]) and np.all(np.imag(cplx["K"][2]) == 0.0)
    fused_counts_ok(cplx)
    assert real["counts"] == NONE   # (real operands never count)


def bit_equal(a, b):
    return (a["it"] == b["it"] and list(a["e"]) == list(b["e"]) and list(a["sigma"]) == list(b["sigma"]) and a["energy"] == b["energy"] and
            all(np.array_equal(x, y) for x, y in zip(a["K"], b["K"])))


@pytest.mark.parametrize("which", ["spgemm_fma", "complex_tile", "complex_sessions"])
def test_outside_the_gates_bit_for_bit(nt, fma, banded, which):
    n = SOLVE[0]
    nt.set_option(which, 0)
    a = trs4(nt, n, banded, 1, n / 2.0, iters=6)
    b = trs4(nt, n, banded, 0, n / 2.0, iters=6)
    assert a["counts"] == NONE == b["counts"]
    assert bit_equal(a, b)


def test_a_real_operand_is_untouched(nt, fma):
    n, h = SOLVE[0], SOLVE[1]
    trip = banded_triplets(n, h)
    a = trs4(nt, n, trip, 1, n / 2.0, iters=6)
    b = trs4(nt, n, trip, 0, n / 2.0, iters=6)
    assert a["counts"] == NONE == b["counts"]
    assert bit_equal(a, b)


def hermitian(trip, phase=0.1):
    """a Hermitian complex operand with the pattern and |values| of a real symmetric one: H(r, c) = v exp(i phase (r - c))"""
    c, r, v = trip
    return c, r, v * np.exp(1j * phase * (r.astype(np.float64) - c.astype(np.float64)))


def test_a_complex_lattice_stays_in_block_form(nt, fma):
    """an operand without runs: inside the complex session the products leave complex block form and the loop's vocabulary calls
    take the block algebra; the fused passes leave block form alone (a gate)"""
    L = 12
    n = L ** 3
    trip = hermitian(lattice_triplets(L))
    nt.set_option("block_path", 2)
    nt.set_option("block_complex", 1)
    on = trs4(nt, n, trip, 1, n / 2.0, thr=SOLVE[2])
    off = trs4(nt, n, trip, 0, n / 2.0, thr=SOLVE[2])
    print("block algebra", on["block"], off["block"], "fallbacks", on["block"]["fallbacks"], "counts", on["counts"], "slab algebra", on["slab"])
    agree(on, off, n, SOLVE[2], "lattice density, option 1 against option 0")
    assert on["block"]["operations"] >= on["it"] - 1
    assert on["counts"]["traces"] == 0 and on["counts"]["operands"] == 0 and on["counts"]["energies"] == 0, on["counts"]
