"""GPU: complex ScaleAndFold in a complex slab session (option complex_scale_fold; csrc/slab_extra.hip k_saf_update<double2, .> and
k_sa_dot_trace_c, engine.hpp ps_saf_update / ps_saf_dot_trace).  Behind its one product X X -> X2 an iteration of the fold branch
calls, with the vocabulary at threshold 0, X *= 2 alpha; X += (-alpha^2) X2; energy = 2 Re dot(X, WH), and the next iteration begins
with trace(X).  The fused update reads the runs of X, X2 and WH once, writes the new X and returns both sums; in the scale branch,
whose product's result is the new X, one pass over X and WH returns them.

The kernels are reached with crafted operands through nt.scale_fold_update_step / nt.scale_fold_dot_trace and compared with (i) the
same calls spelled with the vocabulary on compressed columns (slab_algebra = 0) and (ii) a numpy restatement written here, part by
part -- never with the fused code itself.  numpy's float64 products and sums are the correctly rounded ones the kernel spells as
__dmul_rn / __dadd_rn, so patterns are compared for equality and values with np.array_equal; the energy, summed in another order,
within the worst-case bound of a reordered sum of rounded terms.

The trace.  It decides the next branch, so the update's trace is held to the bits of MatrixTrace of the new X: MatrixTrace_ps_wrp
through the C ABI, called inside the session on the new X in slab form.  With the option on, MatrixTrace of a complex slab-form
matrix in a complex session is the pass over its runs (psmatrix.cpp trace_local -> slab_dot_trace_c), whose sum over the columns
is the one the fused passes make -- so every trace(X) the loop takes of an X in slab form, fused or behind a refused pass, has the
same bits.  MatrixTrace of a matrix in compressed columns (k_trace: outside a session, or with the option at 0) sums the same real
parts in another fixed order; it is held to the bound of a reordered sum.

The solver is compared with option 0, with a dense numpy restatement of the loop, and bit for bit outside the option's gates.
The solver's trace record holds no trace(X), so the margin between trace(X) and the electron count is taken from the dense
restatement of the option-0 loop, whose branch sequence is asserted to be the one option 0 took."""
import math

import numpy as np
import pytest

from gen import banded_triplets, lattice_triplets

pytestmark = pytest.mark.gpu
N = 259   # (not a multiple of the 4 waves of a workgroup)
ALPHAS = (0.75, 1.25)   # 2 alpha and alpha^2 are short binary fractions, which the planted cancellations need
NONE = dict(updates=0, dot_traces=0, refused=0)
OPTIONS = ("spgemm_fma", "complex_tile", "complex_sessions", "complex_scale_fold", "scale_fold_step", "slab_algebra", "block_path",
           "block_complex")
TRIP = 2 * 64   # rows one trip of the complex update's chunk loop covers (SAF_KC_C = 2 chunks of 64 rows)


def factors(alpha):
    """(a, b) as solvers.cpp rounds them"""
    return -1.0 * alpha * alpha, 2 * alpha


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture()
def fma(nt):
    keep = {k: nt.get_option(k) for k in OPTIONS}
    nt.set_option("spgemm_fma", 1)   # (set explicitly: the in-process baseline is unfused)
    nt.set_option("complex_tile", 1)
    nt.set_option("complex_sessions", 1)
    nt.set_option("slab_algebra", 1)
    nt.set_option("complex_scale_fold", 1)
    yield
    for k, v in keep.items():
        nt.set_option(k, v)


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
EMPTY = {"X": {7, 40}, "X2": {8, 40}, "WH": {11}}   # empty in each operand in turn, column 40 in X and X2
DIAG_ONLY = {13}
BELOW, ABOVE = 60, 150    # columns whose runs lie wholly below / above the diagonal row in every operand
NO_DIAG = 110             # a column whose X and X2 have a hole on the diagonal inside their runs
LONG = 129                # a column whose X spans rows 1 .. 257: three trips of the chunk loop
CANCEL, CANCEL_RE, ONLY_X2 = 30, 29, 31   # see _plant
ROW = 33
FAR = 200                 # the column of the refusal test


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


def _part(x, x2, alpha):
    """one part of an entry through the two calls, every operation rounded on its own (DensityMatrixSolversModule.F90:1066-1068):
    ScaleMatrix(X, 2 alpha), then IncrementMatrix(X2, X, -alpha^2); an absent entry enters as 0"""
    a, b = factors(alpha)
    return b * x + a * x2


def _plant(X, X2, alpha):
    """cancellations, exact by construction and checked here from the numpy values alone"""
    y, yi = 0.75, 0.625            # x2's parts
    w, wi = alpha * y / 2.0, alpha * yi / 2.0   # x's parts: (2 alpha) w == alpha^2 y exactly for these alpha
    assert _part(w, y, alpha) == 0.0 and _part(wi, yi, alpha) == 0.0 and w != 0.0 and wi != 0.0
    ai, bi = 0.3125, 0.4375        # an imaginary part that does not cancel
    assert _part(ai, bi, alpha) != 0.0
    # both parts cancel: no entry of the new X
    _set(X, CANCEL, ROW, complex(w, wi))
    _set(X2, CANCEL, ROW, complex(y, yi))
    # the real part alone cancels: the entry is kept
    _set(X, CANCEL_RE, ROW, complex(w, ai))
    _set(X2, CANCEL_RE, ROW, complex(y, bi))
    # an entry present only in X2: o = (-alpha^2) x2
    _set(X, ONLY_X2, ROW, 0)
    _set(X2, ONLY_X2, ROW, complex(y, yi))
    for M in (X, X2):
        _set(M, NO_DIAG, NO_DIAG, 0)


@pytest.fixture(scope="module")
def operands():
    out = {}
    for alpha in ALPHAS:
        rng = np.random.default_rng(20261020)
        X, X2, WH = (_runs(rng, N, EMPTY[k]) for k in ("X", "X2", "WH"))
        rows = np.arange(1, 258)
        X[LONG] = (rows, 10.0 ** rng.uniform(-6.0, 0.0, len(rows)) + 1j * 10.0 ** rng.uniform(-6.0, 0.0, len(rows)))
        _plant(X, X2, alpha)
        out[alpha] = (X, X2, WH)
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


def restated(X, X2, WH, alpha, n=N):
    """the new X column by column, the terms of Re dot(X, WH) and the real parts of the new diagonal: an absent entry enters as
    (0, 0), an entry exists where either part is not zero; a stored zero of WH adds no term"""
    new, terms, diag = {}, [], np.zeros(n)
    for j in range(n):
        x, x2, w = (_dense(M, j, n) for M in (X, X2, WH))
        o_re, o_im = _part(x.real, x2.real, alpha), _part(x.imag, x2.imag, alpha)
        rows = np.nonzero((o_re != 0.0) | (o_im != 0.0))[0]
        if len(rows):
            new[j] = (rows, o_re[rows] + 1j * o_im[rows])
        has = rows[w[rows] != 0.0]
        terms += [o_re[has] * w.real[has], o_im[has] * w.imag[has]]
        diag[j] = o_re[j]
    return new, np.concatenate(terms), diag


@pytest.fixture(scope="module")
def references(operands):
    return {alpha: restated(*operands[alpha], alpha) for alpha in ALPHAS}


def _sum_bound(terms):
    """any summation order of m rounded terms is within m 2^-52 sum |t| of their exact sum (u = 2^-53 per addition, the pair sums
    o.re wh.re + o.im wh.im inside an entry included, with room for the second-order part): a derived bound"""
    return math.fsum(terms), len(terms) * 2.0 ** -52 * math.fsum(np.abs(terms))


def _hull(cols_list, j):
    rows = [M[j][0] for M in cols_list if j in M]
    if not rows:
        return 0, 0
    rows = np.concatenate(rows)
    return rows.min() // 16 * 16, (rows.max() // 16 + 1) * 16


def test_the_inputs_reach_every_branch(operands, references):
    """from the operands and the numpy restatement alone"""
    for alpha in ALPHAS:
        X, X2, WH = operands[alpha]
        new, terms, diag = references[alpha]
        a, b = factors(alpha)
        assert 7 not in X and 7 in X2 and 8 not in X2 and 8 in X and 40 not in X and 40 not in X2 and 40 in WH and 11 not in WH
        assert 11 in X and 11 in X2
        for M in (X, X2):
            assert 0 in M and N - 1 in M and M[BELOW][0][0] > BELOW and M[ABOVE][0][-1] < ABOVE and list(M[13][0]) == [13]
            assert NO_DIAG not in M[NO_DIAG][0] and M[NO_DIAG][0][0] < NO_DIAG < M[NO_DIAG][0][-1]
            assert np.all(M[5][1].real != 0.0) and np.all(M[5][1].imag != 0.0) and not np.array_equal(M[5][1].real, M[5][1].imag)
        # trips of the chunk loop: one, two and three
        spans = [hi - lo for lo, hi in (_hull((X, X2), j) for j in range(N))]
        assert spans[40] == 0 and 0 < min(s for s in spans if s) <= TRIP and any(TRIP < s <= 2 * TRIP for s in spans)
        assert X[LONG][0][0] == 1 and X[LONG][0][-1] == 257 and spans[LONG] > 2 * TRIP
        # no column of these operands is refused: the hull is bounded by the two aligned slots and the pads between them
        for j in range(N):
            own = sum((M[j][0][-1] // 16 + 1) * 16 - M[j][0][0] // 16 * 16 for M in (X, X2) if j in M)
            assert spans[j] <= own + 2 * 16
        # columns empty in both give an empty column; the diagonal is absent where no run holds it
        assert 40 not in new and all(diag[j] == 0.0 for j in (40, BELOW, ABOVE, NO_DIAG)) and diag[13] != 0.0 and diag[N - 1] != 0.0
        for j in (BELOW, ABOVE, NO_DIAG):
            assert j not in new[j][0]
        assert list(new[13][0]) == [13]
        # one-sided columns: the scaled X alone, and (-alpha^2) X2 alone
        assert np.array_equal(new[8][0], X[8][0]) and np.array_equal(new[8][1].real, b * X[8][1].real)
        assert np.array_equal(new[7][0], X2[7][0]) and np.array_equal(new[7][1].imag, a * X2[7][1].imag)
        # the cancellations
        assert all(ROW in M[c][0] for M in (X, X2) for c in (CANCEL, CANCEL_RE))
        assert ROW not in new[CANCEL][0] and new[CANCEL][0][0] < ROW < new[CANCEL][0][-1]
        v = new[CANCEL_RE][1][new[CANCEL_RE][0] == ROW]
        assert len(v) == 1 and v[0].real == 0.0 and v[0].imag != 0.0
        assert ROW not in X[ONLY_X2][0] and ROW in X2[ONLY_X2][0] and X[ONLY_X2][0][0] < ROW < X[ONLY_X2][0][-1]
        x2v = X2[ONLY_X2][1][X2[ONLY_X2][0] == ROW][0]
        assert new[ONLY_X2][1][new[ONLY_X2][0] == ROW][0] == complex(a * x2v.real, a * x2v.imag)
        # no scaled entry underflows, no stored zero anywhere
        for M in (X, X2, WH):
            assert all(np.all((v.real != 0.0) | (v.imag != 0.0)) for _, v in M.values())
        assert all(np.all(np.abs(b * v.real) > 1e-300) and np.all(np.abs(a * v.imag) > 1e-300) for M in (X, X2) for _, v in M.values())
        assert len(terms) > 2000


def _vocabulary(nt, MX, MX2, MW, alpha):
    """the calls of solvers.cpp solver_scale_and_fold behind its product, through the C ABI on compressed columns"""
    a, b = factors(alpha)
    V = nt.Matrix_ps(MX)
    V.Scale(b)
    V.Increment(MX2, a, 0.0)
    return V, complex(V.Dot(MW)).real, V.Trace()


@pytest.mark.parametrize("alpha", ALPHAS)
def test_update_bit_for_bit(nt, fma, operands, references, alpha):
    X, X2, WH = operands[alpha]
    new, terms, diag = references[alpha]
    a, b = factors(alpha)
    want = srt(_triplets(new))
    Ms = [_matrix(nt, c) for c in (X, X2, WH)]
    before = [srt(m.triplets()) for m in Ms]
    # (i) the vocabulary on compressed columns against (ii) the restatement
    nt.set_option("slab_algebra", 0)
    V, ev, tv = _vocabulary(nt, *Ms, alpha)
    nt.set_option("slab_algebra", 1)
    assert same(srt(V.triplets()), want), "compressed columns against the restatement"
    # the fused update; then, in the same session, MatrixTrace through the C ABI of the restated new X in slab form (the scale
    # branch's pass brings it there)
    O, Mn = nt.Matrix_ps(N), _matrix(nt, new)
    c0, r0, s0 = nt.complex_scale_fold_counts(), nt.scale_fold_step_counts(), nt.slab_algebra_counts()
    with nt.solver_session():
        got = nt.scale_fold_update_step(Ms[0], Ms[1], a, b, Ms[2], O)
        c1, s1 = nt.complex_scale_fold_counts(), nt.slab_algebra_counts()
        in_slab_form = nt.scale_fold_dot_trace(Mn, Ms[2])
        c2, s2 = nt.complex_scale_fold_counts(), nt.slab_algebra_counts()
        ts = Mn.Trace()
        s3 = nt.slab_algebra_counts()
    print(alpha, "counts", c0, c1, c2, "slab algebra", s0, s1, s2, s3)
    assert got is not None and in_slab_form is not None
    e, t = got
    assert delta(c1, c0) == dict(updates=1, dot_traces=0, refused=0) and delta(c2, c1) == dict(updates=0, dot_traces=1, refused=0)
    assert s3["others"] - s2["others"] == 1 and s3["refusals"] == s0["refusals"], "MatrixTrace was taken in slab form"
    assert nt.scale_fold_step_counts() == r0, "the real loop's counters never count a complex pass"
    assert s1["merges"] - s0["merges"] == 1 and s1["others"] - s0["others"] == 2 and s1["refusals"] == s0["refusals"]
    for m, bf in zip(Ms, before):
        assert same(srt(m.triplets()), bf), "the operands are as they were"
    assert O.IsComplex()
    g = srt(O.triplets())
    print(alpha, "entries", len(want[2]))
    assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]), "pattern"
    assert same(g, want), "values against the restatement"
    assert same(g, srt(V.triplets())), "values against compressed columns"
    # the trace: the bits of MatrixTrace of the new X in the session, and of the scale branch's pass; within the bound of any
    # summation order of the diagonal, as MatrixTrace on compressed columns is
    exact_t, bound_t = _sum_bound(diag)
    to = O.Trace()
    print(alpha, "trace", t, "MatrixTrace in the session", ts, "scale-branch pass", in_slab_form[1], "on compressed columns", tv, to,
          "exact", exact_t, "|difference|", abs(t - exact_t), "bound", bound_t)
    assert t == ts
    assert t == in_slab_form[1]
    assert abs(t - exact_t) <= bound_t
    assert tv == to and abs(tv - exact_t) <= bound_t
    # with the option at 0 MatrixTrace in a complex session is what it was: the sum over compressed columns
    nt.set_option("complex_scale_fold", 0)
    with nt.solver_session():
        assert Mn.Trace() == tv
    nt.set_option("complex_scale_fold", 1)
    # the energy's dot
    exact, bound = _sum_bound(terms)
    print(alpha, "dot", e, "scale-branch pass", in_slab_form[0], "exact", exact, "|difference|", abs(e - exact), "bound", bound,
          "compressed columns", ev)
    assert abs(e - exact) <= bound
    assert abs(in_slab_form[0] - exact) <= bound
    assert abs(ev - exact) <= bound


def test_the_refused_column(nt, fma, operands):
    """one column whose X lies in rows 0-5 and whose X2 in rows 250-255: their hull (256 rows) is not bounded by the two slots (16
    rows each) and the pads between them -- the pass is refused as a whole, nothing changes, the counter rises by one; with the
    runs side by side the same call is taken"""
    alpha = ALPHAS[0]
    a, b = factors(alpha)
    X, X2, WH = ({j: (r.copy(), v.copy()) for j, (r, v) in M.items()} for M in operands[alpha])
    rng = np.random.default_rng(7)
    val = lambda: rng.uniform(0.1, 0.9, 6) + 1j * rng.uniform(0.1, 0.9, 6)
    X[FAR] = (np.arange(0, 6), val())
    X2[FAR] = (np.arange(250, 256), val())
    lo, hi = _hull((X, X2), FAR)
    assert hi - lo == 256 > 16 + 16 + 2 * 16
    Ms = [_matrix(nt, c) for c in (X, X2, WH)]
    before = [srt(m.triplets()) for m in Ms]
    O = nt.Matrix_ps(N)
    c0, r0, s0 = nt.complex_scale_fold_counts(), nt.scale_fold_step_counts(), nt.slab_algebra_counts()
    with nt.solver_session():
        got = nt.scale_fold_update_step(Ms[0], Ms[1], a, b, Ms[2], O)
    c1, s1 = nt.complex_scale_fold_counts(), nt.slab_algebra_counts()
    assert got is None
    assert c1 == dict(c0, refused=c0["refused"] + 1), (c0, c1)
    assert s1 == s0 and nt.scale_fold_step_counts() == r0   # (a refused pass is no operation and no refusal of the session)
    for m, bf in zip(Ms, before):
        assert same(srt(m.triplets()), bf)
    assert len(O.triplets()[2]) == 0
    # factors that are not finite are refused before anything is launched
    for fa, fb in ((float("nan"), b), (a, float("inf"))):
        with nt.solver_session():
            assert nt.scale_fold_update_step(Ms[0], Ms[1], fa, fb, Ms[2], O) is None
    assert nt.complex_scale_fold_counts() == dict(c0, refused=c0["refused"] + 3)
    # the runs side by side
    X2[FAR] = (np.arange(4, 10), X2[FAR][1])
    M2 = _matrix(nt, X2)
    with nt.solver_session():
        got = nt.scale_fold_update_step(Ms[0], M2, a, b, Ms[2], O)
    assert got is not None
    assert same(srt(O.triplets()), srt(_triplets(restated(X, X2, WH, alpha)[0])))


def test_three_forms_of_wh(nt, fma, operands, references):
    """WH in compressed columns, in complex slab form, and as a read-only view that stores zeros in holes of its runs (the same
    values: a stored zero adds an exact zero).  The update enters WH into slab form or a view; the scale-branch pass reads all
    three as they stand.  The traces do not depend on WH; the view's runs are those of the slab form with the holes' zeros
    stored, so the scale-branch pass over either computes the same sums in the same order"""
    alpha = ALPHAS[1]
    a, b = factors(alpha)
    X, X2, WH = operands[alpha]
    new, terms, diag = references[alpha]
    WHz = {j: (rows.copy(), vals.copy()) for j, (rows, vals) in WH.items()}
    planted = 0
    for j in (ONLY_X2, CANCEL, LONG):
        rows = WH[j][0]
        holes = np.setdiff1d(np.arange(rows[0], rows[-1] + 1), rows)
        for r in np.intersect1d(holes, new[j][0])[:2]:   # (where the new X holds an entry: the zero meets a value)
            k = int(np.searchsorted(WHz[j][0], r))
            WHz[j] = (np.insert(WHz[j][0], k, r), np.insert(WHz[j][1], k, 0.0))
            planted += 1
    assert planted >= 2
    exact, bound = _sum_bound(terms)
    assert _sum_bound(restated(X, X2, WHz, alpha)[1]) == (exact, bound), "the stored zeros add no term"
    MX, MX2, Mn = _matrix(nt, X), _matrix(nt, X2), _matrix(nt, new)
    MW_cols, MW_slab, MW_view = _matrix(nt, WH), _matrix(nt, WH), _matrix(nt, WHz)
    assert np.sum(MW_view.triplets()[2] == 0.0) == planted
    outs = [nt.Matrix_ps(N) for _ in range(3)]
    c0, v0 = nt.complex_scale_fold_counts(), nt.slab_view_counts()
    with nt.solver_session():
        u_cols = nt.scale_fold_update_step(MX, MX2, a, b, MW_slab, outs[0])   # (enters WH: it is in complex slab form from here on)
        u_slab = nt.scale_fold_update_step(MX, MX2, a, b, MW_slab, outs[1])
        u_view = nt.scale_fold_update_step(MX, MX2, a, b, MW_view, outs[2])   # (enters WH as a read-only view)
        d_cols = nt.scale_fold_dot_trace(Mn, MW_cols)
        d_slab = nt.scale_fold_dot_trace(Mn, MW_slab)
        d_view = nt.scale_fold_dot_trace(Mn, MW_view)
    print("update", u_cols, u_slab, u_view, "scale-branch pass", d_cols, d_slab, d_view, "exact", exact, "bound", bound, "views",
          v0, nt.slab_view_counts())
    assert None not in (u_cols, u_slab, u_view, d_cols, d_slab, d_view)
    assert delta(nt.complex_scale_fold_counts(), c0) == dict(updates=3, dot_traces=3, refused=0)
    assert nt.slab_view_counts()["built"] == v0["built"] + 1, "the WH with stored zeros became a view"
    for got in (u_cols, u_slab, u_view, d_cols, d_slab, d_view):
        assert abs(got[0] - exact) <= bound
        assert got[1] == u_cols[1], "the trace does not depend on WH"
    assert u_slab == u_cols and u_view == u_cols and d_view == d_slab, "the same runs, the same order"
    want = srt(_triplets(new))
    for O in outs:
        assert same(srt(O.triplets()), want)
    assert same(srt(MW_view.triplets()), srt(_triplets(WHz))), "the stored zeros are still there"
    assert same(srt(MW_cols.triplets()), srt(_triplets(WH)))


def test_zero_imaginary_parts_give_the_real_kernel(nt, fma, operands):
    """the same entry points on real matrices run the real kernels: their new X bit for bit in the real parts, every imaginary
    part 0, the trace and the dot with the same bits (the same terms in the same order)"""
    alpha = ALPHAS[0]
    a, b = factors(alpha)
    zr = [{j: (rows, vals.real + 0j) for j, (rows, vals) in M.items()} for M in operands[alpha]]
    exact, bound = _sum_bound(restated(*zr, alpha)[1])
    Oc, Or = nt.Matrix_ps(N), nt.Matrix_ps(N)
    Mc, Mr = [_matrix(nt, M) for M in zr], [_matrix(nt, M, real=True) for M in zr]
    nt.set_option("scale_fold_step", 1)
    c0, r0 = nt.complex_scale_fold_counts(), nt.scale_fold_step_counts()
    with nt.solver_session():
        gc = nt.scale_fold_update_step(Mc[0], Mc[1], a, b, Mc[2], Oc)
        c1, r1 = nt.complex_scale_fold_counts(), nt.scale_fold_step_counts()
        gr = nt.scale_fold_update_step(Mr[0], Mr[1], a, b, Mr[2], Or)
    assert gc is not None and gr is not None
    assert delta(c1, c0) == dict(updates=1, dot_traces=0, refused=0) and r1 == r0, "the complex call counts as complex only"
    assert nt.complex_scale_fold_counts() == c1, "real operands never count here"
    assert delta(nt.scale_fold_step_counts(), r1) == dict(updates=1, dot_traces=0, refused=0)
    print("dot", gc[0], gr[0], "trace", gc[1], gr[1])
    assert gc[1] == gr[1]
    # (hpcp_term adds an exact zero to each term; a lane visits its rows in ascending order at either chunk depth; hulls aligned to
    # 16 rows instead of the real slots' 32 move a term by 16 lanes at most, inside the four lanes wave_sum_f64 adds first)
    assert gc[0] == gr[0]
    assert abs(gc[0] - exact) <= bound and abs(gr[0] - exact) <= bound
    assert Oc.IsComplex() and not Or.IsComplex()
    c, r = srt(Oc.triplets()), srt(Or.triplets())
    assert np.array_equal(c[0], r[0]) and np.array_equal(c[1], r[1]), "pattern"
    assert np.array_equal(c[2].real, r[2]) and np.all(c[2].imag == 0.0)
    assert len(r[2]) > 1000


def test_gates_of_the_diagnostics(nt, fma, operands):
    """the option at 0, no session, a session that does not take complex operands, mixed real and complex operands: declined,
    nothing counted anywhere, every matrix as it was"""
    alpha = ALPHAS[0]
    a, b = factors(alpha)
    Ms = [_matrix(nt, c) for c in operands[alpha]]
    Rs = [_matrix(nt, c, real=True) for c in operands[alpha]]
    before = [srt(m.triplets()) for m in Ms + Rs]
    O = nt.Matrix_ps(N)
    c0, r0, s0 = nt.complex_scale_fold_counts(), nt.scale_fold_step_counts(), nt.slab_algebra_counts()

    def declined(X, X2, WH):
        assert nt.scale_fold_update_step(X, X2, a, b, WH, O) is None and nt.scale_fold_dot_trace(X, WH) is None

    nt.set_option("complex_scale_fold", 0)
    with nt.solver_session():
        declined(*Ms)
    nt.set_option("complex_scale_fold", 1)
    declined(*Ms)   # (outside a session)
    with nt.solver_session(False):
        declined(*Ms)
    nt.set_option("scale_fold_step", 1)
    with nt.solver_session():
        declined(Ms[0], Ms[1], Rs[2])
        declined(Rs[0], Rs[1], Ms[2])
        assert nt.scale_fold_update_step(Ms[0], Rs[1], a, b, Ms[2], O) is None
        assert nt.scale_fold_update_step(Rs[0], Ms[1], a, b, Rs[2], O) is None
    assert nt.complex_scale_fold_counts() == c0 and nt.scale_fold_step_counts() == r0 and nt.slab_algebra_counts() == s0
    assert len(O.triplets()[2]) == 0
    for m, bf in zip(Ms + Rs, before):
        assert same(srt(m.triplets()), bf)


# ------------------------------------------------------------------ the solver
SOLVE = (1536, 16, 1e-7, 12)
OCCUPATION = 0.5


def close(got, want, n, thr, what, rel=1e-10):
    """the rule of tests/test_gpu_complex_hpcp.py: larger differences only at the threshold, entry counts nearly equal"""
    import scipy.sparse as sp
    G = sp.csr_matrix((got[2], (got[1] - 1, got[0] - 1)), shape=(n, n))
    W = sp.csr_matrix((want[2], (want[1] - 1, want[0] - 1)), shape=(n, n))
    scale = max(1.0, np.abs(want[2]).max())
    D = (G - W).tocoo()
    bad = np.abs(D.data) > rel * scale
    print(what, "max |difference|", np.abs(D.data).max() if D.nnz else 0.0, "beyond", rel * scale, ":", int(bad.sum()), "entries", G.nnz, W.nnz)
    assert np.all(np.abs(D.data[bad]) <= thr * (1 + 1e-9) + rel * scale), "%s: max |d| = %g" % (what, np.abs(D.data).max())
    assert abs(G.nnz - W.nnz) <= max(8, 1e-5 * W.nnz), "%s: %d vs %d entries" % (what, G.nnz, W.nnz)


def frontier(trip, n, nel):
    """homo and lumo: the eigenvalues on either side of the occupation, from the dense operand"""
    c, r, v = trip
    H = np.zeros((n, n), dtype=np.complex128 if np.iscomplexobj(v) else np.float64)
    H[r - 1, c - 1] = v
    ev = np.linalg.eigvalsh(H)
    k = int(round(nel))
    return float(ev[k - 1]), float(ev[k])


def saf(nt, n, trip, opt, nel, homo_lumo, iters=SOLVE[3], thr=SOLVE[2]):
    nt.set_option("complex_scale_fold", opt)
    Hm = nt.Matrix_ps.from_triplets(n, *trip)
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    p = nt.SolverParameters()
    p.SetThreshold(thr)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(iters)
    p.SetMonitorConvergence(False)
    K = nt.Matrix_ps(n)
    c0, r0, b0, s0 = nt.complex_scale_fold_counts(), nt.scale_fold_step_counts(), nt.block_algebra_counts(), nt.slab_algebra_counts()
    energy = nt.DensityMatrixSolvers.ScaleAndFold(Hm, I, nel, K, homo_lumo[0], homo_lumo[1], p)
    c1, r1, b1, s1 = nt.complex_scale_fold_counts(), nt.scale_fold_step_counts(), nt.block_algebra_counts(), nt.slab_algebra_counts()
    tr = nt.solver_trace()
    return dict(K=srt(K.triplets()), energy=energy, it=tr["iterations"], sigma=np.asarray(tr["sigma"]).copy(),
                e=np.asarray(tr["energy"]).copy(), nnz=np.asarray(tr["nnz"]).copy(), counts=delta(c1, c0), real_counts=delta(r1, r0),
                block=delta(b1, b0), slab=delta(s1, s0))


def agree(a, b, n, thr, what):
    """the numbers a complex session is held to against option 0 (agree and close of tests/test_gpu_complex_hpcp.py; ScaleAndFold
    records its branch, -1 scale and +1 fold, where HPCP records sigma: the sequence is identical)"""
    print(what, "iterations", a["it"], b["it"], "branches equal", bool(np.array_equal(a["sigma"], b["sigma"])), "max relative energy difference",
          float(np.max(np.abs(a["e"] - b["e"]) / np.abs(b["e"]))), "entry counts equal", bool(np.array_equal(a["nnz"], b["nnz"])))
    assert a["it"] == b["it"]
    assert np.array_equal(a["sigma"], b["sigma"]), "branch sequence"
    assert np.allclose(a["e"], b["e"], rtol=1e-10, atol=0.0)
    assert abs(a["energy"] - b["energy"]) <= 1e-10 * abs(b["energy"])
    close(a["K"], b["K"], n, thr, what)


def fused_counts_ok(r):
    c = r["counts"]
    assert c["updates"] + c["dot_traces"] >= r["it"] - 1 and c["refused"] == 0, c
    assert r["real_counts"] == NONE


def dense_saf(trip, n, nel, homo_lumo, thr, iters):
    """solvers.cpp solver_scale_and_fold with dense numpy arrays: Gershgorin bounds as DensityFrame takes them, the product cut at
    |x| > thr, the merges at threshold 0; returns trace(X) at the head of every iteration, its branch (-1 scale, +1 fold) and
    its energy"""
    c, r, v = trip
    H = np.zeros((n, n), dtype=np.complex128)
    H[r - 1, c - 1] = v
    cut = lambda M: np.where(np.abs(M) > thr, M, 0.0)
    I = np.eye(n)
    WH = cut(H)   # (ISQ = I: the two products of the similarity transform are exact, their thresholds this one)
    dg = np.diag(WH).real
    rad = np.abs(WH).sum(axis=0) - np.abs(np.diag(WH))
    e_min, e_max = float(np.min(dg - rad)), float(np.max(dg + rad))
    X = ((-1.0) * WH + e_max * I) * (1.0 / (e_max - e_min))
    Beta = (e_max - homo_lumo[1]) / (e_max - e_min)
    BetaBar = (e_max - homo_lumo[0]) / (e_max - e_min)
    traces, branches, energies = [], [], []
    for _ in range(iters):
        t = float(np.trace(X).real)
        if t > nel:
            alpha = 2.0 / (2.0 - Beta)
            X = alpha * X + (1.0 - alpha) * I
            X = cut(X @ X)
            Beta = (alpha * Beta + 1 - alpha) * (alpha * Beta + 1 - alpha)
            BetaBar = (alpha * BetaBar + 1 - alpha) * (alpha * BetaBar + 1 - alpha)
        else:
            alpha = 2.0 / (1.0 + BetaBar)
            X = (2 * alpha) * X + (-1.0 * alpha * alpha) * cut(X @ X)
            Beta = 2.0 * alpha * Beta - alpha * alpha * Beta * Beta
            BetaBar = 2.0 * alpha * BetaBar - alpha * alpha * BetaBar * BetaBar
        traces.append(t)
        branches.append(-1.0 if t > nel else 1.0)
        energies.append(2.0 * float(np.sum(X.real * WH.real + X.imag * WH.imag)))
    return np.array(traces), np.array(branches), np.array(energies)


@pytest.fixture(scope="module")
def banded():
    n = SOLVE[0]
    trip = banded_triplets(n, SOLVE[1], complex_=True)
    return trip, frontier(trip, n, OCCUPATION * n)


@pytest.fixture(scope="module")
def dense(banded):
    trip, hl = banded
    n, _, thr, iters = SOLVE
    return dense_saf(trip, n, OCCUPATION * n, hl, thr, iters)


@pytest.fixture(scope="module")
def solves(nt, banded):
    """option 0 and option 1 on the banded operand, once for the tests below"""
    trip, hl = banded
    n = SOLVE[0]
    keep = {k: nt.get_option(k) for k in OPTIONS}
    for k in ("spgemm_fma", "complex_tile", "complex_sessions", "slab_algebra"):
        nt.set_option(k, 1)
    try:
        return dict(off=saf(nt, n, trip, 0, OCCUPATION * n, hl), on=saf(nt, n, trip, 1, OCCUPATION * n, hl))
    finally:
        for k, v in keep.items():
            nt.set_option(k, v)


def test_solver_inputs(solves, dense):
    """conditions on the inputs, on the option-0 run: both branches occur, the run does not end early, and trace(X) stays away from
    the electron count by more than 1e-6 at the head of every iteration, so that a last-bit difference cannot flip a branch (the
    traces are those of the dense restatement, whose branch sequence is the one option 0 took)"""
    off = solves["off"]
    traces, branches, _ = dense
    nel = OCCUPATION * SOLVE[0]
    print("option 0: branches", off["sigma"].tolist(), "dense trace(X) - nel", (traces - nel).tolist())
    assert off["it"] == SOLVE[3], "the run does not converge early"
    assert set(off["sigma"].tolist()) == {-1.0, 1.0}, "both branches occur"
    assert np.array_equal(off["sigma"], branches), "the dense restatement takes option 0's branches"
    assert np.all(np.abs(traces - nel) > 1e-6)
    assert off["counts"] == NONE == off["real_counts"]


def test_solver_option_1_against_option_0(solves):
    n = SOLVE[0]
    on, off = solves["on"], solves["off"]
    print("counts", on["counts"], "slab algebra", on["slab"], off["slab"], "branches", on["sigma"].tolist())
    assert on["it"] == SOLVE[3]
    agree(on, off, n, SOLVE[2], "density, option 1 against option 0")
    fused_counts_ok(on)
    assert on["counts"]["updates"] >= 1 and on["counts"]["dot_traces"] >= 1, "both fused passes ran"
    assert on["slab"]["products"] >= on["it"] - 1, "the loop's products ran in complex slab form"
    assert on["slab"]["refusals"] <= off["slab"]["refusals"]


# what the EXISTING path (option 0) differs by from the dense restatement below, measured once on an MI355X (printed by the test on
# every run): the largest relative energy difference over the twelve iterations.  Both options are held to ten times this figure
# -- the margin covers an entry that lands on the other side of the threshold -- and to nothing measured with option 1 itself.
OPTION_0_ENERGY = 1.416e-14   # (option 1 measured 4.481e-15)


def test_solver_against_a_dense_restatement(solves, dense):
    """the energies of every iteration against the dense restatement at the same threshold, option 0 and option 1 under the same
    pinned bound"""
    on, off = solves["on"], solves["off"]
    _, branches, we = dense
    assert off["it"] == on["it"] == SOLVE[3]
    d = {k: float(np.max(np.abs(r["e"] - we) / np.abs(we))) for k, r in (("off", off), ("on", on))}
    print("against the dense restatement, max relative energy difference: option 0 %.3e, option 1 %.3e" % (d["off"], d["on"]))
    assert np.array_equal(on["sigma"], branches)
    assert d["off"] <= 10.0 * OPTION_0_ENERGY
    assert d["on"] <= 10.0 * OPTION_0_ENERGY


def bit_equal(a, b):
    return (a["it"] == b["it"] and list(a["e"]) == list(b["e"]) and list(a["sigma"]) == list(b["sigma"]) and a["energy"] == b["energy"] and
            np.array_equal(a["nnz"], b["nnz"]) and all(np.array_equal(x, y) for x, y in zip(a["K"], b["K"])))


@pytest.mark.parametrize("which", ["spgemm_fma", "complex_tile", "complex_sessions"])
def test_outside_the_gates_bit_for_bit(nt, fma, banded, which):
    trip, hl = banded
    n = SOLVE[0]
    nt.set_option(which, 0)
    a = saf(nt, n, trip, 1, OCCUPATION * n, hl, iters=6)
    b = saf(nt, n, trip, 0, OCCUPATION * n, hl, iters=6)
    assert a["counts"] == NONE == b["counts"] and a["real_counts"] == NONE == b["real_counts"]
    assert bit_equal(a, b)


def test_option_0_is_the_loop_as_before(nt, fma, banded, solves):
    """with the option at 0 a complex operand opens no session whatever scale_fold_step says: no counter moves, no operation in
    slab form, and the two settings of the real loop's option give the same bits"""
    trip, hl = banded
    n = SOLVE[0]
    nt.set_option("scale_fold_step", 0)
    a = saf(nt, n, trip, 0, OCCUPATION * n, hl)
    nt.set_option("scale_fold_step", 1)
    b = saf(nt, n, trip, 0, OCCUPATION * n, hl)
    for r in (a, b):
        assert r["counts"] == NONE == r["real_counts"] and r["slab"]["products"] == 0 and r["slab"]["merges"] == 0
    assert bit_equal(a, b) and bit_equal(a, solves["off"])


def test_a_real_operand_is_untouched(nt, fma):
    n, h = SOLVE[0], SOLVE[1]
    trip = banded_triplets(n, h)
    hl = frontier(trip, n, OCCUPATION * n)
    a = saf(nt, n, trip, 1, OCCUPATION * n, hl, iters=6)
    b = saf(nt, n, trip, 0, OCCUPATION * n, hl, iters=6)
    assert a["counts"] == NONE == b["counts"]
    assert a["real_counts"] == b["real_counts"]
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
    hl = frontier(trip, n, n / 2.0)
    nt.set_option("block_path", 2)
    nt.set_option("block_complex", 1)
    on = saf(nt, n, trip, 1, n / 2.0, hl, iters=8)
    off = saf(nt, n, trip, 0, n / 2.0, hl, iters=8)
    print("block algebra", on["block"], off["block"], "counts", on["counts"], "slab algebra", on["slab"])
    agree(on, off, n, SOLVE[2], "lattice density, option 1 against option 0")
    assert on["block"]["operations"] >= on["it"] - 1
    assert on["counts"]["updates"] == 0 and on["counts"]["dot_traces"] == 0, on["counts"]
