"""GPU: complex PM purification in a complex slab session (option complex_pm; csrc/slab_extra.hip k_pm_sigma<double2> and
k_pm_update<double2, ., 2>, engine.hpp ps_pm_sigma / ps_pm_update on complex operands).  Whenever sigma > 1/2 the update scales the
iterate by a1 = 0: compressed columns then hold stored (0, 0) entries, and AddSparseVectors copies a column's tail unfiltered, so a
stored zero beyond the other operand's last row survives and steers the merges that follow.  The fused path keeps zero-free runs of
(re, im) pairs and carries those rows in a list, as the real session does (tests/test_gpu_pm_session.py).

The kernels are reached with crafted operands through nt.pm_fused_step and are compared with (a) the vocabulary on compressed
columns (slab_algebra = 0: ScaleMatrix and IncrementMatrix of the C ABI on complex matrices) and (b) a numpy restatement of
AddSparseVectors.f90 on complex vectors written here -- never with the fused code itself.  Every scalar of the loop is real, so
the restatement scales and adds part by part; numpy's float64 products and sums are the correctly rounded ones the kernels spell as
__dmul_rn / __dadd_rn, so the update is compared bit for bit, both parts as int64.  The threshold is on the modulus, a hypot on
both sides: the operands are drawn so that no modulus a threshold decision reads lies within 1e-9 relative of the threshold
(checked here on the CPU), which keeps a one-ulp difference between two hypot implementations from deciding a pattern.  A stored
zero has signs in compressed columns that a row list does not carry: stored zeros are compared as rows whose value is zero.

A cancellation to exactly (0, 0).  The issue behind this file lists "a cancellation to exactly (0, 0) in a tail, which creates a
stored zero" among the branches.  Under AddSparseVectors a sum is only formed where both lists hold the row, and such a sum is
kept iff its modulus exceeds the threshold -- never for (0, 0), at any threshold, however far the row lies beyond the third
operand's last row.  The restatement, which decides here, drops the planted cancellation (row CANCEL_ROW of column CANCEL, beyond
X3's last row in that column), and so must both device paths: the test asserts that.  Stored zeros arise from a1 = 0 only."""
import math

import numpy as np
import pytest

from gen import banded_triplets, lattice_triplets

pytestmark = pytest.mark.gpu
N = 259   # (not a multiple of the 4 waves of a workgroup)
ALIGN = 16          # rows a complex slot is aligned to
FITS = 2 * 64       # rows the complex update keeps in registers between its loops (PM_KC_C = 2 chunks of 64 rows)
NONE = dict(sigma=0, updates=0, zeros=0, left=0)
OPTIONS = ("spgemm_fma", "complex_tile", "complex_sessions", "complex_pm", "pm_session", "slab_algebra", "block_path", "block_complex")
NARROW, LONG = 20, 129            # a column whose walked extent fits FITS rows in every case, one whose X spans rows 1 .. 257
CANCEL, CANCEL_ROW = 30, 33       # merge 1 at sg = 0.3 sums to exactly (0, 0) there; X3's column ends at row 31
CANCEL_RE, CANCEL_RE_ROW = 29, 32   # ... and to (0, im != 0) there: an ordinary entry


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


def _with_options(nt, arith):
    keep = {k: nt.get_option(k) for k in OPTIONS}
    nt.set_option("spgemm_fma", arith)
    nt.set_option("complex_tile", 1)
    nt.set_option("complex_sessions", 1)
    nt.set_option("slab_algebra", 1)
    nt.set_option("complex_pm", 1)
    yield arith
    for k, v in keep.items():
        nt.set_option(k, v)


@pytest.fixture(params=[1, 0], ids=["fma", "unfused"])
def fma(nt, request):
    """both arithmetic modes; the complex path needs FMA arithmetic, complex_tile and complex_sessions: under `unfused` the
    diagnostic is refused and a solve takes the loop on compressed columns"""
    yield from _with_options(nt, request.param)


@pytest.fixture()
def fma_only(nt):
    yield from _with_options(nt, 1)


def books(nt):
    return nt.complex_pm_counts(), nt.pm_session_counts()


def delta(c1, c0):
    return {k: c1[k] - c0[k] for k in c1}


def srt(t):
    c, r, v = (np.asarray(x) for x in t)
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def bits(v):
    """both parts of complex values (or real values) as int64; indices as they are"""
    v = np.asarray(v)
    if np.iscomplexobj(v):
        return np.ascontiguousarray(v.real).view(np.int64), np.ascontiguousarray(v.imag).view(np.int64)
    if v.dtype != np.float64:
        return (v,)
    return (np.ascontiguousarray(v).view(np.int64),)


def same_bits(a, b):
    return all(np.array_equal(p, q) for p, q in zip(bits(a), bits(b)))


def cpx(re, im):
    """complex values from their parts, no arithmetic (signs of zeros kept)"""
    out = np.empty(len(re), dtype=np.complex128)
    out.real = re
    out.imag = im
    return out


def scale(alpha, v):
    """a real factor times complex values, part by part (Sc<double2>::scale)"""
    return cpx(alpha * v.real, alpha * v.imag)


def coefficients(sg):
    if sg > 0.5:
        return 0.0, 1.0 + 1.0 / sg, -1.0 / sg
    return (1.0 - 2.0 * sg) / (1.0 - sg), (1.0 + sg) / (1.0 - sg), -1.0 / (1.0 - sg)


# ------------------------------------------------------------------ operands
def _runs(rng, n, empty, diag_only, fixed=None):
    """{column: (rows, complex values)}: a run around the diagonal with half-widths 6..90 drawn per side, ~12 % holes inside, parts
    log-uniform in [1e-6, 1] with a random sign each; ~6 % of the entries purely real, ~6 % purely imaginary"""
    cols = {}
    for j in range(n):
        if j in empty:
            continue
        if j in diag_only:
            rows = np.array([j])
        else:
            if fixed and j in fixed:
                f, l = fixed[j]
            else:
                f, l = max(0, j - int(rng.integers(6, 91))), min(n - 1, j + int(rng.integers(6, 91)))
            rows = np.arange(f, l + 1)
            keep = rng.random(len(rows)) > 0.12
            keep[0] = keep[-1] = True
            rows = rows[keep]
        part = lambda: 10.0 ** rng.uniform(-6.0, 0.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
        re, im = part(), part()
        kind = rng.random(len(rows))
        im[kind < 0.06] = 0.0
        re[kind > 0.94] = 0.0
        cols[j] = (rows, cpx(re, im))
    return cols


def _set(cols, j, r, v):
    rows, vals = cols[j]
    if r in rows:
        vals[rows == r] = v
    else:
        k = int(np.searchsorted(rows, r))
        cols[j] = (np.insert(rows, k, r), np.insert(vals, k, v))


def _preimage(a, target):
    """x with a * x == target exactly (a correctly rounded product), searched among the neighbours of target / a"""
    x = target / a
    if a * x == target:
        return x
    up = dn = x
    for _ in range(16):
        up, dn = math.nextafter(up, math.inf), math.nextafter(dn, -math.inf)
        for y in (up, dn):
            if a * y == target:
                return y
    raise AssertionError("no preimage")


def _plant(X, X2, X3):
    """at sg = 0.3: merge 1 (Y = a2 X2 + a1 X) sums to exactly (0, 0) at (CANCEL_ROW, CANCEL) and to (0, im) at (CANCEL_RE_ROW,
    CANCEL_RE); exact by construction and checked here from the numpy values alone"""
    a1, a2, _ = coefficients(0.3)
    x2 = complex(0.75, 0.625)
    wa = complex(a2 * x2.real, a2 * x2.imag)
    x = complex(_preimage(a1, -wa.real), _preimage(a1, -wa.imag))
    assert a2 * x2.real + a1 * x.real == 0.0 and a2 * x2.imag + a1 * x.imag == 0.0 and x.real != 0.0 and x.imag != 0.0
    _set(X2, CANCEL, CANCEL_ROW, x2)
    _set(X, CANCEL, CANCEL_ROW, x)
    assert X3[CANCEL][0][-1] < CANCEL_ROW <= min(X[CANCEL][0][-1], X2[CANCEL][0][-1])
    xr = complex(x.real, 0.3)
    assert a2 * x2.real + a1 * xr.real == 0.0 and a2 * x2.imag + a1 * xr.imag > 0.5
    _set(X2, CANCEL_RE, CANCEL_RE_ROW, x2)
    _set(X, CANCEL_RE, CANCEL_RE_ROW, xr)


@pytest.fixture(scope="module")
def operands():
    rng = np.random.default_rng(20261020)
    narrow = {NARROW: (NARROW - 10, NARROW + 12)}
    # empty columns (one operand, two, all three), a diagonal-only column; columns 0 and N - 1 are ordinary runs
    X = _runs(rng, N, empty={7, 40, 41, 100}, diag_only={13}, fixed={NARROW: narrow[NARROW], LONG: (1, 257)})
    X2 = _runs(rng, N, empty={8, 40, 100, 200}, diag_only={13}, fixed=narrow)
    X3 = _runs(rng, N, empty={9, 41, 100, 201}, diag_only={13}, fixed={NARROW: narrow[NARROW], CANCEL: (24, 31)})
    _plant(X, X2, X3)
    # 40 listed rows beyond the last non-zero of their columns of X (some beyond X2 and X3 too, some not)
    Z = {}
    cand = [j for j in X if X[j][0][-1] < N - 2]
    while sum(len(v) for v in Z.values()) < 40:
        j = int(rng.choice(cand))
        r = int(min(N - 1, X[j][0][-1] + rng.integers(1, 30)))
        Z[j] = np.union1d(Z.get(j, np.array([], dtype=np.int64)), [r])
    return X, X2, X3, Z


EMPTY = (np.array([], dtype=np.int64), np.array([], dtype=np.complex128))


def _with_zeros(col, zrows):
    rows, vals = col
    if zrows is None or len(zrows) == 0:
        return rows, vals
    rows = np.concatenate([rows, zrows])
    vals = np.concatenate([vals, np.zeros(len(zrows), dtype=vals.dtype)])
    o = np.argsort(rows)
    return rows[o], vals[o]


def _triplets(cols, zeros=None, real=False):
    c, r, v = [], [], []
    for j in sorted(set(cols) | set(zeros or {})):
        rows, vals = _with_zeros(cols.get(j, EMPTY), (zeros or {}).get(j))
        c.append(np.full(len(rows), j + 1))
        r.append(rows + 1)
        v.append(vals.real.copy() if real else vals)
    if not c:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64 if real else np.complex128)
    return np.concatenate(c).astype(np.int32), np.concatenate(r).astype(np.int32), np.concatenate(v)


def _matrix(nt, cols, zeros=None, n=N, real=False):
    c, r, v = _triplets(cols, zeros, real)
    M = nt.Matrix_ps.from_triplets(n, c, r, v)
    assert len(M.triplets()[2]) == len(v)   # (stored zeros are kept)
    return M


def _pattern_matrix(nt, zeros, n=N):
    if not zeros:
        return nt.Matrix_ps(n)
    return _matrix(nt, {j: (rows, np.ones(len(rows), dtype=np.complex128)) for j, rows in zeros.items()}, n=n)


# ------------------------------------------------------------------ AddSparseVectors.f90 on complex vectors, restated
def add_sparse(ra, va, rb, vb, alpha, thr, log=None, mods=None):
    """c = alpha a + b on sorted sparse complex vectors, alpha real: inside the overlap of the two lists an entry is kept iff its
    modulus > thr, once one list is exhausted the tail of the other is copied unfiltered.  log (optional) collects (row, branch)
    records, mods the moduli the threshold decisions read."""
    wa = scale(alpha, va)
    rc, cre, cim = [], [], []

    def decide(re, im):
        m = math.hypot(re, im)
        if mods is not None:
            mods.append(m)
        return m > thr

    def put(r, re, im):
        rc.append(r); cre.append(re); cim.append(im)

    A, B = 0, 0
    while A < len(ra) and B < len(rb):
        if ra[A] == rb[B]:
            re, im = wa[A].real + vb[B].real, wa[A].imag + vb[B].imag
            keep = decide(re, im)
            if keep:
                put(ra[A], re, im)
            if log is not None:
                log.append((int(ra[A]), "both_kept" if keep else "both_filtered"))
            A += 1
            B += 1
        elif ra[A] > rb[B]:
            keep = decide(vb[B].real, vb[B].imag)
            if keep:
                put(rb[B], vb[B].real, vb[B].imag)
            if log is not None:
                log.append((int(rb[B]), "b_kept" if keep else "b_filtered"))
            B += 1
        else:
            keep = decide(wa[A].real, wa[A].imag)
            if keep:
                put(ra[A], wa[A].real, wa[A].imag)
            if log is not None:
                log.append((int(ra[A]), "a_kept" if keep else "a_filtered"))
            A += 1
    while A < len(ra):
        put(ra[A], wa[A].real, wa[A].imag)
        if log is not None:
            log.append((int(ra[A]), "a_tail_small" if math.hypot(wa[A].real, wa[A].imag) <= thr else "a_tail"))
        A += 1
    while B < len(rb):
        put(rb[B], vb[B].real, vb[B].imag)
        if log is not None:
            log.append((int(rb[B]), "b_tail_small" if math.hypot(vb[B].real, vb[B].imag) <= thr else "b_tail"))
        B += 1
    return np.array(rc, dtype=np.int64), cpx(np.array(cre, dtype=np.float64), np.array(cim, dtype=np.float64))


def restated_update(X, X2, X3, Z, sg, thr, n=N):
    """(result columns {j: (rows, values)} with stored zeros, branch statistics) of ScaleMatrix(X u Z, a1); IncrementMatrix(X2, ., a2,
    thr); IncrementMatrix(X3, ., a3, thr)"""
    a1, a2, a3 = coefficients(sg)
    out, st = {}, dict(both_filtered=0, one_sided_filtered=0, small_tail_1_dropped_2=0, dropped_1_small_tail_2=0, zero_survives=0,
                       zero_dies=0, zero_created=0)
    mods, logs = [], {}
    for j in range(n):
        xr, xv = _with_zeros(X.get(j, EMPTY), Z.get(j))
        sx = scale(a1, xv)
        l1, l2 = [], []
        yr, yv = add_sparse(*X2.get(j, EMPTY), xr, sx, a2, thr, l1, mods)
        fr, fv = add_sparse(*X3.get(j, EMPTY), yr, yv, a3, thr, l2, mods)
        if len(fr):
            out[j] = (fr, fv)
        if j in (CANCEL, CANCEL_RE):
            logs[j] = (dict(l1), dict(l2))
        both = l1 + l2
        st["both_filtered"] += sum(b == "both_filtered" for _, b in both)
        st["one_sided_filtered"] += sum(b in ("a_filtered", "b_filtered") for _, b in both)
        small1 = {r for r, b in l1 if b in ("a_tail_small", "b_tail_small")}
        st["small_tail_1_dropped_2"] += len(small1 - set(fr.tolist()))
        gone1 = {r for r, b in l1 if b.endswith("filtered")}
        st["dropped_1_small_tail_2"] += len(gone1 & {r for r, b in l2 if b in ("a_tail_small", "b_tail_small")})
        zin = set(xr[sx == 0.0].tolist())    # rows the first merge reads as stored zeros of the scaled iterate
        zout = set(fr[fv == 0.0].tolist())
        st["zero_survives"] += len(zin & zout)
        st["zero_dies"] += len(zin - zout)
        st["zero_created"] += len(zout - zin)
    st["mods"] = np.array(mods)
    st["logs"] = logs
    return out, st


CASES = [(thr, sg, zmode) for thr in (0.0, 1e-3) for sg in (0.3, 0.7) for zmode in ("empty", "listed")]


@pytest.fixture(scope="module")
def restated(operands):
    X, X2, X3, Z = operands
    return {(thr, sg, zm): restated_update(X, X2, X3, Z if zm == "listed" else {}, sg, thr) for thr, sg, zm in CASES}


def _walked(cols_list, zeros, j):
    """rows the update walks in column j, aligned: (0, 0) for a column with nothing"""
    rows = [c[j][0] for c in cols_list if j in c] + ([zeros[j]] if j in zeros else [])
    if not rows:
        return 0, 0
    lo, hi = min(int(r[0]) for r in rows), max(int(r[-1]) for r in rows)
    return lo // ALIGN * ALIGN, (hi // ALIGN + 1) * ALIGN


def test_the_inputs_reach_every_branch(operands, restated):
    """from the numpy restatement alone: both present and filtered, one-sided and filtered, a tail kept below thr by the first merge and
    dropped by the second, a row the first merge drops that the second keeps as a tail below thr, a stored zero that survives and one
    that does not, the planted cancellations, purely real and purely imaginary entries, both paths of the update (registers and
    re-reading), and no modulus near the threshold"""
    X, X2, X3, Z = operands
    tot = {}
    for (thr, sg, zm), (want, st) in restated.items():
        for k, v in st.items():
            if k not in ("mods", "logs"):
                tot[k] = tot.get(k, 0) + v
        if sg > 0.5 or zm == "listed":
            assert st["zero_survives"] > 0 and st["zero_dies"] > 0, ((thr, sg, zm), st)
        if thr > 0:
            assert st["both_filtered"] > 0 and st["one_sided_filtered"] > 0, ((thr, sg, zm), st)
            assert st["small_tail_1_dropped_2"] > 0 and st["dropped_1_small_tail_2"] > 0, ((thr, sg, zm), st)
            near = np.abs(st["mods"] - thr) <= 1e-9 * thr
            assert not near.any(), ("a modulus within 1e-9 relative of the threshold", st["mods"][near])
        # (a stored zero arises from a1 = 0 and from nothing else: see the module docstring)
        assert st["zero_created"] == 0, ((thr, sg, zm), st)
        if sg < 0.5:
            l1, _ = st["logs"][CANCEL]
            assert l1[CANCEL_ROW] == "both_filtered" and CANCEL_ROW not in want[CANCEL][0], "the exact cancellation is dropped"
            l1, _ = st["logs"][CANCEL_RE]
            rows, vals = want[CANCEL_RE]
            v = vals[rows == CANCEL_RE_ROW]
            assert l1[CANCEL_RE_ROW] == "both_kept" and len(v) == 1 and v[0].real == 0.0 and abs(v[0].imag) > 0.5, "one part cancels"
    allv = np.concatenate([c[j][1] for c in (X, X2, X3) for j in c])
    assert np.sum((allv.imag == 0.0) & (allv.real != 0.0)) > 50 and np.sum((allv.real == 0.0) & (allv.imag != 0.0)) > 50
    assert not np.any((allv.real == 0.0) & (allv.imag == 0.0))
    for cols, gone in ((X, 7), (X2, 8), (X3, 9)):
        assert gone not in cols
    assert all(len(c[13][0]) == 1 for c in (X, X2, X3))
    ext = {j: _walked((X, X2, X3), Z, j) for j in range(N)}
    width = {j: e[1] - e[0] for j, e in ext.items()}
    assert 0 < width[NARROW] <= FITS and width[LONG] > FITS and X[LONG][0][0] == 1 and X[LONG][0][-1] == 257
    print("branches over all cases:", tot, "columns kept in registers:", sum(0 < w <= FITS for w in width.values()),
          "columns read twice:", sum(w > FITS for w in width.values()))


def _check_update(want, Out, Zout):
    wc, wr, wv = _triplets(want)
    oc, orr, ov = srt(Out.triplets())
    zc, zr, zv = srt(Zout.triplets())
    assert np.all(ov != 0.0) and np.all(zv == 0.0)
    nzm = wv != 0.0
    assert np.array_equal(oc, wc[nzm]) and np.array_equal(orr, wr[nzm]), "non-zeros: pattern"
    assert same_bits(ov, wv[nzm]), "non-zeros: both parts, bit for bit"
    assert np.array_equal(zc, wc[~nzm]) and np.array_equal(zr, wr[~nzm]), "stored zeros: rows"
    return len(wv), int((~nzm).sum())


@pytest.mark.parametrize("thr,sg,zmode", CASES)
def test_update_bit_for_bit(nt, fma, operands, restated, thr, sg, zmode):
    X, X2, X3, Z = operands
    Z = Z if zmode == "listed" else {}
    a1, a2, a3 = coefficients(sg)
    want, _ = restated[(thr, sg, zmode)]
    wc, wr, wv = _triplets(want)
    # the vocabulary on compressed columns
    nt.set_option("slab_algebra", 0)
    W = _matrix(nt, X, Z)
    M2, M3 = _matrix(nt, X2), _matrix(nt, X3)
    W.Scale(a1)
    W.Increment(M2, a2, thr)
    W.Increment(M3, a3, thr)
    cc, cr, cv = srt(W.triplets())
    assert np.array_equal(cc, wc) and np.array_equal(cr, wr), "compressed columns against the restatement: pattern"
    assert same_bits(cv[wv != 0.0], wv[wv != 0.0]) and np.all(cv[wv == 0.0] == 0.0)
    # the fused step
    nt.set_option("slab_algebra", 1)
    MX, MZ = _matrix(nt, X), _pattern_matrix(nt, Z)
    Out, Zout = nt.Matrix_ps(N), nt.Matrix_ps(N)
    before = [srt(m.triplets()) for m in (MX, MZ, M2, M3)]
    b0 = books(nt)
    got = nt.pm_fused_step(MX, MZ, M2, M3, a1, a2, a3, thr, Out, Zout)
    assert books(nt) == b0   # (the diagnostic keeps no books)
    for m, b in zip((MX, MZ, M2, M3), before):
        assert all(same_bits(p, q) for p, q in zip(srt(m.triplets()), b))
    if not fma:
        assert got is None and len(Out.triplets()[2]) == 0 and len(Zout.triplets()[2]) == 0, "unfused arithmetic: refused"
        return
    assert got is not None
    assert Out.IsComplex() and Zout.IsComplex()
    print("case", (thr, sg, zmode), "entries, stored zeros", _check_update(want, Out, Zout))


@pytest.mark.parametrize("thr", [0.0, 1e-3])
@pytest.mark.parametrize("zmode", ["empty", "listed"])
def test_sigma_pass(nt, fma, operands, thr, zmode):
    """trace and Re dot(., X) of Temp = X - X2 merged at thr against Trace / Dot of the compressed-column Temp and the restatement, to
    1e-13 x the sum of the terms' magnitudes, each real product a term (a reordered sum of the same terms)"""
    X, X2, X3, Z = operands
    Z = Z if zmode == "listed" else {}
    tr, dt, atr, adt = 0.0, 0.0, 0.0, 0.0
    for j in range(N):
        xr, xv = _with_zeros(X.get(j, EMPTY), Z.get(j))
        rr, rv = add_sparse(*X2.get(j, EMPTY), xr, xv, -1.0, thr)
        d = rv[rr == j].real
        tr += d.sum()
        atr += np.abs(d).sum()
        both, ia, ib = np.intersect1d(rr, xr, return_indices=True)
        terms = np.concatenate([rv[ia].real * xv[ib].real, rv[ia].imag * xv[ib].imag])
        dt += terms.sum()
        adt += np.abs(terms).sum()
    nt.set_option("slab_algebra", 0)
    W = _matrix(nt, X, Z)
    M2, M3 = _matrix(nt, X2), _matrix(nt, X3)
    T = nt.Matrix_ps(W)
    T.Increment(M2, -1.0, thr)
    ctr, cdt = T.Trace(), complex(T.Dot(W)).real
    nt.set_option("slab_algebra", 1)
    MX, MZ = _matrix(nt, X), _pattern_matrix(nt, Z)
    Out, Zout = nt.Matrix_ps(N), nt.Matrix_ps(N)
    got = nt.pm_fused_step(MX, MZ, M2, M3, 0.5, 1.5, -1.0, thr, Out, Zout)
    assert abs(ctr - tr) <= 1e-13 * atr and abs(cdt - dt) <= 1e-13 * adt, "compressed columns against the restatement"
    if not fma:
        assert got is None
        return
    assert got is not None
    print("trace", got[0], ctr, tr, "dot", got[1], cdt, dt, "bounds", 1e-13 * atr, 1e-13 * adt)
    assert abs(got[0] - ctr) <= 1e-13 * atr and abs(got[0] - tr) <= 1e-13 * atr
    assert abs(got[1] - cdt) <= 1e-13 * adt and abs(got[1] - dt) <= 1e-13 * adt


# ------------------------------------------------------------------ zero imaginary parts
def _real_file_operands():
    """the operands of tests/test_gpu_pm_session.py: its recipe, its seed, its order of draws"""
    def runs(rng, n, empty, diag_only):
        cols = {}
        for j in range(n):
            if j in empty:
                continue
            if j in diag_only:
                rows = np.array([j])
            else:
                f, l = max(0, j - int(rng.integers(6, 91))), min(n - 1, j + int(rng.integers(6, 91)))
                rows = np.arange(f, l + 1)
                keep = rng.random(len(rows)) > 0.12
                keep[0] = keep[-1] = True
                rows = rows[keep]
            vals = 10.0 ** rng.uniform(-6.0, 0.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
            cols[j] = (rows, vals)
        return cols
    rng = np.random.default_rng(20261019)
    X = runs(rng, N, {7, 40, 41, 100}, {13})
    X2 = runs(rng, N, {8, 40, 100, 200}, {13})
    X3 = runs(rng, N, {9, 41, 100, 201}, {13})
    Z = {}
    cand = [j for j in X if X[j][0][-1] < N - 2]
    while sum(len(v) for v in Z.values()) < 40:
        j = int(rng.choice(cand))
        r = int(min(N - 1, X[j][0][-1] + rng.integers(1, 30)))
        Z[j] = np.union1d(Z.get(j, np.array([], dtype=np.int64)), [r])
    return X, X2, X3, Z


@pytest.mark.parametrize("sg", [0.3, 0.7])
def test_zero_imaginary_parts_give_the_real_kernel(nt, fma_only, sg):
    """the real file's operands as complex matrices with zero imaginary parts: Out's real parts have the bits of the real step's Out,
    every imaginary part is zero, the rows of Zout are the same, and so are both sums"""
    X, X2, X3, Z = _real_file_operands()
    a1, a2, a3 = coefficients(sg)
    thr = 1e-3
    as_c = lambda cols: {j: (r, v.astype(np.complex128)) for j, (r, v) in cols.items()}
    real = [_matrix(nt, {j: (r, v + 0j) for j, (r, v) in c.items()}, real=True) for c in (X, X2, X3)]
    RZ = _matrix(nt, {j: (rows, np.ones(len(rows)) + 0j) for j, rows in Z.items()}, real=True)
    ROut, RZout = nt.Matrix_ps(N), nt.Matrix_ps(N)
    rs = nt.pm_fused_step(real[0], RZ, real[1], real[2], a1, a2, a3, thr, ROut, RZout)
    cplx = [_matrix(nt, as_c(c)) for c in (X, X2, X3)]
    COut, CZout = nt.Matrix_ps(N), nt.Matrix_ps(N)
    cs = nt.pm_fused_step(cplx[0], _pattern_matrix(nt, Z), cplx[1], cplx[2], a1, a2, a3, thr, COut, CZout)
    assert rs is not None and cs is not None
    rc, rr, rv = srt(ROut.triplets())
    cc, cr, cv = srt(COut.triplets())
    assert not ROut.IsComplex() and COut.IsComplex()
    assert np.array_equal(rc, cc) and np.array_equal(rr, cr) and same_bits(rv, np.ascontiguousarray(cv.real)) and np.all(cv.imag == 0.0)
    rz, cz = srt(RZout.triplets()), srt(CZout.triplets())
    assert len(rz[0]) > 0 and np.array_equal(rz[0], cz[0]) and np.array_equal(rz[1], cz[1]) and np.all(cz[2] == 0.0)
    assert rs == cs, (rs, cs)


# ------------------------------------------------------------------ refusal, gates
def test_refusal_leaves_everything_as_it_was(nt, fma):
    """one column whose runs in X and X3 lie n / 2 rows apart: the union extent is beyond what the column's three slots and two pads
    bound -- not taken, nothing written, the books unmoved; the same column with X3 beside X is taken"""
    n, j = 4099, 5
    col = lambda f, l: {j: (np.arange(f, l + 1), cpx(np.linspace(0.1, 0.9, l - f + 1), np.linspace(-0.7, 0.2, l - f + 1)))}
    MX, M2, M3 = _matrix(nt, col(0, 9), n=n), _matrix(nt, col(0, 9), n=n), _matrix(nt, col(n // 2 + 1, n // 2 + 11), n=n)
    MZ, Out, Zout = nt.Matrix_ps(n), nt.Matrix_ps(n), nt.Matrix_ps(n)
    before = [srt(m.triplets()) for m in (MX, M2, M3)]
    b0 = books(nt)
    assert nt.pm_fused_step(MX, MZ, M2, M3, 0.5, 1.5, -1.0, 0.0, Out, Zout) is None
    assert books(nt) == b0
    for m, b in zip((MX, M2, M3), before):
        assert all(same_bits(p, q) for p, q in zip(srt(m.triplets()), b))
    assert len(Out.triplets()[2]) == 0 and len(Zout.triplets()[2]) == 0 and len(MZ.triplets()[2]) == 0
    # the same column with X3 beside X is taken (FMA arithmetic)
    M3 = _matrix(nt, col(4, 20), n=n)
    got = nt.pm_fused_step(MX, MZ, M2, M3, 0.5, 1.5, -1.0, 0.0, Out, Zout)
    if not fma:
        assert got is None and books(nt) == b0
        return
    assert got is not None and len(Out.triplets()[2]) == 21


def test_gates_of_the_diagnostic(nt, fma, operands):
    """complex_pm = 0: complex operands are not taken and no counter moves; mixed kinds are not taken; real operands give the bits and
    the pm_session counts with complex_pm = 1 that they give with 0"""
    X, X2, X3, Z = operands
    a1, a2, a3 = coefficients(0.7)
    MX, M2, M3, MZ = _matrix(nt, X), _matrix(nt, X2), _matrix(nt, X3), _pattern_matrix(nt, Z)
    R2 = _matrix(nt, X2, real=True)
    Out, Zout = nt.Matrix_ps(N), nt.Matrix_ps(N)
    s0, b0 = nt.slab_algebra_counts(), books(nt)
    nt.set_option("complex_pm", 0)
    assert nt.pm_fused_step(MX, MZ, M2, M3, a1, a2, a3, 1e-3, Out, Zout) is None
    nt.set_option("complex_pm", 1)
    assert nt.pm_fused_step(MX, MZ, R2, M3, a1, a2, a3, 1e-3, Out, Zout) is None, "mixed kinds"
    assert books(nt) == b0 and nt.slab_algebra_counts() == s0
    assert len(Out.triplets()[2]) == 0 and len(Zout.triplets()[2]) == 0
    runs, real_ops = [], _real_file_operands()   # (the complex operands' real parts would store zeros)
    for opt in (0, 1):
        nt.set_option("complex_pm", opt)
        RX, RM2, RM3 = (_matrix(nt, {j: (r, v + 0j) for j, (r, v) in c.items()}, real=True) for c in real_ops[:3])
        RZ = _matrix(nt, {j: (rows, np.ones(len(rows)) + 0j) for j, rows in real_ops[3].items()}, real=True)
        ROut, RZout = nt.Matrix_ps(N), nt.Matrix_ps(N)
        p0 = nt.pm_session_counts()
        sc = nt.pm_fused_step(RX, RZ, RM2, RM3, a1, a2, a3, 1e-3, ROut, RZout)
        runs.append((sc, srt(ROut.triplets()), srt(RZout.triplets()), delta(nt.pm_session_counts(), p0)))
    nt.set_option("complex_pm", 1)
    assert runs[0][0] is not None and runs[0][0] == runs[1][0] and runs[0][3] == runs[1][3]
    assert all(same_bits(p, q) for k in (1, 2) for p, q in zip(runs[0][k], runs[1][k]))
    assert nt.complex_pm_counts() == b0[0]


# ------------------------------------------------------------------ the solver
SOLVE_N, SOLVE_H, SOLVE_THR, SOLVE_ITERS = 512, 10, 1e-8, 14


def pm_solve(nt, nel, opt, trip=None, n=SOLVE_N, iters=SOLVE_ITERS):
    nt.set_option("complex_pm", opt)
    if trip is None:
        trip = banded_triplets(n, SOLVE_H, complex_=True)
    H = nt.Matrix_ps.from_triplets(n, *trip)
    assert H.IsComplex() and len(H.triplets()[2]) == len(trip[2])
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    p = nt.SolverParameters()
    p.SetThreshold(SOLVE_THR)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(iters)
    p.SetMonitorConvergence(False)
    K = nt.Matrix_ps(n)
    c0, r0, s0 = nt.complex_pm_counts(), nt.pm_session_counts(), nt.slab_algebra_counts()
    e = nt.DensityMatrixSolvers.PM(H, I, float(nel), K, p)
    c1, r1, s1 = nt.complex_pm_counts(), nt.pm_session_counts(), nt.slab_algebra_counts()
    tr = nt.solver_trace()
    return dict(K=srt(K.triplets()), e=e[0] if isinstance(e, tuple) else e, iters=tr["iterations"], nnz=np.asarray(tr["nnz"]).copy(),
                sigma=np.asarray(tr["sigma"]).copy(), energy=np.asarray(tr["energy"]).copy(), counts=delta(c1, c0),
                real_counts=delta(r1, r0), products=s1["products"] - s0["products"])


def bit_equal(a, b):
    return (a["iters"] == b["iters"] and np.array_equal(a["nnz"], b["nnz"]) and same_bits(a["sigma"], b["sigma"]) and
            same_bits(a["energy"], b["energy"]) and all(same_bits(p, q) for p, q in zip(a["K"], b["K"])))


def density_difference(a, b, n):
    import scipy.sparse as sp
    G = sp.csr_matrix((a["K"][2], (a["K"][1] - 1, a["K"][0] - 1)), shape=(n, n))
    W = sp.csr_matrix((b["K"][2], (b["K"][1] - 1, b["K"][0] - 1)), shape=(n, n))
    D = abs(G - W)
    return D.max() if D.nnz else 0.0


@pytest.mark.parametrize("nel", [128, 256, 384])
def test_solver_in_slab_form(nt, fma, nel):
    """banded_triplets(512, 10, complex_=True), thr 1e-8, 14 iterations, ISQ = I: sigma stays below 1/2 (nel 128), above it (384),
    crosses it (256).  Option 1 against option 0: iteration counts, sigma > 1/2 decisions and nnz traces equal, sigma to 1e-10,
    energies to 1e-10 relative, densities to 1e-9 (the bounds test_solver_in_slab_form of tests/test_gpu_pm_session.py holds the
    real path to); pm_session_counts never moves.  Unfused arithmetic: a gate -- option 1 is option 0 bit for bit"""
    off = pm_solve(nt, nel, 0)
    on = pm_solve(nt, nel, 1)
    assert off["counts"] == NONE == off["real_counts"] == on["real_counts"] and off["products"] == 0
    if not fma:
        assert on["counts"] == NONE and on["products"] == 0 and bit_equal(on, off)
        return
    dk = density_difference(on, off, SOLVE_N)
    print("nel", nel, "sigma", on["sigma"], "counts on", on["counts"], "products", on["products"])
    print("nnz on ", on["nnz"].tolist())
    print("nnz off", off["nnz"].tolist())
    print("max differences: sigma", np.max(np.abs(on["sigma"] - off["sigma"])), "energy (relative)",
          np.max(np.abs(on["energy"] - off["energy"]) / np.abs(off["energy"])), "density", dk)
    assert on["iters"] == off["iters"] == SOLVE_ITERS
    assert np.array_equal(on["sigma"] > 0.5, off["sigma"] > 0.5)
    assert np.array_equal(on["nnz"], off["nnz"])
    assert np.max(np.abs(on["sigma"] - off["sigma"])) <= 1e-10
    assert np.all(np.abs(on["energy"] - off["energy"]) <= 1e-10 * np.abs(off["energy"]))
    assert dk <= 1e-9
    assert on["counts"]["updates"] >= 13 and on["counts"]["left"] == 0 and on["products"] >= 26, (on["counts"], on["products"])
    if nel == 128:
        assert on["counts"]["zeros"] == 0
    else:
        assert on["counts"]["zeros"] > 0


def test_starting_iterate_with_a_stored_zero_leaves_the_fused_path(nt, fma):
    """a complex Hamiltonian that stores a zero off its diagonal: the starting iterate stores it too, its slab form is a read-only
    view, and the first sigma pass refuses -- the iterate is materialised, the session closed, the solve finishes on compressed
    columns (once: left == 1, nothing fused) with the entry counts of option 0 and its density to 1e-9"""
    col, row, val = banded_triplets(SOLVE_N, SOLVE_H, complex_=True)
    val = val.copy()
    val[(col == 101) & (row == 104)] = 0.0
    val[(col == 104) & (row == 101)] = 0.0
    off = pm_solve(nt, 256, 0, trip=(col, row, val))
    on = pm_solve(nt, 256, 1, trip=(col, row, val))
    print("counts", on["counts"], "products", on["products"])
    assert on["real_counts"] == NONE == off["real_counts"] == off["counts"]
    if not fma:
        assert on["counts"] == NONE and bit_equal(on, off)
        return
    assert on["counts"] == dict(sigma=0, updates=0, zeros=0, left=1), on["counts"]
    assert on["iters"] == off["iters"] and np.array_equal(on["nnz"], off["nnz"])
    assert np.max(np.abs(on["sigma"] - off["sigma"])) <= 1e-10
    assert density_difference(on, off, SOLVE_N) <= 1e-9


def hermitian(trip, phase=0.1):
    """a Hermitian complex operand with the pattern and |values| of a real symmetric one: H(r, c) = v exp(i phase (r - c))"""
    c, r, v = trip
    return c, r, v * np.exp(1j * phase * (r.astype(np.float64) - c.astype(np.float64)))


def test_a_complex_lattice_stays_in_block_form(nt, fma):
    """an operand without runs: inside the complex session the products leave complex block form, which the fused passes leave alone
    (a gate, not a refusal): the complex PM counters do not move and the density has option 0's bits"""
    L = 12
    n = L ** 3
    trip = hermitian(lattice_triplets(L))
    nt.set_option("block_path", 2)
    nt.set_option("block_complex", 1)
    on = pm_solve(nt, n / 2.0, 1, trip=trip, n=n, iters=8)
    off = pm_solve(nt, n / 2.0, 0, trip=trip, n=n, iters=8)
    print("counts", on["counts"], off["counts"], "iterations", on["iters"], off["iters"])
    assert on["counts"] == NONE == off["counts"] and on["real_counts"] == NONE == off["real_counts"]
    assert on["iters"] == off["iters"] and np.array_equal(on["nnz"], off["nnz"])
    assert all(same_bits(p, q) for p, q in zip(on["K"], off["K"]))
