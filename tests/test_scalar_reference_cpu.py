"""CPU: the references of the scalar-reduction tests (tests/scalar_reference.py) checked against exact rational arithmetic, and
the case table checked for what it promises -- the column kinds of every code path of k_dot, the extreme columns at the indices
where the reductions change stage, bounds that a single dropped entry exceeds."""
import math
from fractions import Fraction

import numpy as np
import pytest

import scalar_reference as R

REAL_CASES = [k for k in R.CASE_TABLE if k[1] == "real"]
INT_CASES = [k for k in R.CASE_TABLE if k[1] == "int"]


def ident(key):
    return "%s-%s-%s" % (key[0], key[1], "c" if key[2] else "r")


def test_two_product_and_fsum_dot_equal_rational_arithmetic():
    c = R.case("mixed", "real", True)
    n = c["n"]
    ta, tb = c["ops"]["A"], c["ops"]["B"]
    ia, ib = R.matched(ta, tb, n)
    sub = np.arange(0, len(ia), max(1, len(ia) // 400))[:400]
    sa = tuple(x[ia[sub]] for x in ta)
    sb = tuple(x[ib[sub]] for x in tb)
    (re, im), _ = R.dot_real(sa, sb, n)
    fre = sum((Fraction(float(a.real)) * Fraction(float(b.real)) + Fraction(float(a.imag)) * Fraction(float(b.imag)) for a, b in zip(sa[2], sb[2])), Fraction(0))
    fim = sum((Fraction(float(a.real)) * Fraction(float(b.imag)) - Fraction(float(a.imag)) * Fraction(float(b.real)) for a, b in zip(sa[2], sb[2])), Fraction(0))
    assert len(sa[2]) >= 300
    assert re == float(fre) and im == float(fim)
    x, y = np.real(sa[2]).copy(), np.imag(sb[2]).copy()
    p, e = R.two_product(x, y)
    assert all(Fraction(float(a)) * Fraction(float(b)) == Fraction(float(q)) + Fraction(float(r)) for a, b, q, r in zip(x, y, p, e))


def test_moduli_are_double_doubles_of_the_exact_modulus():
    v = R.values(np.random.default_rng(5), 200, "real", True)
    hi, lo = R.moduli(v)
    for z, h, l in zip(v, hi, lo):
        m2 = Fraction(float(z.real)) ** 2 + Fraction(float(z.imag)) ** 2
        m = Fraction(float(h)) + Fraction(float(l))
        assert abs(m * m - m2) <= m2 * Fraction(1, 2 ** 95)
    assert np.array_equal(R.moduli(np.array([-3.0, 4.0]))[0], [3.0, 4.0])


@pytest.mark.parametrize("key", INT_CASES, ids=ident)
def test_integer_family_is_exact_in_binary64(key):
    c = R.case(*key)
    worst = 0
    for name, t in c["ops"].items():
        x, y = np.real(t[2]), np.imag(t[2])
        assert np.all(x == np.rint(x)) and np.all(y == np.rint(y)) and np.all((x != 0) | (y != 0)), name
        m = R.int_moduli(t[2])
        assert np.array_equal(m * m, (x * x + y * y).astype(np.int64)), name      # the modulus is an integer
        assert m.max() <= (17 if np.iscomplexobj(t[2]) else 8), name
        worst = max(worst, len(t[2]))
    # the largest possible sum: every entry matched, every product 17 * 17
    assert worst * 17 * 17 < R.INT_SUM_LIMIT
    # a product of two lattice operands (203 entries per row), summed against a third over 1728^2 entries
    assert 1728 * 1728 * 203 * 17 * 17 * 17 < R.INT_SUM_LIMIT


@pytest.mark.parametrize("key", REAL_CASES, ids=ident)
def test_bounds_are_below_the_smallest_term(key):
    """a dropped, doubled or mis-paired entry moves a sum by a whole term: every bound must be smaller than the smallest one"""
    c = R.case(*key)
    n = c["n"]
    for name, t in c["ops"].items():
        m = np.abs(t[2])
        assert m.min() >= 0.5 and m.max() < 1.0, name
        if np.iscomplexobj(t[2]):
            assert min(np.abs(t[2].real).min(), np.abs(t[2].imag).min()) >= 0.5 * math.sin(math.pi / 8) - 1e-12
    for a, b in c["dots"]:
        (re, im), (bre, bim) = R.dot_real(c["ops"][a], c["ops"][b], n)
        # |conj(a) b| >= 0.25, so one of its parts is at least 0.25 / sqrt(2)
        assert max(bre, bim) < 0.25 / math.sqrt(2.0), (a, b, bre, bim)
        if not (np.iscomplexobj(c["ops"][a][2]) or np.iscomplexobj(c["ops"][b][2])):
            assert bre < 0.25
    for name in c["singles"]:
        t = c["ops"][name]
        least = 0.5 * math.sin(math.pi / 8) if c["cplx"] else 0.5
        assert R.trace_real(t)[1] < least
        assert R.norm_real(t, n)[1] < 0.5
        assert max(R.gershgorin_real(t, n)[1]) < least
    if c["shape"] == "mixed":
        assert R.norm_real(R.asymmetry_operand(c["ops"]["A"], n), n)[1] < 0.5
        s, tol = R.sigma_real(c["ops"]["A"], n)
        assert tol < 1e-6 * s        # (an entry lost from the Norm column moves sigma by 2 * 0.5 / N > 6e-4 relative)


@pytest.mark.parametrize("cplx", [False, True])
def test_the_cancelling_pair_cancels(cplx):
    c = R.case("mixed", "real", cplx)
    re, im = R.dot_factors(c["ops"]["A"], c["ops"]["Bx"], c["n"])
    for fs in (re, im):
        v, k, sabs, _ = R.fsum_products(fs)
        if k:
            assert k > 30000 and abs(v) < 1e-6 * sabs, (v, sabs)
    assert abs(R.fsum_products(re)[0]) == 0.0       # (exactly: a tolerance relative to the result passes nothing but 0)


def profile(t, n):
    """(entries, first row, last row) of every column, 0-based; empty columns: (0, n, -1)"""
    col = t[0].astype(np.int64) - 1
    row = t[1].astype(np.int64) - 1
    cnt = np.bincount(col, minlength=n)
    first = np.full(n, n)
    last = np.full(n, -1)
    np.minimum.at(first, col, row)
    np.maximum.at(last, col, row)
    return cnt, first, last


def dot_path(cnt, first, last, j):
    """the branch of k_dot a column of its second operand takes"""
    if cnt[j] == 0:
        return "empty"
    if last[j] - first[j] + 1 <= R.DOT_WINDOW:
        return "window"
    return "rows" if cnt[j] <= R.DOT_WINDOW else "global"


@pytest.mark.parametrize("family,cplx", [(f, c) for f in ("int", "real") for c in (False, True)])
def test_mixed_case_holds_every_column_kind_on_either_side(family, cplx):
    c = R.case("mixed", family, cplx)
    n = c["n"]
    pa, pb = profile(c["ops"]["A"], n), profile(c["ops"]["B"], n)
    seen = set()
    diag = {"A": set(), "B": set()}
    for j, ka, kb, mode in R.mixed_columns():
        for side, p, kind in (("A", pa, ka), ("B", pb, kb)):
            cnt, first, last = p
            span = last[j] - first[j] + 1
            if kind == "empty":
                assert cnt[j] == 0
                continue
            if kind == "band":
                assert cnt[j] <= 7
            if kind == "scatter40":
                assert span > R.DOT_WINDOW and 38 <= cnt[j] <= 40
            if kind == "s700":
                assert span > R.DOT_WINDOW and R.DOT_PRELOAD < cnt[j] <= R.DOT_WINDOW
            if kind in ("wide1100", "full"):
                assert span > R.DOT_WINDOW and cnt[j] > R.DOT_WINDOW
            if kind == "e400":
                assert span <= R.DOT_WINDOW and cnt[j] > R.DOT_PRELOAD
            if kind == "e10":
                assert span <= R.DOT_WINDOW and cnt[j] <= 10
            t = c["ops"][side]
            rows = t[1][t[0] == j + 1] - 1
            where = "absent" if j not in rows else "first" if rows[0] == j else "last" if rows[-1] == j else "inside"
            assert where == mode or (where == "inside" and mode != "absent"), (j, side, kind, mode, where)
            diag[side].add((kind, where))
        seen.add((ka, dot_path(*pb, j)))
        seen.add(("B:" + kb, dot_path(*pa, j)))        # Dot(B, A): the kinds of B probe the paths of A
    for side in ("", "B:"):
        for kind in R.KINDS:
            for path in ("window", "rows", "global", "empty"):
                assert (side + kind, path) in seen, (side, kind, path)
    for side in ("A", "B"):
        for where in ("absent", "first", "last"):
            assert {k for k, w in diag[side] if w == where} >= {"scatter40", "s700", "wide1100", "e400", "e10", "band"}, (side, where)
    # the last entry of a column on the global-search path has a partner (a match at l == be - 1)
    ia, ib = R.matched(c["ops"]["A"], c["ops"]["B"], n)
    last_of_b = np.flatnonzero(np.concatenate((c["ops"]["B"][0][1:] != c["ops"]["B"][0][:-1], [True])))
    hit = np.intersect1d(ib, last_of_b)
    cols = c["ops"]["B"][0][hit] - 1
    assert any(dot_path(*pb, j) == "global" and pa[0][j] > 0 for j in cols)
    assert any(dot_path(*pb, j) == "rows" and pa[0][j] > 0 for j in cols)


@pytest.mark.parametrize("family,cplx", [(f, c) for f in ("int", "real") for c in (False, True)])
def test_long_case_has_its_wide_columns_on_a_waves_second_column(family, cplx):
    c = R.case("long", family, cplx)
    n = c["n"]
    assert n > R.DOT_GRID_COLUMNS and all(j >= R.DOT_GRID_COLUMNS for j in c["special"])
    pa, pb = profile(c["ops"]["A"], n), profile(c["ops"]["B"], n)
    assert {dot_path(*pb, j) for j in c["special"]} == {"window", "rows", "global"}
    assert {dot_path(*pa, j) for j in c["special"]} == {"window", "rows", "global"}
    assert max(pa[0][j] for j in c["special"]) > R.DOT_WINDOW and any(R.DOT_PRELOAD < pb[0][j] <= R.DOT_WINDOW for j in c["special"])


def extreme_columns(t, n):
    """(column of the largest column sum, of the lower Gershgorin end, of the upper one), 0-based"""
    col = t[0].astype(np.int64) - 1
    m = np.abs(t[2])
    off = t[0] != t[1]
    s = np.bincount(col, weights=m, minlength=n)
    r = np.bincount(col[off], weights=m[off], minlength=n)
    d = np.zeros(n)
    dc, dv = R.diagonal(t)
    d[dc.astype(np.int64) - 1] = dv
    return int(np.argmax(s)), int(np.argmin(d - r)), int(np.argmax(d + r))


@pytest.mark.parametrize("family,cplx", [(f, c) for f in ("int", "real") for c in (False, True)])
def test_partials_case_has_its_extremes_where_the_reduction_changes_stage(family, cplx):
    c = R.case("partials", family, cplx)
    n = c["n"]
    assert n > R.REDUCE_ONE_STAGE and n % R.REDUCE_CHUNK != 0
    for k, j in enumerate(R.PARTIALS_EXTREME):
        assert extreme_columns(c["ops"]["P%d" % k], n) == (j, j, j)
    cp, fp, lp = profile(c["ops"]["P1"], n)
    cq, fq, lq = profile(c["ops"]["Q"], n)
    overlap = np.minimum(lp, lq) - np.maximum(fp, fq) + 1
    assert cq[5000] == 0 and cp[5000] > 0
    assert np.all(cq == np.where(cq > 0, lq - fq + 1, 0)) and np.all(cp == lp - fp + 1)      # runs without holes
    some = cq > 0
    assert (overlap[some] <= 0).sum() > 3000 and ((overlap[some] > 0) & (overlap[some] < 81)).sum() > 3000 and (overlap[some] > 64).sum() > 3000


@pytest.mark.parametrize("cplx", [False, True])
def test_strided_case_has_its_extremes_beyond_the_strided_pass(cplx):
    c = R.case("strided", "int", cplx)
    n, s = c["n"], R.STRIDED_SPECIAL
    assert min(s.values()) >= R.STRIDED_COLUMNS
    nrm, lo, hi = extreme_columns(c["ops"]["A"], n)
    assert nrm in (s["hi"], s["lo"]) and lo == s["lo"] and hi == s["hi"]
    t = c["ops"]["A"]
    assert not np.any((t[0] == s["absent"] + 1) & (t[1] == s["absent"] + 1)) and np.sum(t[0] == s["absent"] + 1) == 2
    assert len(t[2]) <= 800000


@pytest.mark.parametrize("world", [2, 3])
def test_panel_operands_have_their_extremes_off_the_first_panel(world):
    n = R.N_MIXED
    for name, (t, ext, gone) in R.panel_operands(world).items():
        b = [n * r // world for r in range(world + 1)]
        assert ext >= b[1] and gone >= b[1]
        nrm, lo, hi = extreme_columns(t, n)
        assert (hi if name == "up" else lo) == ext
        assert not np.any((t[0] == gone + 1) & (t[1] == gone + 1))
        glo, ghi = R.gershgorin_int(t, n)
        assert (ghi > -glo) if name == "up" else (-glo > ghi)


def test_references_agree_with_dense_numpy_on_a_small_operand():
    rng = np.random.default_rng(11)
    n = 40
    for cplx in (False, True):
        col, row = R.band_pattern(n, 6)
        keep = rng.random(len(col)) < 0.7
        ta = R.finish(rng, n, col[keep], row[keep], "int", cplx)
        keep = rng.random(len(col)) < 0.7
        tb = R.finish(rng, n, col[keep], row[keep], "int", cplx)
        A, B = R.dense(ta, n), R.dense(tb, n)
        d = np.sum(np.conj(A) * B)
        assert R.dot_int(ta, tb, n) == (int(round(d.real)), int(round(np.imag(d))))
        assert R.trace_int(ta) == int(round(np.trace(A).real))
        assert R.norm_int(ta, n) == int(round(np.abs(A).sum(axis=0).max()))
        r = np.abs(A).sum(axis=0) - np.abs(np.diag(A))
        assert R.gershgorin_int(ta, n) == (int(round((np.diag(A).real - r).min())), int(round((np.diag(A).real + r).max())))
        D = R.dense(R.asymmetry_operand(ta, n), n)
        assert np.array_equal(D, np.conj(A).T - A)
        perm = rng.permutation(n)
        P = R.dense(R.relabelled(ta, n, perm), n)
        assert np.array_equal(P[np.ix_(perm, perm)], A)
        assert R.from_dense(A)[2].tolist() == ta[2].tolist()
        tr = R.finish(rng, n, col, row, "real", cplx)
        Ar = R.dense(tr, n)
        (re, im), (bre, bim) = R.dot_real(tr, tr, n)
        assert abs(re - np.sum(np.abs(Ar) ** 2)) <= 1e-12 and abs(im) <= bim + 1e-300
        assert abs(R.norm_real(tr, n)[0] - np.abs(Ar).sum(axis=0).max()) <= 1e-13
        (lo, hi), _ = R.gershgorin_real(tr, n)
        rr = np.abs(Ar).sum(axis=0) - np.abs(np.diag(Ar))
        assert abs(lo - (np.diag(Ar).real - rr).min()) <= 1e-13 and abs(hi - (np.diag(Ar).real + rr).max()) <= 1e-13
