"""Operands and exact references of the scalar-reduction tests (tests/test_scalar_reference_cpu.py,
tests/test_gpu_scalar_forms.py and its worker tests/scalar_forms_worker.py).  numpy and the standard library only, no engine
import: the worker and the tests import this module, so all of them see the same bytes.

Every operand is generated WHOLE from the case's seed and returned as column-major sorted 1-based triplets (col, row, val).

Integer family.  Real values are non-zero integers of modulus <= 8.  Complex values are Gaussian integers whose modulus is an
integer: axis-aligned entries of modulus <= 8, or (3, 4), (5, 12), (8, 15) with the parts swapped and signed at random (moduli
5, 13, 17).  Every product, partial sum, column sum, d +- r is an integer far below 2^53 (INT_SUM_LIMIT), so it is exact in
binary64 in any order, fused or not, in double or double-double: the contract is EQUALITY with int64 arithmetic.  1 / (N N) is
one correctly rounded division of exact operands on either side.  Products of two such matrices are integer matrices too.

Real family.  Moduli uniform in [0.5, 1), random signs; a complex value has its argument in [pi/8, 3 pi/8] before the signs, so
both parts are at least 0.19.  The reference of a sum of products is the correctly rounded exact value: Veltkamp / Dekker
two-product, then math.fsum over all high and low parts.  A sum of k rounded terms in any order satisfies
|error| <= 1.01 (k + 1) 2^-53 sum |term| (the gamma_(k-1) bound of the additions plus one rounding per term): bound().  Column
sums of moduli (Norm, MeasureAsymmetry): the terms of a real operand are exact; a complex modulus comes from hypot, documented
at 1 ulp = two roundings, so k + 1 becomes k + 2: bound(k, s, 2).  Gershgorin: with R the exact radius and d the diagonal, both
ends lie within 2^-52 (|d| + R) of d -+ R (the double-double claim of k_colstat / k_sa_colstat).

Shapes (the constants of csrc/kernels.hip they are derived from are quoted below): mixed, long, partials, strided.
"""
import math

import numpy as np

U = 2.0 ** -53
# ---- the constants of the kernels the shapes are derived from (csrc/kernels.hip)
DOT_WINDOW = 1024            # k_dot: W, the LDS window over the row span of a column of B; also the most row ids the LDS search holds
DOT_PRELOAD = 5 * 64         # k_dot: CH * WAVE entries preloaded per column, tail loops behind them
DOT_GRID_COLUMNS = 32768     # dot(): 8192 blocks of 4 waves; a wave takes a second column beyond this many
REDUCE_ONE_STAGE = 8192      # reduce_sum2_async / the min-max reduction: one stage up to this many columns
REDUCE_CHUNK = 2048          # ... chunks of this many partials above it
STRIDED_COLUMNS = 262144     # k_trace / the min-max reduction: 1024 blocks of 256 threads; a strided pass beyond
INT_SUM_LIMIT = 2 ** 53

N_MIXED, N_LONG, N_PARTIALS, N_STRIDED = 1500, 33000, 10500, STRIDED_COLUMNS + 300
KINDS = ("band", "scatter40", "s700", "wide1100", "e400", "e10", "empty", "full")
PYTHAGOREAN = ((3, 4), (5, 12), (8, 15))


# ------------------------------------------------------------------ values
def values(rng, k, family, cplx, size="any"):
    """k stored values of the family; size 'small' / 'large' (integer family): the regular columns of a case with designated
    extreme columns draw small moduli (real <= 4, complex <= 5), the extreme columns large ones (real 7, 8; complex 13, 17)"""
    sign = lambda: rng.choice((-1.0, 1.0), k)     # noqa: E731
    if family == "real":
        m = rng.uniform(0.5, 1.0, k)
        if not cplx:
            return m * sign()
        th = rng.uniform(np.pi / 8, 3 * np.pi / 8, k)
        return m * np.cos(th) * sign() + 1j * (m * np.sin(th) * sign())
    lo, hi = {"any": (1, 9), "small": (1, 5), "large": (7, 9)}[size]
    if not cplx:
        return rng.integers(lo, hi, k).astype(np.float64) * sign()
    axis = rng.integers(lo, hi, k).astype(np.float64) * sign()
    pairs = np.array({"any": PYTHAGOREAN, "small": PYTHAGOREAN[:1], "large": PYTHAGOREAN[1:]}[size], dtype=np.float64)
    pick = pairs[rng.integers(0, len(pairs), k)]
    swap = rng.random(k) < 0.5
    px = np.where(swap, pick[:, 1], pick[:, 0]) * sign()
    py = np.where(swap, pick[:, 0], pick[:, 1]) * sign()
    on_axis = rng.random(k) < (0.0 if size == "large" else 0.5)
    imag_axis = rng.random(k) < 0.5
    re = np.where(on_axis, np.where(imag_axis, 0.0, axis), px)
    im = np.where(on_axis, np.where(imag_axis, axis, 0.0), py)
    return re + 1j * im


# ------------------------------------------------------------------ patterns (0-based inside, 1-based triplets outside)
def band_pattern(n, h):
    j = np.repeat(np.arange(n, dtype=np.int64), 2 * h + 1)
    r = j + np.tile(np.arange(-h, h + 1, dtype=np.int64), n)
    ok = (r >= 0) & (r < n)
    return j[ok], r[ok]


def replace_columns(col, row, special):
    """the pattern with the columns named in `special` ({column: rows}) replaced"""
    keep = ~np.isin(col, np.fromiter(special.keys(), dtype=np.int64, count=len(special)))
    cols = [col[keep]] + [np.full(len(r), j, dtype=np.int64) for j, r in special.items()]
    rows = [row[keep]] + [np.asarray(r, dtype=np.int64) for r in special.values()]
    col, row = np.concatenate(cols), np.concatenate(rows)
    order = np.lexsort((row, col))
    return col[order], row[order]


def finish(rng, n, col, row, family, cplx, large=(), diag_sign=None):
    """values on a pattern: the columns in `large` draw large moduli and all others small ones (none given: any); diag_sign
    {column: +1 / -1}: the sign of the real part of that column's diagonal entry"""
    if len(large):
        val = values(rng, len(col), family, cplx, "small")
        big = np.isin(col, np.asarray(large, dtype=np.int64))
        val[big] = values(rng, int(big.sum()), family, cplx, "large")
    else:
        val = values(rng, len(col), family, cplx)
    for j, s in (diag_sign or {}).items():
        p = np.flatnonzero((col == j) & (row == j))
        assert len(p) == 1
        v = val[p[0]]
        if cplx and v.real == 0.0:      # (an entry on the imaginary axis has no real part to sign: turn it)
            v = complex(v.imag, 0.0)
        val[p[0]] = (abs(v.real) * s + 1j * v.imag) if cplx else abs(v) * s
    return (col + 1).astype(np.int32), (row + 1).astype(np.int32), val


def kind_rows(rng, kind, j, n, mode):
    """rows of one column of the mixed case.  mode: 'first' (the diagonal is the first entry: rows >= j), 'last' (rows <= j),
    'absent' (no diagonal entry)"""
    lo, hi = {"first": (j, n - 1), "last": (0, j), "absent": (0, n - 1)}[mode]

    def pick(count, a, b):
        a, b = max(a, lo), min(b, hi)
        inner = np.arange(a + 1, b, dtype=np.int64)
        rows = np.concatenate(([a, b], rng.choice(inner, min(count - 2, len(inner)), replace=False)))
        return np.unique(rows)

    if kind == "empty":
        return np.zeros(0, dtype=np.int64)
    if kind == "band":
        rows = np.arange(max(lo, j - 3), min(hi, j + 3) + 1, dtype=np.int64)
    elif kind == "full":
        rows = np.arange(lo, hi + 1, dtype=np.int64)
    elif kind in ("scatter40", "s700", "wide1100"):
        rows = pick({"scatter40": 40, "s700": 700, "wide1100": 1100}[kind], lo, hi)
    elif kind == "e400":
        a = {"first": j, "last": j - 999, "absent": max(0, min(j - 500, n - 1000))}[mode]
        rows = pick(400, a, a + 999)
    else:
        a = {"first": j, "last": j - 59, "absent": max(0, j - 30)}[mode]
        rows = pick(10, a, a + 59)
    return rows[rows != j] if mode == "absent" else rows


def mixed_columns():
    """(column, kind on the A side, kind on the B side, diagonal mode) of the 64 special columns of the mixed case: every
    pair of kinds once; the modes rotate, and a mode decides where the column lies (a first-entry diagonal with a row span
    above 1024 needs a column near the left edge)"""
    out = []
    for i, (ka, kb) in enumerate((a, b) for a in KINDS for b in KINDS):
        mode = ("first", "absent", "last")[i % 3]
        j = {"first": 5 + 13 * (i // 3), "absent": 400 + 30 * (i // 3), "last": 1210 + 13 * (i // 3)}[mode]
        out.append((j, ka, kb, mode))
    return out


def cancelling_partner(t):
    """an operand on (almost) the pattern of t whose dot with t cancels EXACTLY: the entries of a column are paired (p, q) and
    hold conj(t_q) and -conj(t_p), so conj(t_p) conj(t_q) - conj(t_q) conj(t_p) = 0; the odd entry of a column is left out"""
    col, row, val = t
    k = len(col)
    first = np.flatnonzero(np.concatenate(([True], col[1:] != col[:-1])))
    start = np.repeat(first, np.diff(np.concatenate((first, [k]))))
    pos = np.arange(k) - start
    nxt = np.concatenate((col[1:] == col[:-1], [False]))
    p = np.flatnonzero((pos % 2 == 0) & nxt)
    q = p + 1
    out = np.zeros_like(val)
    out[p] = np.conj(val[q])
    out[q] = -np.conj(val[p])
    keep = np.sort(np.concatenate((p, q)))
    return col[keep], row[keep], out[keep]


# ------------------------------------------------------------------ the cases
def _seed(shape, family, cplx):
    return 9100 + 100 * ("mixed", "long", "partials", "strided", "lattice", "panels").index(shape) + 10 * (family == "real") + int(cplx)


def mixed_case(family, cplx):
    n = N_MIXED
    rng = np.random.default_rng(_seed("mixed", family, cplx))
    bc, br = band_pattern(n, 3)
    sa, sb = {}, {}
    for j, ka, kb, mode in mixed_columns():
        sa[j] = kind_rows(rng, ka, j, n, mode)
        sb[j] = kind_rows(rng, kb, j, n, mode)
    A = finish(rng, n, *replace_columns(bc, br, sa), family, cplx)
    B = finish(rng, n, *replace_columns(bc, br, sb), family, cplx)
    ops = {"A": A, "B": B, "Bx": cancelling_partner(A)}
    # the other kind of value on the same patterns: a real operand beside a complex one, in either order
    ops["Ao"] = finish(rng, n, A[0].astype(np.int64) - 1, A[1].astype(np.int64) - 1, family, not cplx)
    return {"id": "mixed-%s-%s" % (family, "c" if cplx else "r"), "shape": "mixed", "n": n, "family": family, "cplx": cplx, "ops": ops,
            "dots": [("A", "B"), ("B", "A"), ("A", "A"), ("A", "Bx"), ("Ao", "B"), ("B", "Ao")], "singles": ["A", "B"]}


def long_case(family, cplx):
    """tridiagonal, n = 33 000; beyond column 32 768 (the waves that reach them are on their second column) the wide kinds face
    each other: a span above 1024 with 40 entries, 1100 entries, 400 entries against 10"""
    n = N_LONG
    rng = np.random.default_rng(_seed("long", family, cplx))
    bc, br = band_pattern(n, 1)
    cols = (32800, 32850, 32900, 32950)
    ka = ("scatter40", "wide1100", "e400", "e10")
    kb = ("wide1100", "scatter40", "e10", "e400")

    def rows(kind, j):
        """a stretch of 2000 rows around the column (a span above 1024) for the wide kinds, of 1000 or 60 for the others"""
        cnt, w = {"scatter40": (40, 1000), "wide1100": (1100, 1000), "e400": (400, 500), "e10": (10, 30)}[kind]
        a, b = j - w, min(n - 1, j + w - 1)
        return np.unique(np.concatenate(([a, j, b], rng.choice(np.arange(a + 1, b), cnt - 3, replace=False))))

    sa = {j: rows(k, j) for j, k in zip(cols, ka)}
    sb = {j: rows(k, j) for j, k in zip(cols, kb)}
    A = finish(rng, n, *replace_columns(bc, br, sa), family, cplx)
    B = finish(rng, n, *replace_columns(bc, br, sb), family, cplx)
    return {"id": "long-%s-%s" % (family, "c" if cplx else "r"), "shape": "long", "n": n, "family": family, "cplx": cplx,
            "ops": {"A": A, "B": B}, "dots": [("A", "B"), ("B", "A")], "singles": ["A", "B"], "special": cols}


PARTIALS_EXTREME = (0, REDUCE_ONE_STAGE - 1, REDUCE_ONE_STAGE, N_PARTIALS - 1)


def partials_case(family, cplx):
    """band of half width 40, n = 10 500 (more than 8192 columns, no multiple of 2048): operands P0 .. P3 whose Norm column and
    both Gershgorin extremes are ONE column of 200 entries (large moduli in the integer family) at index 0, 8191, 8192, n - 1;
    Q: runs [j + 10, j + 90] (partly over the band's), [j + 50, j + 130] (disjoint from it) and the band's own in turn, column
    5000 empty"""
    n = N_PARTIALS
    rng = np.random.default_rng(_seed("partials", family, cplx))
    bc, br = band_pattern(n, 40)
    ops = {}
    for k, j in enumerate(PARTIALS_EXTREME):
        a = min(max(0, j - 100), n - 200)
        col, row = replace_columns(bc, br, {j: np.arange(a, a + 200, dtype=np.int64)})
        ops["P%d" % k] = finish(rng, n, col, row, family, cplx, large=(j,) if family == "int" else ())
    j = np.arange(n, dtype=np.int64)
    lo = np.where(j % 3 == 0, j + 10, np.where(j % 3 == 1, j + 50, j - 40))
    hi = np.where(j % 3 == 0, j + 90, np.where(j % 3 == 1, j + 130, j + 40))
    valid = (lo <= n - 1) & (j != 5000)
    lo, hi = np.maximum(lo, 0), np.minimum(hi, n - 1)
    cnt = np.where(valid, hi - lo + 1, 0)
    qc = np.repeat(j, cnt)
    qr = np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    ops["Q"] = finish(rng, n, qc, qr, family, cplx)
    return {"id": "partials-%s-%s" % (family, "c" if cplx else "r"), "shape": "partials", "n": n, "family": family, "cplx": cplx, "ops": ops,
            "dots": [("P0", "P1"), ("P2", "P3"), ("P0", "Q"), ("Q", "P1")], "singles": ["P0", "P1", "P2", "P3", "Q"]}


STRIDED_SPECIAL = {"hi": STRIDED_COLUMNS + 50, "lo": STRIDED_COLUMNS + 150, "absent": STRIDED_COLUMNS + 250}


def strided_case(cplx):
    """tridiagonal, n = 262 144 + 300, integer family: beyond column 262 144 a column of large moduli with a positive diagonal
    (the Norm column or its equal, the upper Gershgorin end), one with a negative diagonal (the lower end) and a column
    without a diagonal entry"""
    n = N_STRIDED
    rng = np.random.default_rng(_seed("strided", "int", cplx))
    bc, br = band_pattern(n, 1)
    s = STRIDED_SPECIAL
    col, row = replace_columns(bc, br, {s["absent"]: np.array([s["absent"] - 1, s["absent"] + 1])})
    A = finish(rng, n, col, row, "int", cplx, large=(s["hi"], s["lo"]), diag_sign={s["hi"]: 1, s["lo"]: -1})
    B = finish(rng, n, bc, br, "int", cplx)
    return {"id": "strided-int-%s" % ("c" if cplx else "r"), "shape": "strided", "n": n, "family": "int", "cplx": cplx,
            "ops": {"A": A, "B": B}, "dots": [("A", "B")], "singles": ["A"]}


PANEL_BAND = 5


def panel_operands(world):
    """the banded integer operands of the slab-panel runs (n = 1500, half width 5, real): 'up' has its upper Gershgorin end in
    a column of large moduli with a positive diagonal inside the LAST panel of `world` ranks, 'down' its lower end in such a
    column with a negative diagonal inside the second panel; each misses the diagonal entry of a column of that panel"""
    n = N_MIXED
    rng = np.random.default_rng(_seed("panels", "int", False) + world)
    bc, br = band_pattern(n, PANEL_BAND)
    b = [n * r // world for r in range(world + 1)]
    out = {}
    for name, panel, s in (("up", world - 1, 1), ("down", 1, -1)):
        ext, gone = b[panel] + 37, b[panel] + 91
        col, row = replace_columns(bc, br, {gone: np.array([r for r in range(gone - PANEL_BAND, gone + PANEL_BAND + 1) if r != gone])})
        out[name] = (finish(rng, n, col, row, "int", False, large=(ext,), diag_sign={ext: s}), ext, gone)
    return out


def lattice_values(family_seed, k, cplx):
    """integer values for the k entries of a lattice pattern (tests/gen.py lattice_triplets), moduli small enough for a product"""
    rng = np.random.default_rng(_seed("lattice", "int", cplx) + family_seed)
    return values(rng, k, "int", cplx)


_CACHE = {}


def case(shape, family, cplx):
    key = (shape, family, cplx)
    if key not in _CACHE:
        _CACHE[key] = {"mixed": mixed_case, "long": long_case, "partials": partials_case}[shape](family, cplx) if shape != "strided" else strided_case(cplx)
    return _CACHE[key]


CASE_TABLE = [(s, f, c) for s in ("mixed", "long", "partials") for f in ("int", "real") for c in (False, True)] + [("strided", "int", False), ("strided", "int", True)]


# ------------------------------------------------------------------ references
def keys(t, n):
    return (t[0].astype(np.int64) - 1) * n + (t[1].astype(np.int64) - 1)


def matched(ta, tb, n):
    """positions in ta and tb of the entries both hold"""
    _, ia, ib = np.intersect1d(keys(ta, n), keys(tb, n), assume_unique=True, return_indices=True)
    return ia, ib


def dot_factors(ta, tb, n):
    """sum conj(a) b as sums of real products: ([(x, y), ...] of the real part, [...] of the imaginary part)"""
    ia, ib = matched(ta, tb, n)
    a, b = ta[2][ia], tb[2][ib]
    ar, br = np.real(a).astype(np.float64), np.real(b).astype(np.float64)
    re, im = [(ar, br)], []
    ca, cb = np.iscomplexobj(a), np.iscomplexobj(b)
    if ca and cb:
        re.append((np.imag(a), np.imag(b)))
    if cb:
        im.append((ar, np.imag(b)))
    if ca:
        im.append((-np.imag(a), br))
    return re, im


def dot_int(ta, tb, n):
    """(re, im) of sum conj(a) b in int64"""
    re, im = dot_factors(ta, tb, n)
    tot = lambda fs: int(sum(int((np.rint(x).astype(np.int64) * np.rint(y).astype(np.int64)).sum()) for x, y in fs))   # noqa: E731
    return tot(re), tot(im)


def two_product(x, y):
    """x y = p + e exactly (Veltkamp split, Dekker product)"""
    p = x * y
    cx, cy = 134217729.0 * x, 134217729.0 * y
    xh, yh = cx - (cx - x), cy - (cy - y)
    xl, yl = x - xh, y - yh
    e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    return p, e


def bound(k, sum_abs, roundings=1):
    """|error| of a sum of k terms, each carrying `roundings` roundings, in any order"""
    return 1.01 * (k + roundings) * U * sum_abs


def fsum_products(factors):
    """(correctly rounded exact sum, number of terms, sum of |term|, smallest |term|) of sum x y over the pairs of arrays"""
    parts, k, sabs, least = [], 0, 0.0, math.inf
    for x, y in factors:
        p, e = two_product(x, y)
        parts.extend(p.tolist())
        parts.extend(e.tolist())
        k += len(p)
        sabs += float(np.abs(p).sum())
        if len(p):
            least = min(least, float(np.abs(p).min()))
    return math.fsum(parts), k, sabs, least


def dot_real(ta, tb, n):
    """((re, im), (bound of re, bound of im)) of sum conj(a) b, real family"""
    re, im = dot_factors(ta, tb, n)
    (vr, kr, sr, _), (vi, ki, si, _) = fsum_products(re), fsum_products(im)
    return (vr, vi), (bound(kr, sr), bound(ki, si))


def diagonal(t):
    d = t[0] == t[1]
    return t[0][d], np.real(t[2][d]).astype(np.float64)


def trace_int(t):
    return int(np.rint(diagonal(t)[1]).astype(np.int64).sum())


def trace_real(t):
    d = diagonal(t)[1]
    return math.fsum(d.tolist()), bound(len(d), float(np.abs(d).sum()))


def moduli(val):
    """(hi, lo): the modulus of every value as an unevaluated sum, |v| = hi + lo to about 2^-100"""
    if not np.iscomplexobj(val):
        return np.abs(val), np.zeros(len(val))
    x, y = np.real(val).copy(), np.imag(val).copy()
    m = np.hypot(x, y)
    (px, ex), (py, ey), (pm, em) = two_product(x, x), two_product(y, y), two_product(m, m)
    resid = np.array([math.fsum(q) for q in zip(px, ex, py, ey, -pm, -em)]) if len(m) else np.zeros(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        lo = np.where(m > 0, resid / (2.0 * m), 0.0)
    return m, lo


def int_moduli(val):
    m = np.rint(np.hypot(np.real(val), np.imag(val))).astype(np.int64)
    return m


def norm_int(t, n):
    return int(np.bincount(t[0].astype(np.int64) - 1, weights=int_moduli(t[2]).astype(np.float64), minlength=n).max()) if len(t[0]) else 0


def _exact_column_sums(t, cols):
    """{column (1-based): (exact sum of moduli correctly rounded, entries)} of the given columns"""
    out = {}
    for c in cols:
        sel = t[0] == c
        hi, lo = moduli(t[2][sel])
        out[int(c)] = (math.fsum(hi.tolist() + lo.tolist()), int(sel.sum()))
    return out


def norm_real(t, n):
    """(max column sum of moduli, bound): the exact sums of the columns within 1e-9 of the largest approximate sum"""
    approx = np.bincount(t[0].astype(np.int64) - 1, weights=np.abs(t[2]), minlength=n)
    cand = np.flatnonzero(approx >= approx.max() * (1 - 1e-9)) + 1
    sums = _exact_column_sums(t, cand)
    best = max(sums.values())
    return best[0], bound(max(k for _, k in sums.values()), best[0], 2 if np.iscomplexobj(t[2]) else 1)


def gershgorin_int(t, n):
    col = t[0].astype(np.int64) - 1
    off = t[0] != t[1]
    r = np.bincount(col[off], weights=int_moduli(t[2][off]).astype(np.float64), minlength=n)
    d = np.zeros(n)
    dc, dv = diagonal(t)
    d[dc.astype(np.int64) - 1] = dv
    return int((d - r).min()), int((d + r).max())


def gershgorin_real(t, n):
    """((lo, hi), (tolerance of lo, of hi)): the correctly rounded d - R and d + R of the extreme columns, 2^-52 (|d| + R)"""
    col = t[0].astype(np.int64) - 1
    off = t[0] != t[1]
    r = np.bincount(col[off], weights=np.abs(t[2][off]), minlength=n)
    d = np.zeros(n)
    dc, dv = diagonal(t)
    d[dc.astype(np.int64) - 1] = dv
    toff = tuple(x[off] for x in t)
    out = []
    for ends, s in ((d - r, -1.0), (d + r, 1.0)):
        ext = ends.min() if s < 0 else ends.max()
        cand = np.flatnonzero(np.abs(ends - ext) <= 1e-9 * max(1.0, abs(ext)))
        best = None
        for c in cand:
            hi, lo = moduli(toff[2][toff[0] == c + 1])
            R = math.fsum(hi.tolist() + lo.tolist())
            v = math.fsum([d[c]] + (s * hi).tolist() + (s * lo).tolist())
            if best is None or (v < best[0] if s < 0 else v > best[0]):
                best = (v, 2.0 ** -52 * (abs(d[c]) + R))
        out.append(best)
    return (out[0][0], out[1][0]), (out[0][1], out[1][1])


def asymmetry_operand(t, n):
    """the entries of A^H - A as the engine forms them: one rounded subtraction per part (exact in the integer family), so its
    column sums of moduli are MeasureAsymmetry"""
    k = keys(t, n)
    kt = (t[1].astype(np.int64) - 1) * n + (t[0].astype(np.int64) - 1)
    allk = np.concatenate((kt, k))
    uniq, inv = np.unique(allk, return_inverse=True)
    first = np.zeros(len(uniq), dtype=t[2].dtype)
    second = np.zeros(len(uniq), dtype=t[2].dtype)
    first[inv[:len(k)]] = np.conj(t[2])
    second[inv[len(k):]] = t[2]
    diff = first - second
    return (uniq // n + 1).astype(np.int32), (uniq % n + 1).astype(np.int32), diff


def sigma_int(t, n):
    nrm = float(norm_int(t, n))
    return 1.0 / (nrm * nrm)


def sigma_real(t, n):
    """1 / (N N): twice the relative bound of N, the rounding of the product and of the quotient on either side"""
    nrm, b = norm_real(t, n)
    s = 1.0 / (nrm * nrm)
    return s, s * 1.01 * (2.0 * b / nrm + 4.0 * U)


def dense(t, n):
    D = np.zeros((n, n), dtype=t[2].dtype)
    D[t[1].astype(np.int64) - 1, t[0].astype(np.int64) - 1] = t[2]
    return D


def from_dense(D):
    c, r = np.nonzero(D.T)
    return (c + 1).astype(np.int32), (r + 1).astype(np.int32), np.ascontiguousarray(D.T[c, r])


def relabelled(t, n, perm):
    """the matrix under the symmetric permutation: entry (i, j) moves to (perm[i], perm[j])"""
    c, r = perm[t[0].astype(np.int64) - 1], perm[t[1].astype(np.int64) - 1]
    order = np.lexsort((r, c))
    return (c[order] + 1).astype(np.int32), (r[order] + 1).astype(np.int32), t[2][order]


def split_for_rank(t, c0, c1):
    """the triplets of the columns (c0, c1] (1-based)"""
    sel = (t[0] > c0) & (t[0] <= c1)
    return t[0][sel], t[1][sel], t[2][sel]
