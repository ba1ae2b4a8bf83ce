"""Seeded operands for the tests of the real thin-operand gather kernels (ntpoly_amd/csrc/spgemm_thin.hip k_spgemm_thin,
k_thin_slab_left, k_thin_slab_right) -- numpy only, no engine.  Every generator returns operands as 1-based (col, row, val)
triplets sorted by column then row, exact zeros removed, together with what the case promises about them;
tests/test_thin_cases_cpu.py asserts those promises against the oracle, tests/test_gpu_thin_real_sessions.py and
tests/test_gpu_thin.py multiply the operands on the GPU.

"thin" = at most 8 n entries (kernels.hpp slab_thin_rule); THIN_MAXK = 64 non-zeros of a column of a thin right operand
are what k_thin_slab_right lists in LDS, a 64-row chunk is what thin_store writes or zero-fills at a time."""
import numpy as np

from gen import banded_triplets

THIN_MAXK = 64
CHUNK = 64


def tidy(col, row, val):
    """sorted by column then row, exact zeros removed"""
    col, row, val = np.asarray(col, dtype=np.int64), np.asarray(row, dtype=np.int64), np.asarray(val)
    k = val != 0
    col, row, val = col[k], row[k], val[k]
    o = np.lexsort((row, col))
    return col[o].astype(np.int32), row[o].astype(np.int32), val[o]


def per_column(t, n):
    """entries per column, index 1 .. n (index 0 unused)"""
    return np.bincount(t[0], minlength=n + 1)


def wide_operand(n, h, empty_cols=(), cplx=False):
    c, r, v = banded_triplets(n, h, complex_=cplx, shift=0.37)
    k = ~np.isin(c, np.asarray(empty_cols, dtype=np.int64))
    return tidy(c[k], r[k], v[k])


def thin_values(col, row, rng, cplx):
    v = np.where(col == row, 1.0, 0.05 * rng.choice([-1.0, 1.0], len(col))) * rng.uniform(0.5, 1.5, len(col))
    if cplx:
        v = v * (1.0 + 1j * rng.uniform(-0.7, 0.7, len(col)))
    return v


def thin_operand(n, seed, empty_rows=(), columns=None, full_diagonal=False, cplx=False):
    """a diagonal with 2 % of its entries dropped (none with full_diagonal) plus entries within reach <= 4 of it, about 3 per
    column; columns: {column: rows} -- those columns list exactly these rows"""
    rng = np.random.default_rng(seed)
    j = np.arange(1, n + 1, dtype=np.int64)
    keep = np.ones(n, dtype=bool) if full_diagonal else rng.random(n) >= 0.02
    cols, rows = [j[keep]], [j[keep]]
    for _ in range(2):
        off = rng.integers(1, 5, n) * rng.choice([-1, 1], n)
        ok = (j + off >= 1) & (j + off <= n) & (rng.random(n) < 0.9)
        cols.append(j[ok])
        rows.append((j + off)[ok])
    col, row = np.concatenate(cols), np.concatenate(rows)
    if columns:
        k = ~np.isin(col, np.asarray(list(columns), dtype=np.int64))
        col, row = col[k], row[k]
        for cj, rj in columns.items():
            col = np.concatenate([col, np.full(len(rj), cj, dtype=np.int64)])
            row = np.concatenate([row, np.asarray(rj, dtype=np.int64)])
    key = np.unique(col * (n + 1) + row)
    col, row = key // (n + 1), key % (n + 1)
    k = ~np.isin(row, np.asarray(empty_rows, dtype=np.int64))
    col, row = col[k], row[k]
    return tidy(col, row, thin_values(col, row, rng, cplx))


# ------------------------------------------------------------------ base case
BASE_SHAPES = [(1003, 20), (2048, 70)]      # no multiple of 4, 16 or 64; block windows of more than 128 rows
BASE_SCALARS = [(-0.5, 1e-7), (1.0, 0.0)]   # (alpha, threshold)


def base_case(n, h):
    """promises: thin holds at most 8 n entries, wide more; columns 1, 17, 500, n of wide are empty, rows 3, 64, 700, n - 1 of thin"""
    empty_cols, empty_rows = (1, 17, 500, n), (3, 64, 700, n - 1)
    return dict(n=n, wide=wide_operand(n, h, empty_cols), thin=thin_operand(n, n + h, empty_rows), empty_cols=empty_cols,
                empty_rows=empty_rows)


# ------------------------------------------------------------------ 64 / 65 non-zeros in a column of the thin right operand
def boundary_case(kind):
    """n = 1500, thin operand on the right.  "at_64": column 300 lists 64 consecutive rows, column 800 lists 64 rows spread
    with holes over the 200 rows 700 .. 899 (first and last of them included) -- no column lists more.  "at_65": the same with
    row 332 added to column 300 (65 entries).  "long": the two columns of 64, column 1100 with 130 and column 1290 with 200
    consecutive rows.  promises: `counts` = {column: entries}, `most` = the largest column count of the operand"""
    n, h = 1500, 20
    rng = np.random.default_rng(64)
    spread = np.sort(np.concatenate([[700, 899], 701 + rng.choice(198, THIN_MAXK - 2, replace=False)]))
    columns = {300: np.arange(268, 268 + THIN_MAXK), 800: spread}
    counts = {300: THIN_MAXK, 800: THIN_MAXK}
    if kind == "at_65":
        columns[300] = np.arange(268, 268 + THIN_MAXK + 1)
        counts[300] = THIN_MAXK + 1
    elif kind == "long":
        columns[1100] = np.arange(1035, 1035 + 130)
        columns[1290] = np.arange(1190, 1190 + 200)
        counts.update({1100: 130, 1290: 200})
    else:
        assert kind == "at_64"
    return dict(n=n, wide=wide_operand(n, h), thin=thin_operand(n, 11, columns=columns), counts=counts, most=max(counts.values()),
                spread_rows=spread, alpha=1.0, thr=1e-8)


# ------------------------------------------------------------------ ties of slab_thin_rule
def counted_operand(n, count, seed):
    """a band of half-width 4 (full diagonal) with off-diagonal entries removed at random until exactly `count` are left"""
    rng = np.random.default_rng(seed)
    j = np.arange(1, n + 1, dtype=np.int64)
    col = np.repeat(j, 9)
    row = col + np.tile(np.arange(-4, 5), n)
    ok = (row >= 1) & (row <= n)
    col, row = col[ok], row[ok]
    off = np.flatnonzero(col != row)
    drop = len(col) - count
    assert 0 <= drop <= len(off)
    keep = np.ones(len(col), dtype=bool)
    keep[rng.choice(off, drop, replace=False)] = False
    col, row = col[keep], row[keep]
    return tidy(col, row, thin_values(col, row, rng, False))


def rule_tie_cases():
    """n = 256, 8 n = 2048.  (name, A, B, side): side = the gather kernel slab_thin_rule(nnz A, nnz B, n) names for A B --
    "left" (nnz A <= 8 n and nnz B >= nnz A), otherwise "right" (nnz B <= 8 n), otherwise "none" """
    n = 256
    wide = wide_operand(n, 20)
    return n, [
        ("a_8n", counted_operand(n, 8 * n, 1), wide, "left"),
        ("a_8n_plus_1", counted_operand(n, 8 * n + 1, 2), wide, "none"),
        ("b_equals_a", counted_operand(n, 1500, 3), counted_operand(n, 1500, 4), "left"),
        ("b_equals_a_minus_1", counted_operand(n, 1500, 3), counted_operand(n, 1499, 5), "right"),
        ("b_8n", wide, counted_operand(n, 8 * n, 6), "right"),
        ("b_8n_plus_1", wide, counted_operand(n, 8 * n + 1, 7), "none"),
    ]


def thin_rule(nnz_a, nnz_b, n):
    """kernels.hpp slab_thin_rule, restated"""
    return "left" if (nnz_a <= 8 * n and nnz_b >= nnz_a) else "right" if nnz_b <= 8 * n else "none"


# ------------------------------------------------------------------ the dense rule (DenseBranch.f90: threshold on the unscaled sum)
DENSE_ALPHAS = (0.5, 2.0)


def dense_rule_case(cplx=False):
    """n = 48: a thin operand of five diagonals, |values| in (0.5, 1.5) with random signs (234 entries: more than 0.1 n^2 =
    230.4, fewer than 8 n = 384) and a band of half-width 10 with uniform(-1, 1) values; threshold 0.6, alpha 0.5 and 2.0.
    promises: min(nnz) > 0.1 n^2, so the reference keeps an entry when |sum| > thr whatever alpha; for either alpha at least 100
    entries of either product (thin x band, band x thin) fare differently under |alpha sum| > thr"""
    n = 48
    rng = np.random.default_rng(48)
    j = np.arange(1, n + 1, dtype=np.int64)

    def band(hw):
        col = np.repeat(j, 2 * hw + 1)
        row = col + np.tile(np.arange(-hw, hw + 1), n)
        ok = (row >= 1) & (row <= n)
        return col[ok], row[ok]

    tc, tr = band(2)
    tv = rng.uniform(0.5, 1.5, len(tc)) * rng.choice([-1.0, 1.0], len(tc))
    bc, br = band(10)
    bv = rng.uniform(-1.0, 1.0, len(bc))
    if cplx:
        tv = tv * np.exp(1j * rng.uniform(-3.0, 3.0, len(tc)))
        bv = (bv + 1j * rng.uniform(-1.0, 1.0, len(bc))) / np.sqrt(2.0)   # (magnitudes as in the real case)
    return dict(n=n, thin=tidy(tc, tr, tv), wide=tidy(bc, br, bv), thr=0.6, alphas=DENSE_ALPHAS)


# ------------------------------------------------------------------ gaps inside a result column
def gap_case():
    """n = 1024: every column j of the wide operand holds two clusters, rows j - 200 .. j - 100 and j + 100 .. j + 200 (those
    inside the matrix), |values| in (0.5, 1.5); the thin operand is near-identity (reach <= 4).  promises: in either product at
    least 100 result columns hold two kept entries 129 or more rows apart with nothing kept between them (a whole 64-row chunk
    without a kept entry between two written ones), inside a block window of more than 192 rows; threshold 1e-9 prunes nothing"""
    n = 1024
    rng = np.random.default_rng(1024)
    j = np.arange(1, n + 1, dtype=np.int64)
    offs = np.concatenate([np.arange(-200, -99), np.arange(100, 201)])
    col = np.repeat(j, len(offs))
    row = col + np.tile(offs, n)
    ok = (row >= 1) & (row <= n)
    col, row = col[ok], row[ok]
    val = rng.uniform(0.5, 1.5, len(col)) * rng.choice([-1.0, 1.0], len(col))
    return dict(n=n, wide=tidy(col, row, val), thin=thin_operand(n, 77), alpha=1.0, thr=1e-9)


def column_gaps(t, n):
    """per column (index 1 .. n) the largest distance between two consecutive entries; 0 for columns of fewer than two"""
    c, r = t[0].astype(np.int64), t[1].astype(np.int64)
    gaps = np.zeros(n + 1, dtype=np.int64)
    same = c[1:] == c[:-1]
    np.maximum.at(gaps, c[1:][same], (r[1:] - r[:-1])[same])
    return gaps


# ------------------------------------------------------------------ result columns whose entries are all pruned
PRUNED_RUNS = ((40, 60), (300, 330), (500, 512))   # columns first .. last (1-based, inclusive) of the wide operand scaled by 1e-12


def pruned_case():
    """n = 512: the columns PRUNED_RUNS of a band of half-width 20 are scaled by 1e-12, threshold 1e-9.  promises: thin x wide
    has no entry in any scaled column; wide x thin (column j of the result draws on the columns j - 4 .. j + 4 of wide) none in
    the columns at least 4 inside a run; every other column of either result holds entries"""
    n = 512
    c, r, v = wide_operand(n, 20)
    scaled = np.zeros(n + 1, dtype=bool)
    inner = np.zeros(n + 1, dtype=bool)
    for a, b in PRUNED_RUNS:
        scaled[a:b + 1] = True
        inner[a + 4:(n if b == n else b - 4) + 1] = True
    v = np.where(scaled[c], v * 1e-12, v)
    return dict(n=n, wide=tidy(c, r, v), thin=thin_operand(n, 512), alpha=1.0, thr=1e-9, dead_left=np.flatnonzero(scaled),
                dead_right=np.flatnonzero(inner))
