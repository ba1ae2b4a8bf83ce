"""No GPU: every promise of the operand generators of tests/thin_cases.py, asserted on the operands themselves and on the
oracle's FMA product of them (oracle_py.set_fma(True): the arithmetic of the slab sessions' gather kernels).  The GPU tests
(tests/test_gpu_thin_real_sessions.py, tests/test_gpu_thin.py) rely on these properties to reach a branch of a kernel; here they
are conditions that hold or fail without one."""
import numpy as np
import pytest

import thin_cases as tc


@pytest.fixture()
def O():
    from oracle import oracle_py as O
    O.set_fma(True)
    yield O
    O.set_fma(False)


def srt(t):
    c, r, v = (np.asarray(x) for x in t)
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def product(O, n, X, Y, alpha, thr):
    return srt(O.ps_multiply(O.Mat.from_triplets(n, n, *X), O.Mat.from_triplets(n, n, *Y), None, alpha, 0.0, thr).triplets())


def is_tidy(t, n):
    c, r, v = t
    key = c.astype(np.int64) * (n + 1) + r
    return bool(np.all(np.diff(key) > 0) and np.all(v != 0) and c.min() >= 1 and c.max() <= n and r.min() >= 1 and r.max() <= n)


@pytest.mark.parametrize("n,h", tc.BASE_SHAPES)
def test_base_case(O, n, h):
    case = tc.base_case(n, h)
    wide, thin = case["wide"], case["thin"]
    assert is_tidy(wide, n) and is_tidy(thin, n)
    assert len(thin[2]) <= 8 * n < len(wide[2])
    assert not np.isin(wide[0], case["empty_cols"]).any() and not np.isin(thin[1], case["empty_rows"]).any()
    assert np.abs(thin[1].astype(np.int64) - thin[0]).max() <= 4
    # the same generator gives the same operands
    again = tc.base_case(n, h)
    assert all(np.array_equal(a, b) for a, b in zip(thin + wide, again["thin"] + again["wide"]))
    for alpha, thr in tc.BASE_SCALARS:
        for X, Y in ((thin, wide), (wide, thin)):
            got = product(O, n, X, Y, alpha, thr)
            assert len(got[2]) > 8 * n and np.all(np.abs(got[2]) > thr)
    # empty columns of the wide operand are empty columns of thin x wide; empty rows of thin are empty rows of it
    got = product(O, n, thin, wide, 1.0, 0.0)
    assert not np.isin(got[0], case["empty_cols"]).any() and not np.isin(got[1], case["empty_rows"]).any()


@pytest.mark.parametrize("kind", ["at_64", "at_65", "long"])
def test_boundary_case(O, kind):
    case = tc.boundary_case(kind)
    n, thin, wide = case["n"], case["thin"], case["wide"]
    assert is_tidy(wide, n) and is_tidy(thin, n)
    assert len(thin[2]) <= 8 * n < len(wide[2])
    per = tc.per_column(thin, n)
    for col, count in case["counts"].items():
        assert per[col] == count, (col, per[col], count)
    assert per.max() == case["most"] == {"at_64": 64, "at_65": 65, "long": 200}[kind]
    assert (per == 64).sum() == (1 if kind == "at_65" else 2)
    if kind == "at_65":
        assert (per == 65).sum() == 1 and (per > 65).sum() == 0
        # one entry more than "at_64", nothing else differs
        base = tc.boundary_case("at_64")["thin"]
        assert len(thin[2]) == len(base[2]) + 1
    # the spread column: 64 entries over a run of 200 rows, holes of its own inside
    rows = thin[1][thin[0] == 800]
    assert len(rows) == 64 and rows.max() - rows.min() + 1 == 200 and np.diff(rows).max() > 1
    got = product(O, n, wide, thin, case["alpha"], case["thr"])
    assert tc.per_column(got, n)[300] > 64


def test_rule_tie_cases(O):
    n, cases = tc.rule_tie_cases()
    assert n == 256
    want = {"a_8n": (8 * n, None), "a_8n_plus_1": (8 * n + 1, None), "b_equals_a": (1500, 1500), "b_equals_a_minus_1": (1500, 1499),
            "b_8n": (None, 8 * n), "b_8n_plus_1": (None, 8 * n + 1)}
    sides = {"a_8n": "left", "a_8n_plus_1": "none", "b_equals_a": "left", "b_equals_a_minus_1": "right", "b_8n": "right",
             "b_8n_plus_1": "none"}
    assert [c[0] for c in cases] == list(want)
    for name, A, B, side in cases:
        assert is_tidy(A, n) and is_tidy(B, n)
        na, nb = want[name]
        assert na is None or len(A[2]) == na, (name, len(A[2]))
        assert nb is None or len(B[2]) == nb, (name, len(B[2]))
        if na is None:
            assert len(A[2]) > 8 * n + 1     # (the wide operand)
        if nb is None:
            assert len(B[2]) > 8 * n + 1
        assert side == sides[name] == tc.thin_rule(len(A[2]), len(B[2]), n), name
        assert tc.per_column(B, n).max() <= tc.THIN_MAXK or side != "right"
        assert len(product(O, n, A, B, 1.0, 1e-8)[2]) > 0


@pytest.mark.parametrize("cplx", [False, True])
def test_dense_rule_case(O, cplx):
    case = tc.dense_rule_case(cplx)
    n, thin, wide, thr = case["n"], case["thin"], case["wide"], case["thr"]
    assert n == 48 and is_tidy(thin, n) and is_tidy(wide, n)
    assert len(thin[2]) == 234 and 0.1 * n * n < len(thin[2]) <= 8 * n < len(wide[2])
    assert min(len(thin[2]), len(wide[2])) > 0.1 * n * n
    assert np.all((np.abs(thin[2]) > 0.5) & (np.abs(thin[2]) < 1.5))
    for X, Y in ((thin, wide), (wide, thin)):
        sums = product(O, n, X, Y, 1.0, 0.0)      # (alpha 1, threshold 0: every non-zero sum, unscaled)
        kept_dense = np.abs(sums[2]) > thr
        patterns = []
        for alpha in case["alphas"]:
            got = product(O, n, X, Y, alpha, thr)
            # the reference's dense branch: threshold on the unscaled sum, then alpha
            assert np.array_equal(got[0], sums[0][kept_dense]) and np.array_equal(got[1], sums[1][kept_dense])
            kept_sparse = np.abs(alpha * sums[2]) > thr
            differ = int((kept_sparse != kept_dense).sum())
            print("cplx", cplx, "alpha", alpha, "dense rule keeps", int(kept_dense.sum()), "sparse rule would keep", int(kept_sparse.sum()))
            assert differ >= 100, (alpha, differ)
            patterns.append(got)
        assert np.array_equal(patterns[0][0], patterns[1][0]) and np.array_equal(patterns[0][1], patterns[1][1])


def test_gap_case(O):
    case = tc.gap_case()
    n, thin, wide = case["n"], case["thin"], case["wide"]
    assert n == 1024 and is_tidy(thin, n) and is_tidy(wide, n)
    assert len(thin[2]) <= 8 * n < len(wide[2])
    for X, Y in ((thin, wide), (wide, thin)):
        got = product(O, n, X, Y, case["alpha"], case["thr"])
        unpruned = product(O, n, X, Y, case["alpha"], 0.0)
        assert len(got[2]) == len(unpruned[2])                      # (the threshold prunes nothing)
        gaps = tc.column_gaps(got, n)
        assert (gaps >= 2 * tc.CHUNK + 1).sum() >= 100, int((gaps >= 129).sum())
        span = np.array([got[1][got[0] == j].max() - got[1][got[0] == j].min() + 1 for j in (300, 512, 700)])
        assert span.min() > 3 * tc.CHUNK                           # (a window of more than 192 rows)


def test_pruned_case(O):
    case = tc.pruned_case()
    n, thin, wide = case["n"], case["thin"], case["wide"]
    assert n == 512 and is_tidy(thin, n) and is_tidy(wide, n)
    assert len(thin[2]) <= 8 * n < len(wide[2])
    for X, Y, dead in ((thin, wide, case["dead_left"]), (wide, thin, case["dead_right"])):
        got = product(O, n, X, Y, case["alpha"], case["thr"])
        sums = product(O, n, X, Y, case["alpha"], 0.0)
        per, per0 = tc.per_column(got, n), tc.per_column(sums, n)
        assert len(dead) >= 8 and np.all(per[dead] == 0) and np.all(per0[dead] > 0)     # computed, then pruned whole
        if X is thin:
            assert np.array_equal(np.flatnonzero(per[1:] == 0) + 1, dead)
        # four dead columns in a row that start at a multiple of 4 (0-based): a whole column group of k_thin_slab_left
        d0 = dead - 1
        assert any(j % 4 == 0 and np.isin([j + 1, j + 2, j + 3], d0).all() for j in d0)
        # the product that follows reads the result with its empty columns
        assert len(product(O, n, got, wide, 1.0, case["thr"])[2]) > 0
