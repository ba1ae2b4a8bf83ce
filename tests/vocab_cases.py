"""Case table and operand generator of the multi-rank vocabulary test (tests/test_gpu_multirank_vocabulary.py and its
worker tests/multirank_vocab_worker.py).  numpy only, no engine import: the worker and the test both import this
module, so both see the same bytes.

Every operand is generated WHOLE from the case's seed and returned as column-major sorted 1-based triplets
(col, row, val); values are uniform in (-1, 1), complex operands draw a second array for the imaginary parts, exact
zeros are removed.  The families are the degenerate panels of a column-panel distribution over 2-4 ranks:

  tiny      n = 1, 2, 3, dense: with more ranks than columns some ranks own a panel of width 0
  narrow    n = 5, 7, density 0.5: panels 1-3 columns wide and unequal
  scatter   n = 67, density 0.10, no band (the halo degenerates to the full gather); column n//3 and row n//2 empty
  factor    n = 130, L with entries in its first 9 columns only (density 0.6 there), products L L^T and L^T L with
            L^T from Transpose: the ranks >= 1 hold panels of L without an entry
  holes     n = 130, band h = 3; columns and rows [b-4, b+4) emptied around every panel boundary b of 2, 3 and 4
            ranks at once: gaps in front of the first needed column; B2 the whole band, whose panels ask their
            neighbours for emptied columns only: owner segments with columns but no entries
  interior  n = 130, A a band (h = 3); B a block diagonal whose blocks lie inside the panels of 2, 3 and 4 ranks
            (every column names local columns of A only: nothing is received); B2 two entries per column, at rows 1
            and n (no column is interior)
"""
import numpy as np

WORLDS = (2, 3, 4)
# C.Gemm(A, B, None, alpha, beta, threshold)
PRODUCT_PARAMS = ((1.0, 0.0, 0.0), (-0.5, 0.0, 1e-3), (2.0, 0.7, 0.0))
# B.Increment(A, alpha, threshold), under increment_force_seq 0, 1, 2
INCREMENT_PARAMS = ((1.0, 0.0), (0.37, 0.3))
INCREMENT_SEQ = (0, 1, 2)
HALO_OVERLAP = (0, 2, 3)
FAMILIES = (("tiny", (1, 2, 3)), ("narrow", (5, 7)), ("scatter", (67,)), ("factor", (130,)), ("holes", (130,)),
            ("interior", (130,)))
BAND = 3


def panel_bounds(n, world):
    """first column (0-based) of every rank's panel, and n"""
    return [n * r // world for r in range(world + 1)]


def boundaries(n):
    """the panel boundaries inside (0, n) of every world of the test"""
    return sorted({n * r // w for w in WORLDS for r in range(1, w)})


def triplets(D):
    """dense array -> (col, row, val), 1-based, sorted by column then row, exact zeros removed"""
    c, r = np.nonzero(D.T)
    return (c + 1).astype(np.int32), (r + 1).astype(np.int32), np.ascontiguousarray(D.T[c, r])


def dense(n, t, cplx=None):
    col, row, val = t
    D = np.zeros((n, n), dtype=complex if (np.iscomplexobj(val) if cplx is None else cplx) else float)
    D[row - 1, col - 1] = val
    return D


def _random(rng, n, density, cplx, mask=None):
    v = rng.uniform(-1.0, 1.0, (n, n))
    if cplx:
        v = v + 1j * rng.uniform(-1.0, 1.0, (n, n))
    keep = rng.random((n, n)) < density
    if mask is not None:
        keep &= mask
    return np.where(keep, v, 0.0)


def _band(n, h):
    i = np.arange(n)
    return np.abs(i[:, None] - i[None, :]) <= h


def empty_holes(D):
    """columns and rows [b-4, b+4) around every panel boundary emptied"""
    n = D.shape[0]
    for b in boundaries(n):
        D[:, b - 4:b + 4] = 0.0
        D[b - 4:b + 4, :] = 0.0
    return D


def _operand(family, rng, n, cplx, which):
    """one operand of the family: which = 'A' (left), 'B' (right), 'B2' (a second right operand: holes, interior)"""
    if family == "tiny":
        return _random(rng, n, 1.0, cplx)
    if family == "narrow":
        return _random(rng, n, 0.5, cplx)
    if family == "scatter":
        D = _random(rng, n, 0.10, cplx)
        D[:, n // 3] = 0.0
        D[n // 2, :] = 0.0
        return D
    if family == "factor":     # ('B' is L^T: the worker makes it by Transpose, the test by numpy)
        mask = np.zeros((n, n), dtype=bool)
        mask[:, :9] = True
        return _random(rng, n, 0.6, cplx, mask)
    if family == "holes":
        D = _random(rng, n, 1.0, cplx, _band(n, BAND))
        return D if which == "B2" else empty_holes(D)
    if family == "interior":
        if which == "A":
            return _random(rng, n, 1.0, cplx, _band(n, BAND))
        if which == "B":       # blocks of at most 6 columns, none across a panel boundary of any world
            mask = np.zeros((n, n), dtype=bool)
            edges = [0] + boundaries(n) + [n]
            for a, b in zip(edges[:-1], edges[1:]):
                for s in range(a, b, 6):
                    e = min(b, s + 6)
                    mask[s:e, s:e] = True
            return _random(rng, n, 0.8, cplx, mask)
        mask = np.zeros((n, n), dtype=bool)
        mask[0, :] = True
        mask[n - 1, :] = True
        return _random(rng, n, 1.0, cplx, mask)
    raise ValueError(family)


def make_case(family, fi, n, cplx):
    rng = np.random.default_rng(7000 + 1000 * fi + 2 * n + int(cplx))
    ops = {"A": _operand(family, rng, n, cplx, "A")}
    if family == "factor":
        ops["B"] = ops["A"].T.copy()
    else:
        ops["B"] = _operand(family, rng, n, cplx, "B")
    if family in ("holes", "interior"):
        ops["B2"] = _operand(family, rng, n, cplx, "B2")
    ops["C0"] = _random(rng, n, 0.05, cplx)          # what a product with beta != 0 finds in C
    if n <= 7:     # (5 % of at most 49 elements is mostly nothing: one more product on a C that holds entries)
        ops["C1"] = _random(rng, n, 0.6, cplx)
    if cplx:
        ops["Ar"] = _operand(family, rng, n, False, "A")     # a real left operand beside a complex right one
        ops["C0r"] = _random(rng, n, 0.05, False)            # a real C under complex operands
        if n <= 7:
            ops["C1r"] = _random(rng, n, 0.6, False)
    lookup = (rng.permutation(n) + 1).astype(np.int32)
    # MatrixDiagonalScale: one triplet per odd column, then a second one on column 1
    dcol = np.concatenate((np.arange(1, n + 1, 2), [1])).astype(np.int32)
    dval = rng.uniform(-2.0, 2.0, len(dcol))
    if cplx:
        dval = dval + 1j * rng.uniform(-2.0, 2.0, len(dcol))
    right = ["B", "B2"] if "B2" in ops else ["B"]
    pairs = [("A", b) for b in right] + [("A", "A")]
    if family == "factor":
        pairs.insert(1, ("B", "A"))    # L^T L
    return {"id": "%s%d%s" % (family, n, "c" if cplx else "r"), "family": family, "n": n, "cplx": cplx,
            "ops": {k: triplets(v) for k, v in ops.items()}, "transposed": {"B": "A"} if family == "factor" else {},
            "lookup": lookup, "diag": (dcol, dcol.copy(), dval), "pairs": pairs, "overlap_pairs": [("A", b) for b in right]}


def cases():
    out = []
    for fi, (family, sizes) in enumerate(FAMILIES):
        for n in sizes:
            for cplx in (False, True):
                out.append(make_case(family, fi, n, cplx))
    return out


def product_runs(case):
    """(tag, left, right, alpha, beta, threshold, operand C is pre-filled with or None) of every product of the case"""
    runs = []
    for left, right in case["pairs"]:
        for k, (alpha, beta, thr) in enumerate(PRODUCT_PARAMS):
            runs.append(("p%d_%s_%s" % (k, left, right), left, right, alpha, beta, thr, "C0" if beta != 0.0 else None))
    if "C1" in case["ops"]:
        alpha, beta, thr = PRODUCT_PARAMS[2]
        runs.append(("p2_A_B_on_C1", "A", "B", alpha, beta, thr, "C1"))
    if case["cplx"]:
        runs.append(("mix_Ar_B", "Ar", "B", 1.0, 0.0, 0.0, None))
        runs.append(("mix_C0r", "A", "B", 2.0, 0.7, 0.0, "C0r"))
        if "C1r" in case["ops"]:
            runs.append(("mix_C1r", "A", "B", 2.0, 0.7, 0.0, "C1r"))
    return runs


def split_for_rank(t, rank, world):
    """the triplets a rank passes to a fill that is NOT prepartitioned: position i of the whole list goes to rank i % world"""
    sel = np.arange(len(t[0])) % world == rank
    return t[0][sel], t[1][sel], t[2][sel]
