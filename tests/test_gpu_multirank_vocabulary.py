"""GPU: the distributed vocabulary on DEGENERATE panels across 2, 3 and 4 ranks -- panels of width 0, of 1-3 unequal
columns, panels without an entry, owner segments with columns but no entries, panels that receive nothing, columns of
which none is interior -- through every multi-rank entry point of the matrix vocabulary: Gemm (alpha, beta with a
pre-filled C, thresholds, A = B, real beside complex, a real C under complex operands), the overlapped halo exchange
under every setting, Transpose, Conjugate, Increment (three merge settings), PairwiseMultiply, Scale, Dot, Trace, Norm,
GetMatrixSize, GershgorinBounds, MeasureAsymmetry, Symmetrize, IsIdentity, FillIdentity, PermuteMatrix and its undo,
FillPermutation, the fill that is not prepartitioned, GetMatrixSlice, ResizeMatrix, GetMatrixBlock,
MatrixDiagonalScale and GatherMatrixToProcess.  The cases and their operands are tests/vocab_cases.py; one worker
process per rank (tests/multirank_vocab_worker.py) runs all of them, the ranks share the one GPU and exchange through
the shared-memory test transport, as in tests/test_gpu_multirank.py.  This process computes every reference on the CPU
(numpy and the C oracle) and never opens the GPU.

Contracts (those of tests/test_gpu_parity.py, tests/test_gpu_extras.py and tests/test_gpu_multirank.py):
  unfused products   the concatenated rank panels equal the oracle's product bit for bit on the sparse branch; to
                     1e-13 max(1, |want|max) + 2 thr where the reference takes its dense branch
                     (min(nnzA, nnzB) / n^2 > 0.1), and to 1e-13 max(1, |want|max) where beta != 0
  FMA products       bit for bit the one-rank run of the same arithmetic, which matches the oracle to
                     1e-13 max(1, |want|max) + 2 thr
  halo overlap       the products under halo_overlap 0, 2 and 3 are bit-identical to each other and to the default
  Increment, PairwiseMultiply   the oracle's, bit for bit; Dot, Trace, Norm, Gershgorin to 1e-13; GetMatrixSize exact
  data movement      Transpose, Conjugate, Scale, permute / undo, the permutation product, slice, resize, block, diagonal
                     scale, both gathers and the fill from anywhere equal numpy's result exactly
  Symmetrize at atol 1e-16, MeasureAsymmetry at rel 1e-13
  panels tile [0, n) in rank order with boundaries floor(n r / world); a rank with a panel of width 0 returns empty
  triplet arrays; every rank returns the same value for every scalar and predicate.

GetMatrixSlice asks for rows [2, n-1] x columns [1, ceil(n/2)]: the 1 x 1 and 2 x 2 cases have no such slice, so the
slice runs for n >= 3 (a condition of the case table, the same in every world)."""
import os
import subprocess
import sys
import time
import uuid

import numpy as np
import pytest

import vocab_cases as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Measured on an MI355X: one run (all ranks, every case of the table) takes 0.5 s on one rank, 1.2 s on two, 1.9 s on
# three and 2.5 s on four (a two-rank run of tests/test_gpu_multirank.py's worker: 1.1 s); the limit is five times the
# longest, rounded up
RUN_TIMEOUT = 15
SFX = ("_col", "_row", "_val")


def run_world(world, tmp_path, arith="unfused"):
    out = str(tmp_path / ("w%d%s" % (world, arith)))
    name = "t%s" % uuid.uuid4().hex[:12]
    assert world <= 4
    procs = []
    t0 = time.time()
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name,
                   NTPOLY_AMD_SHM_MB="8", NTPOLY_AMD_SPGEMM_FMA="1" if arith == "fma" else "0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "multirank_vocab_worker.py"), out], env=env,
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
    print("vocabulary run: world %d, %s: %.1f s" % (world, arith, time.time() - t0))
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d of %d failed:\n%s" % (r, world, logs[r][-3000:])
    return [dict(np.load(out + ".%d.npz" % r)) for r in range(world)]


# ------------------------------------------------------------------ references (CPU)
def sorted_triplets(t):
    order = np.lexsort((t[1], t[0]))
    return t[0][order], t[1][order], t[2][order]


def diagonal_scaled(case):
    """MatrixDiagonalScale: column c of A times the triplet's value, one triplet after the other, in the engine's
    arithmetic (separate multiplications and additions)"""
    n, cplx = case["n"], case["cplx"]
    fr, fi = np.ones(n), np.zeros(n)
    for c, v in zip(case["diag"][0], case["diag"][2]):
        re, im = float(np.real(v)), float(np.imag(v))
        a, b = fr[c - 1], fi[c - 1]
        if cplx:
            fr[c - 1], fi[c - 1] = a * re - b * im, a * im + b * re
        else:
            fr[c - 1] = a * re
    col, row, val = case["ops"]["A"]
    if not cplx:
        return col, row, fr[col - 1] * val
    x, y = fr[col - 1], fi[col - 1]
    return col, row, (x * val.real - y * val.imag) + 1j * (x * val.imag + y * val.real)


def compute_expected(arith):
    """every reference of every case, from the case table alone: {case id: {tag: triplets | scalar}}"""
    from oracle import oracle_py as O
    O.set_fma(arith == "fma")
    try:
        out = {}
        for case in V.cases():
            n, cplx = case["n"], case["cplx"]
            ops = case["ops"]
            kind = complex if cplx else float
            e = {}

            def omat(t, as_complex=False):
                return O.Mat.from_triplets(n, n, t[0], t[1], t[2].astype(complex) if as_complex else t[2])

            a = V.dense(n, ops["A"], cplx)
            Ao, Bo = omat(ops["A"]), omat(ops["B"])
            e["A"] = ops["A"]
            for tag, left, right, alpha, beta, thr, prefill in V.product_runs(case):
                Lo, Ro = omat(ops[left], cplx), omat(ops[right], cplx)
                Co = omat(ops[prefill], cplx) if prefill else None
                e[tag] = O.ps_multiply(Lo, Ro, Co, alpha, beta, thr).triplets()
                e[tag + ".dense_branch"] = min(len(ops[left][0]), len(ops[right][0])) / float(n * n) > 0.1
            e["transpose"] = V.triplets(a.T)
            if cplx:
                e["conjugate"] = V.triplets(a.conj())
            for k, (alpha, thr) in enumerate(V.INCREMENT_PARAMS):
                e["inc%d" % k] = O.increment(Ao, Bo, alpha, thr).triplets()
            e["pairwise"] = O.pairwise(Ao, Bo).triplets()
            e["scale"] = (ops["A"][0], ops["A"][1], -2.0 * ops["A"][2])
            e["dot"], e["trace"], e["norm"], e["size"] = O.dot(Ao, Bo), O.trace(Bo), O.norm(Bo), len(ops["A"][0])
            if not cplx:
                e["gershgorin"] = O.gershgorin(Bo)
            e["asymmetry"] = np.abs(a - a.conj().T).sum(axis=0).max()
            e["symmetrize"] = 0.5 * (a + a.conj().T)
            e["is_identity"] = int(np.array_equal(a, np.eye(n)))
            e["identity"] = V.triplets(np.eye(n))
            lookup = case["lookup"]
            e["permute"] = V.triplets(a[np.ix_(lookup - 1, lookup - 1)])     # out(i, j) = in(perm(i), perm(j))
            e["unpermute"] = ops["A"]
            pr = np.zeros((n, n))
            pr[np.arange(n), lookup - 1] = 1.0
            e["fill_permutation"] = V.triplets(pr)
            e["permutation_product"] = V.triplets(a[lookup - 1, :])
            e["fill_anywhere"] = ops["A"]
            if n >= 3:
                half = (n + 1) // 2
                dim = max(n - 2, half)
                s = np.zeros((dim, dim), dtype=kind)
                s[:n - 2, :half] = a[1:n - 1, :half]
                e["slice"], e["slice_dim"] = V.triplets(s), dim
            half = (n + 1) // 2
            e["resize_down"], e["resize_down_dim"] = V.triplets(a[:half, :half]), half
            up = np.zeros((n + 3, n + 3), dtype=kind)
            up[:n, :n] = a
            e["resize_up"], e["resize_up_dim"] = V.triplets(up), n + 3
            e["diagonal_scale"] = diagonal_scaled(case)
            e["gather"] = ops["A"]
            out[case["id"]] = e
        return out
    finally:
        O.set_fma(False)


def block_owner(col, world):
    """GetMatrixBlock with rank r asking for rows [1, n+1) x columns [1 + r, n+1): the boxes of the ranks
    0 .. min(col, world) - 1 hold an entry of column col, and the FIRST of them receives it"""
    return np.zeros_like(col)


# ------------------------------------------------------------------ comparison
def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def within(n, got, want, tol, what):
    gd, wd = V.dense(n, got, True), V.dense(n, want, True)
    err = np.abs(gd - wd).max() if n else 0.0
    assert err <= tol(max(1.0, np.abs(wd).max())), "%s: max |d| = %g" % (what, err)


def check_run(parts, world, arith, expected, single=None):
    """every contract of the module's docstring on the results of one run (parts[r]: what rank r saved); single: the
    one-rank run of the same arithmetic (world > 1)"""
    for case in V.cases():
        cid, n, cplx = case["id"], case["n"], case["cplx"]
        e = expected[cid]
        bounds = V.panel_bounds(n, world)

        def cat(tag, of=parts):
            return tuple(np.concatenate([p["%s.%s%s" % (cid, tag, s)] for p in of]) for s in SFX)

        def tiles(tag, dim):
            want = V.panel_bounds(dim, world)
            for r in range(world):
                got = [int(x) for x in parts[r]["%s.%s_panel" % (cid, tag)]]
                assert got == [dim, want[r], want[r + 1]], (cid, tag, r, got, want)
                col = parts[r]["%s.%s_col" % (cid, tag)]
                if want[r + 1] == want[r]:     # a panel of width 0: empty triplet arrays, not an error
                    assert all(len(parts[r]["%s.%s%s" % (cid, tag, s)]) == 0 for s in SFX), (cid, tag, r)
                assert np.all((col > want[r]) & (col <= want[r + 1])), (cid, tag, r)

        def exact(tag, want, name=None):
            got = cat(tag)
            assert len(got[0]) == len(want[0]) and same(got[:2], want[:2]), "%s %s: pattern differs (%d vs %d entries)" % (
                cid, name or tag, len(got[0]), len(want[0]))
            assert got[2].dtype == want[2].dtype and np.array_equal(got[2], want[2]), "%s %s: values differ, max |d| = %g" % (
                cid, name or tag, np.abs(got[2] - want[2]).max())

        def scalars(tag):
            """one value on every rank"""
            v = [parts[r]["%s.%s" % (cid, tag)] for r in range(world)]
            assert all(np.array_equal(x, v[0]) for x in v), (cid, tag, v)
            return v[0]

        # ---- panels
        tiles("A", n)
        exact("A", e["A"])
        # ---- products
        for tag, left, right, alpha, beta, thr, prefill in V.product_runs(case):
            want, dense_branch = e[tag], e[tag + ".dense_branch"]
            what = "%s %s (world %d, %s)" % (cid, tag, world, arith)
            loose = lambda scale: 1e-13 * scale + 2 * thr * (1 if dense_branch else 0)   # noqa: E731
            if arith == "fma":
                if single is not None:
                    exact(tag, cat(tag, [single]), what + " against one rank")
                else:
                    within(n, cat(tag), want, lambda scale: 1e-13 * scale + 2 * thr, what)
            elif dense_branch or beta != 0.0:
                within(n, cat(tag), want, loose, what)
            else:
                exact(tag, want, what)
        # ---- halo overlap: the same product under every setting
        for left, right in case["overlap_pairs"]:
            base = cat("p0_%s_%s" % (left, right))
            for ov in V.HALO_OVERLAP:
                got = cat("ov%d_%s_%s" % (ov, left, right))
                assert same(got, base), (cid, "halo_overlap", ov, left, right)
        # ---- element-wise calls against the oracle and numpy
        exact("transpose", e["transpose"])
        if cplx:
            exact("conjugate", e["conjugate"])
        for k in range(len(V.INCREMENT_PARAMS)):
            for seq in V.INCREMENT_SEQ:
                exact("inc%d_seq%d" % (k, seq), e["inc%d" % k])
        exact("pairwise", e["pairwise"])
        exact("scale", e["scale"])
        # ---- scalars and predicates: the same on every rank
        d = scalars("dot")
        assert abs(complex(d[0], d[1]) - e["dot"]) <= 1e-13 * max(1.0, abs(e["dot"])), (cid, "dot", d, e["dot"])
        assert float(scalars("trace")[0]) == pytest.approx(e["trace"], rel=1e-13, abs=1e-13), (cid, "trace")
        assert float(scalars("norm")[0]) == pytest.approx(e["norm"], rel=1e-13, abs=1e-13), (cid, "norm")
        assert int(scalars("size")[0]) == e["size"], (cid, "size")
        if not cplx:
            lo, hi = scalars("gershgorin")
            assert lo == pytest.approx(e["gershgorin"][0], rel=1e-13, abs=1e-13), (cid, "gershgorin", lo, e["gershgorin"])
            assert hi == pytest.approx(e["gershgorin"][1], rel=1e-13, abs=1e-13), (cid, "gershgorin", hi, e["gershgorin"])
        assert float(scalars("asymmetry")[0]) == pytest.approx(e["asymmetry"], rel=1e-13), (cid, "asymmetry")
        assert np.allclose(V.dense(n, cat("symmetrize"), cplx), e["symmetrize"], atol=1e-16), (cid, "symmetrize")
        assert int(scalars("is_identity")[0]) == e["is_identity"], (cid, "is_identity")
        exact("identity", e["identity"])
        ident = scalars("identity_scalars")
        assert ident[0] == 1 and ident[1] == n and ident[2] == 1.0, (cid, "identity", ident)
        # ---- relabelling, fill from anywhere
        for tag in ("permute", "unpermute", "fill_permutation", "permutation_product", "fill_anywhere"):
            exact(tag, e[tag])
        # ---- slice, resize, block, diagonal scale
        if n >= 3:
            tiles("slice", e["slice_dim"])
            exact("slice", e["slice"])
        for tag in ("resize_down", "resize_up"):
            tiles(tag, e[tag + "_dim"])
            exact(tag, e[tag])
        owner = block_owner(e["A"][0], world)
        for r in range(world):
            got = sorted_triplets(tuple(parts[r]["%s.block%s" % (cid, s)] for s in SFX))
            want = tuple(x[owner == r] for x in e["A"])
            assert same(got, want), (cid, "block", r, len(got[0]), len(want[0]))
        exact("diagonal_scale", e["diagonal_scale"])
        # ---- gathers: the whole matrix on every rank; on one rank only
        target = min(1, world - 1)
        for r in range(world):
            got = tuple(parts[r]["%s.gather_all%s" % (cid, s)] for s in SFX)
            assert same(got, e["gather"]), (cid, "gather_all", r)
            here = int(parts[r]["%s.gather_one_here" % cid][0])
            assert here == int(r == target), (cid, "gather_one", r, here)
            if here:
                assert same(tuple(parts[r]["%s.gather_one%s" % (cid, s)] for s in SFX), e["gather"]), (cid, "gather_one", r)


# ------------------------------------------------------------------ fixtures and tests
@pytest.fixture(scope="module")
def expected():
    """the CPU references in either arithmetic mode (made on first use, shared and left unchanged)"""
    cache = {}

    def get(arith):
        if arith not in cache:
            cache[arith] = compute_expected(arith)
        return cache[arith]
    return get


@pytest.fixture(scope="module")
def references(tmp_path_factory):
    """the one-rank run in either arithmetic mode (made on first use)"""
    cache = {}

    def get(arith):
        if arith not in cache:
            cache[arith] = run_world(1, tmp_path_factory.mktemp("vocab_ref_" + arith), arith)[0]
        return cache[arith]
    return get


@pytest.mark.parametrize("arith", ["unfused", "fma"])
def test_vocabulary_on_one_rank(arith, references, expected):
    """the worker's one-rank run against the CPU references (the FMA products to 1e-13 max(1, |want|max) + 2 thr)"""
    check_run([references(arith)], 1, arith, expected(arith))


@pytest.mark.parametrize("world,arith", [(w, a) for a in ("unfused", "fma") for w in V.WORLDS])
def test_vocabulary_on_degenerate_panels(world, arith, references, expected, tmp_path):
    single = references(arith)
    parts = run_world(world, tmp_path, arith)
    check_run(parts, world, arith, expected(arith), single)
