"""GPU: PowerBounds on one vector (option power_vector; csrc/power_vector.hip k_pv_step / k_pv_tail / k_pv_finish / k_pv_scale,
solvers_func.cpp power_bounds).

The premise: the reference's iterate is a matrix of N identical columns, a column of a product depends on the same column of the
right operand only, and the engine's products give the same bits for the same column arithmetic.  So (1) for V = N columns x,
every column of MatrixMultiply(A, V) is the same, and the y of power_vector_step equals column 0 in pattern and bits -- real
operands in both arithmetic modes, complex ones in unfused mode; complex in FMA mode runs the complex tile kernel's tolerance mode
and is compared with close() of tests/test_gpu_complex_tile.py (1e-13 of the largest entry).  (2) Ten steps driven through the
entry point give the Ritz values of a dense numpy power iteration with the same pruning to 1e-12.  (3) PowerBounds with the
option at 1 equals the option at 0 to rel 1e-6, the project's own PowerBounds tolerance (the Aitken value amplifies the last bits
of the Ritz values), and so do ComputeExponential and EstimateGap to the tolerances of test_matrix_functions_golden and of the
`gap` case; the counters show which path ran.  (4) The `power` cases of tests/golden/functions.npz -- the reference's own bounds
-- through the new path.  (5) The memory a solve takes, in a fresh process.  (6) Two and three ranks over the shared-memory
transport.

Thresholded case of (1): the threshold is the midpoint between two neighbouring moduli of the dense product's column, chosen so
that it prunes three tenths of its non-zero entries; the test asserts that between a tenth and a half are pruned.  A column with
fewer than four non-zero entries (n = 1) has no such threshold and runs at threshold 0 only."""
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from gen import banded_triplets
from golden_util import Golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION = "power_vector"
REL = 1e-13


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture(params=[1, 0], ids=["fma", "unfused"])
def arith(nt, request):
    before = {k: nt.get_option(k) for k in ("spgemm_fma", OPTION)}
    nt.set_option("spgemm_fma", request.param)
    yield request.param
    for k, v in before.items():
        nt.set_option(k, v)


# ------------------------------------------------------------------ operands
def band(n, hl, hu, shift=2.5):
    """the non-symmetric band of tests/test_gpu_slab_transpose.py: -hu <= row - col <= hl kept, entries above the diagonal halved"""
    col, row, val = banded_triplets(n, max(hl, hu), shift=shift)
    d = row.astype(np.int64) - col
    keep = (d >= -hu) & (d <= hl)
    val = np.where(d < 0, 0.5 * val, val)
    return col[keep], row[keep], val[keep]


def full_row_and_column(n=130):
    """a narrow band with one full row (70) and one full column (5): a chain longer than any slice neighbour's"""
    col, row, val = band(n, 3, 2)
    A = np.zeros((n, n))
    A[row - 1, col - 1] = val
    k = np.arange(n)
    A[70, :] = 0.01 * (1.0 + (k * 37) % 11)
    A[:, 5] = -0.02 * (1.0 + (k * 13) % 7)
    A[70, 70] = 2.0
    A[5, 5] = 3.0
    r, c = np.nonzero(A.T)   # (column-major order)
    return (r + 1).astype(np.int32), (c + 1).astype(np.int32), A[c, r]


def with_empties(n=150):
    """empty rows (3, 64, 100) and empty columns (10, 64, 149)"""
    col, row, val = band(n, 24, 9)
    keep = ~np.isin(row - 1, (3, 64, 100)) & ~np.isin(col - 1, (10, 64, 149))
    return col[keep], row[keep], val[keep]


OPERANDS = {
    "band257": lambda: (257,) + band(257, 24, 9),
    "n63": lambda: (63,) + band(63, 24, 9),
    "n65": lambda: (65,) + band(65, 24, 9),
    "rowcol130": lambda: (130,) + full_row_and_column(130),
    "empties150": lambda: (150,) + with_empties(150),
    "n1": lambda: (1, np.array([1], dtype=np.int32), np.array([1], dtype=np.int32), np.array([2.5])),
}


def make(name, cplx):
    n, col, row, val = OPERANDS[name]()
    if cplx:
        rng = np.random.default_rng(7)
        val = val + 1j * 0.3 * rng.standard_normal(len(val))
    return n, col, row, val


def dense(n, col, row, val):
    A = np.zeros((n, n), dtype=val.dtype)
    A[row - 1, col - 1] = val
    return A


def vectors(n, cplx):
    e1 = np.zeros(n, dtype=np.complex128 if cplx else np.float64)
    e1[0] = 1.0 / n
    rng = np.random.default_rng(11)
    x = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)
    x[rng.random(n) < 1.0 / 3.0] = 0.0
    if n == 1:
        x[0] = 0.75
    return {"e1": e1, "random": x}


def bits(v):
    return np.ascontiguousarray(v).view(np.uint64)


def prune(y, thr):
    return np.where(np.abs(y) > thr, y, 0.0)


def pick_threshold(yd):
    """prunes three tenths of the column's non-zero entries: the midpoint between two neighbouring moduli (None: too few entries)"""
    m = np.sort(np.abs(yd[yd != 0]))
    if len(m) < 4:
        return None
    j = max(1, int(round(0.3 * len(m))))
    if m[j - 1] == m[j]:
        return None
    return 0.5 * (m[j - 1] + m[j])


# ------------------------------------------------------------------ 1. the premise and the step
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("name", list(OPERANDS))
def test_step_is_column_zero_of_the_product(nt, arith, name, cplx):
    n, col, row, val = make(name, cplx)
    A = nt.Matrix_ps.from_triplets(n, col, row, val)
    Ad = dense(n, col, row, val)
    exact = (not cplx) or arith == 0
    for xname, x in vectors(n, cplx).items():
        yd = Ad @ x
        thresholds = [0.0]
        t = pick_threshold(yd)
        if t is not None:
            thresholds.append(t)
        else:
            assert n == 1, "every operand but n = 1 has a pruning threshold"
        # V: n identical columns x (the zeros of x are not stored)
        nzr = np.nonzero(x)[0]
        vcol = np.repeat(np.arange(1, n + 1, dtype=np.int32), len(nzr))
        vrow = np.tile((nzr + 1).astype(np.int32), n)
        V = nt.Matrix_ps.from_triplets(n, vcol, vrow, np.tile(x[nzr], n))
        for thr in thresholds:
            tag = (name, xname, thr)
            if thr > 0:
                share = np.count_nonzero((np.abs(yd) <= thr) & (yd != 0)) / np.count_nonzero(yd)
                assert 0.1 <= share <= 0.5, tag + (share,)
            Cm = nt.Matrix_ps(n)
            Cm.Gemm(A, V, threshold=thr)
            ccol, crow, cval = Cm.triplets()
            assert np.all(cval != 0), tag
            Cd = np.zeros((n, n), dtype=Ad.dtype)
            stored = np.zeros((n, n), dtype=bool)
            Cd[crow - 1, ccol - 1] = cval
            stored[crow - 1, ccol - 1] = True
            # the premise: all columns of the product are the same, pattern and bits
            assert np.array_equal(stored, np.repeat(stored[:, :1], n, axis=1)), tag
            columns = bits(Cd.T)   # (row j: the bits of column j)
            assert np.array_equal(columns, np.repeat(columns[:1], n, axis=0)), tag
            got = nt.power_vector_step(A, x, thr)
            assert got is not None, tag
            y, d1, d2, n1 = got
            if exact:
                assert np.array_equal(y != 0, stored[:, 0]), tag
                assert np.array_equal(bits(y[stored[:, 0]]), bits(Cd[stored[:, 0], 0])), tag
            else:
                # (the rule of close() in tests/test_gpu_complex_tile.py on one column)
                scale = max(1.0, np.abs(Cd[:, 0]).max()) if n else 1.0
                diff = np.abs(y - Cd[:, 0])
                bad = diff > REL * scale
                assert np.all(diff[bad] <= thr * (1 + 1e-9) + REL * scale), tag + (diff.max(),)
                assert abs(np.count_nonzero(y) - np.count_nonzero(stored[:, 0])) <= 8, tag
            # the pruning agrees with the dense product's column
            assert np.array_equal(y != 0, prune(yd, thr) != 0), tag
            # the three sums, over the kept values
            want = (float(np.sum(np.abs(x) ** 2)), float(np.sum((np.conj(x) * y).real)), float(np.sum(np.abs(y))))
            for g, w, what in zip((d1, d2, n1), want, ("d1", "d2", "n1")):
                print(name, xname, thr, what, g, w)
                assert abs(g - w) <= 1e-14 * abs(w), tag + (what, g, w)
            again = nt.power_vector_step(A, x, thr)
            assert np.array_equal(bits(again[0]), bits(y)) and again[1:] == (d1, d2, n1), tag


# ------------------------------------------------------------------ 2. the loop restated
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("thr", [0.0, 1e-5])
def test_ten_steps_through_the_entry_point_are_a_dense_power_iteration(nt, arith, cplx, thr):
    n, col, row, val = make("band257", cplx)
    A = nt.Matrix_ps.from_triplets(n, col, row, val)
    Ad = dense(n, col, row, val)
    x = vectors(n, cplx)["e1"]
    xd = x.copy()
    for step in range(10):
        y, d1, d2, n1 = nt.power_vector_step(A, x, thr)
        yd = prune(Ad @ xd, thr)
        ritz = float(np.sum((np.conj(xd) * yd).real)) / float(np.sum(np.abs(xd) ** 2))
        print(step, d2 / d1, ritz)
        assert d2 / d1 == pytest.approx(ritz, rel=1e-12), step
        x = y * (1.0 / n1)
        xd = yd * (1.0 / float(np.sum(np.abs(yd))))


# ------------------------------------------------------------------ 3. the solver
def solver_operand(nt, name):
    if name == "sym1037":
        n = 1037
        t = banded_triplets(n, 24)
    elif name == "nonsym257":
        n = 257
        t = band(n, 24, 9)
    else:
        n = 1037
        t = banded_triplets(n, 24, complex_=True)
    return n, nt.Matrix_ps.from_triplets(n, *t)


def fixed_steps(nt, steps=10, thr=1e-8):
    p = nt.SolverParameters()
    p.SetThreshold(thr)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(steps)
    p.SetMonitorConvergence(False)
    return p


def grown(nt, before):
    after = nt.power_vector_counts()
    return tuple(after[k] - before[k] for k in ("solves", "steps", "refused"))


SOLVER_OPERANDS = ["sym1037", "nonsym257", "hermitian1037"]


@pytest.mark.parametrize("name", SOLVER_OPERANDS)
def test_power_bounds_on_one_vector_equals_the_n_column_loop(nt, arith, name):
    n, A = solver_operand(nt, name)
    p = fixed_steps(nt)
    res = {}
    for opt in (0, 1):
        nt.set_option(OPTION, opt)
        before = nt.power_vector_counts()
        res[opt] = nt.EigenBounds.PowerBounds(A, p)
        assert grown(nt, before) == ((1, 10, 0) if opt else (0, 0, 0)), (name, opt)
    print(name, res)
    assert res[1] == pytest.approx(res[0], rel=1e-6), name


@pytest.mark.parametrize("name", SOLVER_OPERANDS)
def test_exponential_takes_the_path(nt, arith, name):
    n, A = solver_operand(nt, name)
    thr = 1e-9
    out = {}
    for opt in (0, 1):
        nt.set_option(OPTION, opt)
        p = nt.SolverParameters()
        p.SetThreshold(thr)
        Out = nt.Matrix_ps(n)
        before = nt.power_vector_counts()
        nt.ExponentialSolvers.ComputeExponential(A, Out, p)
        g = grown(nt, before)
        assert (g[0], g[2]) == ((1, 0) if opt else (0, 0)) and (g[1] >= 1) == bool(opt), (name, opt, g)
        out[opt] = Out.to_scipy().toarray()
    # (the tolerance of test_matrix_functions_golden)
    tol = max(1000 * thr, 1e-11) * max(1.0, np.abs(out[0]).max())
    print(name, np.abs(out[1] - out[0]).max(), tol)
    assert np.abs(out[1] - out[0]).max() <= tol, name


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "hermitian"])
def test_estimate_gap_takes_the_path_twice(nt, arith, cplx):
    n = 257
    H = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, 24, complex_=cplx))
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    p = nt.SolverParameters()
    p.SetThreshold(1e-9)
    p.SetConvergeDiff(1e-8)
    K = nt.Matrix_ps(n)
    _, mu = nt.DensityMatrixSolvers.TRS2(H, I, n // 2, K, p)
    gap = {}
    for opt in (0, 1):
        nt.set_option(OPTION, opt)
        before = nt.power_vector_counts()
        gap[opt] = nt.EigenSolvers.EstimateGap(H, K, mu, p)
        g = grown(nt, before)
        assert (g[0], g[2]) == ((2, 0) if opt else (0, 0)), (opt, g)
    print(gap)
    # (the tolerance of the `gap` case of test_remaining_solver_families_golden)
    assert gap[1] == pytest.approx(gap[0], rel=1e-6, abs=1e-9)


# ------------------------------------------------------------------ 4. the goldens through the new path
def test_power_goldens_on_one_vector(nt, arith):
    g = Golden("functions")
    mats = {}
    seen = 0
    nt.set_option(OPTION, 1)
    for i, c in enumerate(g.cases):
        if c["kind"] != "power":
            continue
        if c["matrix"] not in mats:
            t = g.tri(None, "M_" + c["matrix"])
            mats[c["matrix"]] = nt.Matrix_ps.from_triplets(t[0], t[2], t[3], t[4])
        p = nt.SolverParameters()
        p.SetThreshold(c["thr"])
        p.SetConvergeDiff(c["conv"])
        before = nt.power_vector_counts()
        got = nt.EigenBounds.PowerBounds(mats[c["matrix"]], p)
        grew = grown(nt, before)
        print(i, c["matrix"], got, c["bound"], grew)
        assert grew[0] == 1 and grew[1] >= 1 and grew[2] == 0, (i, grew)
        assert got == pytest.approx(c["bound"], rel=1e-6), i
        seen += 1
    assert seen >= 1


# ------------------------------------------------------------------ 5. memory
def test_a_solve_holds_the_gather_form_and_three_vectors(nt):
    """N = 65 536, h = 16, 60 fixed steps in a fresh process: in-use + cached bytes grow by at most 4 (12 nnz + 24 N) -- the gather
    form and three vectors; the factor covers slice padding, the transpose's sort buffers and pool granularity.  The N-column
    loop holds 961 rows x N entries x 12 B, about 750 MB, per copy of its iterate on this input: it cannot pass."""
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "power_vector_worker.py"), "memory"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["counts"] == [1, 60, 0]
    bound = 4 * (12 * rep["nnz"] + 24 * rep["n"])
    assert rep["after"] - rep["before"] <= bound, (rep, bound)


# ------------------------------------------------------------------ 6. several ranks
def run_world(world, tmp_path):
    out = str(tmp_path / ("pv%d" % world))
    name = "p%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name, NTPOLY_AMD_SHM_MB="8")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "power_vector_worker.py"),
                                       "ranks", out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=300)
            logs.append(o)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        try:
            os.unlink("/dev/shm/ntpoly_amd_" + name)
        except OSError:
            pass
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d of %d failed:\n%s" % (r, world, logs[r][-3000:])
    return [json.load(open(out + ".%d.json" % r)) for r in range(world)]


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    return run_world(1, tmp_path_factory.mktemp("pv_ref"))[0]


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_agree_bit_for_bit_and_with_one_rank(world, one_rank, tmp_path):
    parts = run_world(world, tmp_path)
    for arith in ("fma", "unfused"):
        for name in SOLVER_OPERANDS + ["n5"]:
            key = "%s_%s" % (name, arith)
            bounds = [p[key]["bound_hex"] for p in parts]
            print(world, key, bounds, one_rank[key]["bound_hex"])
            assert len(set(bounds)) == 1, (key, bounds)
            assert float.fromhex(bounds[0]) == pytest.approx(float.fromhex(one_rank[key]["bound_hex"]), rel=1e-6), key
            for p in parts:
                assert p[key]["counts"] == [1, 10, 0], (key, p[key]["counts"])
    if world == 3:
        # n = 5 on three ranks: an uneven split of the columns
        assert sorted(p["n5_width"] for p in parts) == [1, 2, 2]
