"""GPU: PM purification with its iterate kept in slab form (option pm_session; csrc/slab_extra.hip k_pm_sigma / k_pm_update,
engine.hpp ps_pm_sigma / ps_pm_update).  Whenever sigma > 1/2 the update scales the iterate by a1 = 0: compressed columns then
hold stored zeros, and AddSparseVectors copies a column's tail unfiltered, so a stored zero beyond the other operand's last row
survives and steers the merges that follow.  The fused path keeps zero-free runs and carries those rows in a list.

The kernels are reached with crafted operands through nt.pm_fused_step and are compared with (a) the vocabulary on compressed
columns (slab_algebra = 0: ScaleMatrix and IncrementMatrix of the C ABI) and (b) a numpy restatement of AddSparseVectors.f90
written here -- never with the fused code itself.  numpy's float64 products and sums are the correctly rounded ones the kernels
spell as __dmul_rn / __dadd_rn, so the update is compared bit for bit.  A stored zero has a sign in compressed columns (0 x a
negative entry is -0.0) that a row list does not carry: stored zeros are compared as rows whose value is zero."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from gen import banded_triplets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 259   # (not a multiple of the 4 waves of a workgroup)


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture(params=[1, 0], ids=["fma", "unfused"])
def fma(nt, request):
    """both arithmetic modes: slots padded to the tile kernel's row alignment (16 x tile_rows), and runs packed back to back"""
    nt.set_option("spgemm_fma", request.param)
    yield request.param
    nt.set_option("spgemm_fma", 0)
    nt.set_option("slab_algebra", 1)
    nt.set_option("pm_session", 1)


# ------------------------------------------------------------------ operands
def _runs(rng, n, empty, diag_only):
    """{column: (rows, values)}: a run around the diagonal with half-widths 6..90 drawn per side, ~12 % holes inside,
    values log-uniform in [1e-6, 1] with a random sign"""
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


@pytest.fixture(scope="module")
def operands():
    rng = np.random.default_rng(20261019)
    # empty columns (one operand, two, all three), a diagonal-only column; columns 0 and N - 1 are ordinary runs
    X = _runs(rng, N, empty={7, 40, 41, 100}, diag_only={13})
    X2 = _runs(rng, N, empty={8, 40, 100, 200}, diag_only={13})
    X3 = _runs(rng, N, empty={9, 41, 100, 201}, diag_only={13})
    # 40 listed rows beyond the last non-zero of their columns of X (some beyond X2 and X3 too, some not)
    Z = {}
    cand = [j for j in X if X[j][0][-1] < N - 2]
    while sum(len(v) for v in Z.values()) < 40:
        j = int(rng.choice(cand))
        r = int(min(N - 1, X[j][0][-1] + rng.integers(1, 30)))
        Z[j] = np.union1d(Z.get(j, np.array([], dtype=np.int64)), [r])
    return X, X2, X3, Z


def _triplets(cols, zeros=None):
    c, r, v = [], [], []
    for j in sorted(set(cols) | set(zeros or {})):
        rows, vals = cols.get(j, (np.array([], dtype=np.int64), np.array([])))
        if zeros and j in zeros:
            rows = np.concatenate([rows, zeros[j]])
            vals = np.concatenate([vals, np.zeros(len(zeros[j]))])
            o = np.argsort(rows)
            rows, vals = rows[o], vals[o]
        c += [j + 1] * len(rows)
        r += list(rows + 1)
        v += list(vals)
    return np.array(c, dtype=np.int32), np.array(r, dtype=np.int32), np.array(v, dtype=np.float64)


def _matrix(nt, cols, zeros=None, n=N):
    c, r, v = _triplets(cols, zeros)
    M = nt.Matrix_ps.from_triplets(n, c, r, v)
    assert len(M.triplets()[2]) == len(v)   # (stored zeros are kept)
    return M


def _pattern_matrix(nt, zeros, n=N):
    if not zeros:
        return nt.Matrix_ps(n)
    return _matrix(nt, {j: (rows, np.ones(len(rows))) for j, rows in zeros.items()}, n=n)


def srt(t):
    c, r, v = t
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


# ------------------------------------------------------------------ AddSparseVectors.f90, restated
def add_sparse(ra, va, rb, vb, alpha, thr, log=None):
    """c = alpha a + b on sorted sparse vectors: inside the overlap of the two lists an entry is kept iff |value| > thr, once one
    list is exhausted the tail of the other is copied unfiltered.  log (optional) collects (row, branch) records."""
    rc, vc = [], []
    A, B = 0, 0
    while A < len(ra) and B < len(rb):
        wa, wb = alpha * va[A], vb[B]
        if ra[A] == rb[B]:
            s = wa + wb
            keep = abs(s) > thr
            if keep:
                rc.append(ra[A]); vc.append(s)
            if log is not None:
                log.append((ra[A], "both_kept" if keep else "both_filtered"))
            A += 1
            B += 1
        elif ra[A] > rb[B]:
            keep = abs(wb) > thr
            if keep:
                rc.append(rb[B]); vc.append(wb)
            if log is not None:
                log.append((rb[B], "b_kept" if keep else "b_filtered"))
            B += 1
        else:
            keep = abs(wa) > thr
            if keep:
                rc.append(ra[A]); vc.append(wa)
            if log is not None:
                log.append((ra[A], "a_kept" if keep else "a_filtered"))
            A += 1
    while A < len(ra):
        rc.append(ra[A]); vc.append(va[A] * alpha)
        if log is not None:
            log.append((ra[A], "a_tail_small" if abs(va[A] * alpha) <= thr else "a_tail"))
        A += 1
    while B < len(rb):
        rc.append(rb[B]); vc.append(vb[B])
        if log is not None:
            log.append((rb[B], "b_tail_small" if abs(vb[B]) <= thr else "b_tail"))
        B += 1
    return np.array(rc, dtype=np.int64), np.array(vc, dtype=np.float64)


EMPTY = (np.array([], dtype=np.int64), np.array([], dtype=np.float64))


def _with_zeros(col, zrows):
    rows, vals = col
    if zrows is None or len(zrows) == 0:
        return rows, vals
    rows = np.concatenate([rows, zrows])
    vals = np.concatenate([vals, np.zeros(len(zrows))])
    o = np.argsort(rows)
    return rows[o], vals[o]


def coefficients(sg):
    if sg > 0.5:
        return 0.0, 1.0 + 1.0 / sg, -1.0 / sg
    return (1.0 - 2.0 * sg) / (1.0 - sg), (1.0 + sg) / (1.0 - sg), -1.0 / (1.0 - sg)


def restated_update(X, X2, X3, Z, sg, thr):
    """(result columns {j: (rows, values)} with stored zeros, branch statistics) of ScaleMatrix(X u Z, a1); IncrementMatrix(X2, ., a2,
    thr); IncrementMatrix(X3, ., a3, thr)"""
    a1, a2, a3 = coefficients(sg)
    out, st = {}, dict(both_filtered=0, one_sided_filtered=0, small_tail_1_dropped_2=0, dropped_1_small_tail_2=0, zero_survives=0,
                       zero_dies=0, zero_from_underflow=0)
    for j in range(N):
        xr, xv = _with_zeros(X.get(j, EMPTY), Z.get(j))
        l1, l2 = [], []
        yr, yv = add_sparse(*X2.get(j, EMPTY), xr, a1 * xv, a2, thr, l1)
        fr, fv = add_sparse(*X3.get(j, EMPTY), yr, yv, a3, thr, l2)
        if len(fr):
            out[j] = (fr, fv)
        logs = l1 + l2
        st["both_filtered"] += sum(b == "both_filtered" for _, b in logs)
        st["one_sided_filtered"] += sum(b in ("a_filtered", "b_filtered") for _, b in logs)
        small1 = {r for r, b in l1 if b in ("a_tail_small", "b_tail_small")}
        st["small_tail_1_dropped_2"] += len(small1 - set(fr.tolist()))
        gone1 = {r for r, b in l1 if b.endswith("filtered")}
        st["dropped_1_small_tail_2"] += len(gone1 & {r for r, b in l2 if b in ("a_tail_small", "b_tail_small")})
        zin = set(xr[xv * a1 == 0.0].tolist())    # rows the first merge reads as stored zeros of the scaled iterate
        zout = set(fr[fv == 0.0].tolist())
        st["zero_survives"] += len(zin & zout)
        st["zero_dies"] += len(zin - zout)
        st["zero_from_underflow"] += len(zout - zin)
    return out, st


CASES = [(thr, sg, zmode) for thr in (0.0, 1e-3) for sg in (0.3, 0.7) for zmode in ("empty", "listed")]


@pytest.fixture(scope="module")
def restated(operands):
    X, X2, X3, Z = operands
    return {(thr, sg, zm): restated_update(X, X2, X3, Z if zm == "listed" else {}, sg, thr) for thr, sg, zm in CASES}


def test_the_inputs_reach_every_branch(restated):
    """from the numpy restatement alone: both present and filtered, one-sided and filtered, a tail kept below thr by the first merge and
    dropped by the second, a row the first merge drops that the second keeps as a tail below thr, a stored zero that survives and one
    that does not"""
    tot = {}
    for (thr, sg, zm), (_, st) in restated.items():
        for k, v in st.items():
            tot[k] = tot.get(k, 0) + v
        if sg > 0.5 or zm == "listed":
            assert st["zero_survives"] > 0 and st["zero_dies"] > 0, ((thr, sg, zm), st)
        if thr > 0:
            assert st["both_filtered"] > 0 and st["one_sided_filtered"] > 0, ((thr, sg, zm), st)
            assert st["small_tail_1_dropped_2"] > 0 and st["dropped_1_small_tail_2"] > 0, ((thr, sg, zm), st)
    print("branches over all cases:", tot)


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
    assert np.array_equal(cv[wv != 0.0].view(np.int64), wv[wv != 0.0].view(np.int64)) and np.all(cv[wv == 0.0] == 0.0)
    # the fused step
    nt.set_option("slab_algebra", 1)
    MX, MZ = _matrix(nt, X), _pattern_matrix(nt, Z)
    Out, Zout = nt.Matrix_ps(N), nt.Matrix_ps(N)
    before = [srt(m.triplets()) for m in (MX, MZ, M2, M3)]
    assert nt.pm_fused_step(MX, MZ, M2, M3, a1, a2, a3, thr, Out, Zout) is not None
    for m, b in zip((MX, MZ, M2, M3), before):
        a = srt(m.triplets())
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
    oc, orr, ov = srt(Out.triplets())
    zc, zr, zv = srt(Zout.triplets())
    assert np.all(ov != 0.0) and np.all(zv == 0.0)
    nzm = wv != 0.0
    assert np.array_equal(oc, wc[nzm]) and np.array_equal(orr, wr[nzm]), "non-zeros: pattern"
    assert np.array_equal(ov.view(np.int64), wv[nzm].view(np.int64)), "non-zeros: values, bit for bit"
    assert np.array_equal(zc, wc[~nzm]) and np.array_equal(zr, wr[~nzm]), "stored zeros: rows"
    print("case", (thr, sg, zmode), "entries", len(wv), "stored zeros", int((~nzm).sum()))


@pytest.mark.parametrize("thr", [0.0, 1e-3])
@pytest.mark.parametrize("zmode", ["empty", "listed"])
def test_sigma_pass(nt, fma, operands, thr, zmode):
    """trace and dot(., X) of Temp = X - X2 merged at thr against Trace / Dot of the compressed-column Temp and the restatement, to
    1e-13 x the sum of the terms' magnitudes (a reordered sum of at most 259 x 181 terms)"""
    X, X2, X3, Z = operands
    Z = Z if zmode == "listed" else {}
    tr, dt, atr, adt = 0.0, 0.0, 0.0, 0.0
    for j in range(N):
        xr, xv = _with_zeros(X.get(j, EMPTY), Z.get(j))
        rr, rv = add_sparse(*X2.get(j, EMPTY), xr, xv, -1.0, thr)
        d = rv[rr == j]
        tr += d.sum()
        atr += np.abs(d).sum()
        both, ia, ib = np.intersect1d(rr, xr, return_indices=True)
        dt += (rv[ia] * xv[ib]).sum()
        adt += np.abs(rv[ia] * xv[ib]).sum()
    nt.set_option("slab_algebra", 0)
    W = _matrix(nt, X, Z)
    M2, M3 = _matrix(nt, X2), _matrix(nt, X3)
    T = nt.Matrix_ps(W)
    T.Increment(M2, -1.0, thr)
    ctr, cdt = T.Trace(), T.Dot(W)
    nt.set_option("slab_algebra", 1)
    MX, MZ = _matrix(nt, X), _pattern_matrix(nt, Z)
    Out, Zout = nt.Matrix_ps(N), nt.Matrix_ps(N)
    got = nt.pm_fused_step(MX, MZ, M2, M3, 0.5, 1.5, -1.0, thr, Out, Zout)
    assert got is not None
    print("trace", got[0], ctr, tr, "dot", got[1], cdt, dt, "bounds", 1e-13 * atr, 1e-13 * adt)
    assert abs(ctr - tr) <= 1e-13 * atr and abs(cdt - dt) <= 1e-13 * adt, "compressed columns against the restatement"
    assert abs(got[0] - ctr) <= 1e-13 * atr and abs(got[0] - tr) <= 1e-13 * atr
    assert abs(got[1] - cdt) <= 1e-13 * adt and abs(got[1] - dt) <= 1e-13 * adt


def test_refusal_leaves_everything_as_it_was(nt, fma):
    """one column whose runs in X and X3 lie n / 2 rows apart: the union extent is beyond what the column's three slots and two pads
    bound (a slot is padded to 16 x tile_rows rows in FMA arithmetic: n is large enough for any tile_rows) -- not taken"""
    n, j = 4099, 5
    col = lambda f, l: {j: (np.arange(f, l + 1), np.linspace(0.1, 0.9, l - f + 1))}
    MX, M2, M3 = _matrix(nt, col(0, 9), n=n), _matrix(nt, col(0, 9), n=n), _matrix(nt, col(n // 2 + 1, n // 2 + 11), n=n)
    MZ, Out, Zout = nt.Matrix_ps(n), nt.Matrix_ps(n), nt.Matrix_ps(n)
    before = [srt(m.triplets()) for m in (MX, M2, M3)]
    c0 = nt.pm_session_counts()
    assert nt.pm_fused_step(MX, MZ, M2, M3, 0.5, 1.5, -1.0, 0.0, Out, Zout) is None
    assert nt.pm_session_counts() == c0
    for m, b in zip((MX, M2, M3), before):
        assert all(np.array_equal(p, q) for p, q in zip(srt(m.triplets()), b))
    assert len(Out.triplets()[2]) == 0 and len(Zout.triplets()[2]) == 0 and len(MZ.triplets()[2]) == 0
    # the same column with X3 beside X is taken
    M3 = _matrix(nt, col(4, 20), n=n)
    assert nt.pm_fused_step(MX, MZ, M2, M3, 0.5, 1.5, -1.0, 0.0, Out, Zout) is not None
    assert len(Out.triplets()[2]) == 21


# ------------------------------------------------------------------ the solver
SOLVE_N, SOLVE_H, SOLVE_THR, SOLVE_ITERS = 512, 10, 1e-8, 14


def pm_solve(nt, nel, H=None, n=SOLVE_N):
    if H is None:
        H = nt.Matrix_ps.from_triplets(n, *banded_triplets(n, SOLVE_H))
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    p = nt.SolverParameters()
    p.SetThreshold(SOLVE_THR)
    p.SetConvergeDiff(1e-30)
    p.SetMaxIterations(SOLVE_ITERS)
    p.SetMonitorConvergence(False)
    K = nt.Matrix_ps(n)
    c0, s0 = nt.pm_session_counts(), nt.slab_algebra_counts()
    e = nt.DensityMatrixSolvers.PM(H, I, float(nel), K, p)
    c1, s1 = nt.pm_session_counts(), nt.slab_algebra_counts()
    tr = nt.solver_trace()
    return dict(K=srt(K.triplets()), e=e[0] if isinstance(e, tuple) else e, iters=tr["iterations"], nnz=tr["nnz"].copy(),
                sigma=tr["sigma"].copy(), energy=tr["energy"].copy(), counts={k: c1[k] - c0[k] for k in c1},
                products=s1["products"] - s0["products"])


@pytest.mark.parametrize("nel", [128, 256, 384])
def test_solver_in_slab_form(nt, fma, nel):
    """banded_triplets(512, 10), thr 1e-8, 14 iterations, ISQ = I: sigma stays below 1/2 (nel 128), above it (384), crosses it (256).
    Option 1 against option 0: iteration counts and nnz traces equal, sigma to 1e-10, energies to 1e-10 relative, densities to 1e-9
    (the bounds test_other_purification_loops_in_slab_form holds HPCP to)"""
    import scipy.sparse as sp
    nt.set_option("pm_session", 0)
    off = pm_solve(nt, nel)
    nt.set_option("pm_session", 1)
    on = pm_solve(nt, nel)
    print("nel", nel, "sigma", on["sigma"], "counts on", on["counts"], "off", off["counts"], "products", on["products"], off["products"])
    print("nnz on ", on["nnz"].tolist())
    print("nnz off", off["nnz"].tolist())
    assert off["counts"] == dict(sigma=0, updates=0, zeros=0, left=0) and off["products"] == 0
    assert on["iters"] == off["iters"] == SOLVE_ITERS
    assert np.array_equal(on["nnz"], off["nnz"])
    assert np.max(np.abs(on["sigma"] - off["sigma"])) <= 1e-10
    assert np.all(np.abs(on["energy"] - off["energy"]) <= 1e-10 * np.abs(off["energy"]))
    G = sp.csr_matrix((on["K"][2], (on["K"][1] - 1, on["K"][0] - 1)), shape=(SOLVE_N, SOLVE_N))
    W = sp.csr_matrix((off["K"][2], (off["K"][1] - 1, off["K"][0] - 1)), shape=(SOLVE_N, SOLVE_N))
    assert abs(G - W).max() <= 1e-9
    assert on["counts"]["updates"] >= 13 and on["counts"]["left"] == 0 and on["products"] >= 26, (on["counts"], on["products"])
    if nel == 128:
        assert on["counts"]["zeros"] == 0
    else:
        assert on["counts"]["zeros"] > 0   # (the reference semantics alone gives 52 at nel = 384 and 145 at nel = 256)


def test_starting_iterate_with_a_stored_zero_leaves_the_fused_path(nt, fma):
    """a Hamiltonian that stores a zero off its diagonal: the starting iterate stores it too, its slab form is a read-only view, and the
    first sigma pass refuses -- the iterate is materialised, the session closed, the solve finishes on compressed columns (once:
    left == 1, nothing fused) with the entry counts of option 0 and its density to 1e-9"""
    import scipy.sparse as sp
    col, row, val = banded_triplets(SOLVE_N, SOLVE_H)
    val = val.copy()
    val[(col == 101) & (row == 104)] = 0.0
    val[(col == 104) & (row == 101)] = 0.0
    H = nt.Matrix_ps.from_triplets(SOLVE_N, col, row, val)
    nt.set_option("pm_session", 0)
    off = pm_solve(nt, 256, H=H)
    nt.set_option("pm_session", 1)
    on = pm_solve(nt, 256, H=H)
    print("counts", on["counts"], "products", on["products"])
    assert on["counts"] == dict(sigma=0, updates=0, zeros=0, left=1), on["counts"]
    assert on["iters"] == off["iters"] and np.array_equal(on["nnz"], off["nnz"])
    assert np.max(np.abs(on["sigma"] - off["sigma"])) <= 1e-10
    G = sp.csr_matrix((on["K"][2], (on["K"][1] - 1, on["K"][0] - 1)), shape=(SOLVE_N, SOLVE_N))
    W = sp.csr_matrix((off["K"][2], (off["K"][1] - 1, off["K"][0] - 1)), shape=(SOLVE_N, SOLVE_N))
    assert abs(G - W).max() <= 1e-9


def test_gates(nt, fma):
    """pm_session = 0 and slab_algebra = 0 are the loop on compressed columns, bit for bit the same result, counters untouched; a
    complex operand takes that loop whatever the option says"""
    nt.set_option("pm_session", 0)
    a = pm_solve(nt, 256)
    nt.set_option("pm_session", 1)
    nt.set_option("slab_algebra", 0)
    b = pm_solve(nt, 256)
    nt.set_option("slab_algebra", 1)
    for r in (a, b):
        assert r["counts"] == dict(sigma=0, updates=0, zeros=0, left=0) and r["products"] == 0
    assert a["iters"] == b["iters"] and np.array_equal(a["nnz"], b["nnz"]) and np.array_equal(a["sigma"], b["sigma"])
    assert all(np.array_equal(p, q) for p, q in zip(a["K"], b["K"]))
    Hc = nt.Matrix_ps.from_triplets(SOLVE_N, *banded_triplets(SOLVE_N, SOLVE_H, complex_=True))
    c = pm_solve(nt, 256, H=Hc)
    nt.set_option("pm_session", 0)
    d = pm_solve(nt, 256, H=Hc)
    nt.set_option("pm_session", 1)
    assert c["counts"] == dict(sigma=0, updates=0, zeros=0, left=0) == d["counts"]
    assert c["iters"] == d["iters"] and np.array_equal(c["nnz"], d["nnz"])
    assert all(np.array_equal(p, q) for p, q in zip(c["K"], d["K"]))


# ------------------------------------------------------------------ two ranks
def run_world(world, tmp_path):
    out = str(tmp_path / ("pm%d" % world))
    name = "p%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name, NTPOLY_AMD_SHM_MB="64",
                   NTPOLY_AMD_SPGEMM_FMA="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "pm_session_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
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
    return [dict(np.load(out + ".%d.npz" % r)) for r in range(world)]


def test_two_ranks_equal_one(tmp_path):
    """the nel = 256 solve as column panels on two ranks (shared-memory transport, FMA arithmetic): iteration count, nnz trace and
    pattern of K equal the one-rank run, values to 1e-8, the fused counters move on both ranks"""
    one = run_world(1, tmp_path)[0]
    two = run_world(2, tmp_path)
    cat = lambda k: np.concatenate([p[k] for p in two])
    assert np.array_equal(cat("col"), one["col"]) and np.array_equal(cat("row"), one["row"])
    assert np.max(np.abs(cat("val") - one["val"])) <= 1e-8
    assert np.array_equal(two[0]["nnz"] + two[1]["nnz"], one["nnz"])
    for r, p in enumerate(two):
        print("rank", r, "counts (sigma, updates, zeros, left)", p["counts"].tolist(), "iterations", int(p["iters"][0]))
        assert int(p["iters"][0]) == int(one["iters"][0]) == SOLVE_ITERS
        assert p["counts"][0] > 0 and p["counts"][1] > 0 and p["counts"][3] == 0, (r, p["counts"])
    assert one["counts"][2] > 0 and two[0]["counts"][2] + two[1]["counts"][2] > 0
