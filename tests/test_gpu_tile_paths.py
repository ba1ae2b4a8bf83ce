"""GPU: every instantiation of the MFMA tile kernel (csrc/spgemm_tile.hip k_spgemm_tile<EPI, NW, R, LAB, OFF32>) and every way it
brings in the multiplier tile, pinned to the oracle's FMA mode bit for bit.  A default run takes ONE of these paths (R = 2, 32-bit
offsets, the right operand as pairs of rows of its runs); the others run when an operand reaches 4 GB, when the left operand
has a halo (panel products across ranks), or with other geometries -- none of which a test-sized operand on one GPU reaches
except through the options tile_rows, tile_waves, tile_off32, tile_bbuf, tile_runs_only and plan_ahead.

Every case PROVES the path it names through the launcher's own record (nt.last_tile_launch(), spgemm_tile.hpp TileLaunchInfo:
the instantiation that was launched and `bsrc`, where the multiplier tile came from -- 0 prepared tiles, 1 the runs through
64-bit pointers, 2 the runs through the buffer per element, 3 the runs as pairs of rows): an option the launcher ignored would
fail the case, not make it vacuous.

 A. fused TRS2 steps (EPI 1: X*X, EPI 2: 2X - X*X) from the X0 of operands(n, h): sigma, pattern and values of the iterate equal
    to the oracle's after every step; energy and trace equal as floats across the option settings.
 B. products of a solver session (EPI 0, the right operand from its runs): C = alpha A B for A != B and A = B.
 C. the label-aware instantiation (LAB): TRS2 on a relabelled band, every setting equal to the default run bit for bit and the
    default run equal to the oracle's solve (pattern; values 1e-13: the label-aware kernel walks k in position order).

FMA arithmetic throughout.  Every option is set before the matrices of a run are built (the slab form's rows are aligned to
16 x tile_rows) and the engine's caches are dropped between settings."""
import numpy as np
import pytest

from gen import banded_triplets, permuted_banded_triplets

pytestmark = pytest.mark.gpu

DEFAULTS = dict(tile_rows=2, tile_waves=0, tile_off32=1, tile_bbuf=2, tile_runs_only=1, plan_ahead=1, tile_skip=1)
GEOMETRIES = [(1, 4), (1, 8), (2, 4), (2, 8), (4, 4), (4, 8)]          # (tile_rows, tile_waves)
# (tile_off32, tile_bbuf, tile_runs_only): the right operand from its runs in each of the three ways, then from prepared tiles
SETTINGS = [(o, b, 1) for o in (1, 0) for b in (2, 1, 0)] + [(o, 2, 0) for o in (1, 0)]
RUN_SETTINGS = [s for s in SETTINGS if s[2] == 1]
BSRC_OF_BBUF = {2: 3, 1: 2, 0: 1}

# n, h, threshold, steps: both sigma signs occur, no iterate stores a zero, the plan fits the kernel's LDS bound
#   200 / 4:    k groups KG = 6, 8, 11 ... 15 (KG = 6 = TILE_PF: the pipeline's prologue is the whole loop), 12.5 blocks
#   777 / 12:   no multiple of the tile height, ragged last block
#   1024 / 24:  max_kn 64 .. 193, tiles are skipped
#   640 / 190:  max_kn beyond 382 in EVERY step: the pair path's fallback inside the kernel to one load per element, the tail loop
#               behind the first 384 rows, more than 64 KB of LDS
#   640 / 186:  max_kn beyond 382 in the first step only
STEP_SHAPES = [(200, 4, 1e-6, 8), (777, 12, 1e-6, 10), (1024, 24, 1e-8, 10), (640, 190, 1e-8, 5), (640, 186, 1e-6, 5)]
# the first step starts from compressed columns (kernels.hip spgemm(): the expansion builds multiplier tiles, bsrc 0 whatever the
# options say) and its result still carries tiles (fuse->result: R.slab->tiles = fz_tiles), which the second step reads
# (slab_step: "in.tiles.p == nullptr" decides); with tile_runs_only the results of slab_step carry runs only, so the right operand
# comes from the runs from the THIRD step on
FIRST_STEP_FROM_RUNS = 2
# ... where the step from compressed columns reaches the tile kernel at all.  spgemm() takes the slab / tile path for "dense runs"
# only, and one of its tests is on the mean length of the expanded columns in their aligned slots (kernels.hip):
#     (double)slab_tot[0] >= 48.0 * (double)hstats[18];  // mean run of the non-empty columns >= 48 rows
# with slots of k_span_aligned, "(l / al + 1) * al - f / al * al", al = 16 x tile_rows.  The narrow bands miss it at the small
# alignments -- (200, 4) with one and two rows per lane, (777, 12) with one: the step is then an unfused product on another kernel
# and the iterate never reaches slab form.  takes_columns() restates the test; run_steps() asserts that the engine decides the
# same way (no launch of the tile kernel in the record) and, where it declines, brings X0 into slab form through a product of a
# solver session instead (X = I X0: slab_multiply has no such test) -- the steps then run on the kernel all the same, from an
# iterate that carries runs only and its segment maxima from the FIRST step on.


def takes_columns(n, h, rows):
    col, row, _ = operands(n, h)[1]
    first = np.full(n, n, dtype=np.int64)
    last = np.full(n, -1, dtype=np.int64)
    np.minimum.at(first, col - 1, row - 1)
    np.maximum.at(last, col - 1, row - 1)
    al = 16 * rows
    return int(((last // al + 1) * al - first // al * al).sum()) >= 48 * n


# n, h, holes, threshold, alpha
PRODUCT_CASES = [(200, 4, 0.0, 1e-6, 1.0), (777, 12, 0.3, 1e-3, 2.0), (1000, 40, 0.2, 1e-6, -0.75), (640, 190, 0.05, 1e-8, 0.5)]
# diagonal of banded_triplets: -1 + 2 k / 1000 + shift, k = 0 .. 999 -- with these shifts no entry is zero (asserted below)
PRODUCT_SHIFTS = (0.0005, 0.1005)

LAB_N, LAB_H, LAB_SEED, LAB_THR, LAB_ITERS = 1024, 24, 7, 1e-8, 8
LAB_GEOMETRIES = [(1, 4), (2, 4), (2, 8)]


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture()
def fma(nt):
    from oracle import oracle_py as O
    nt.set_option("spgemm_fma", 1)
    O.set_fma(True)
    nt.release_cache()
    yield O
    O.set_fma(False)
    nt.set_option("spgemm_fma", 0)
    for name, value in DEFAULTS.items():
        nt.set_option(name, value)
    nt.release_cache()


def configure(nt, rows, waves, off32, bbuf, runs_only, plan_ahead=1):
    nt.release_cache()
    for name, value in dict(DEFAULTS, tile_rows=rows, tile_waves=waves, tile_off32=off32, tile_bbuf=bbuf, tile_runs_only=runs_only,
                            plan_ahead=plan_ahead).items():
        nt.set_option(name, value)


def srt(t):
    c, r, v = t
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def exact(got, want, what):
    g, w = srt(got), srt(want)
    assert len(g[2]) == len(w[2]), "%s: %d vs %d entries" % (what, len(g[2]), len(w[2]))
    assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), what + ": pattern differs"
    assert np.array_equal(g[2], w[2]), "%s: values differ, max |d| = %g" % (what, np.abs(g[2] - w[2]).max())


def want_off32(off32, rows, nw):
    # (launch_spgemm_tile by_off: "if constexpr ((NW == 4 || NW == 8) && RR <= 2)" -- four rows per lane have no OFF32 instantiation)
    return 1 if (off32 != 0 and rows <= 2 and nw in (4, 8)) else 0


# ------------------------------------------------------------------ A. fused steps
_operands = {}


def operands(n, h):
    """(triplets of H, triplets of X0 = (e_max I - H) / (e_max - e_min) with Gershgorin bounds) -- X0 made HERE, so that the
    engine and the oracle start from the same bits; computed once per shape and never changed"""
    if (n, h) not in _operands:
        col, row, val = banded_triplets(n, h)
        radius = np.zeros(n)
        centre = np.zeros(n)
        off = col != row
        np.add.at(radius, col[off] - 1, np.abs(val[off]))
        centre[col[~off] - 1] = val[~off]
        e_min, e_max = float((centre - radius).min()), float((centre + radius).max())
        x = np.where(off, -val, e_max - val) * (1.0 / (e_max - e_min))
        for a in (col, row, val, x):
            a.setflags(write=False)
        _operands[(n, h)] = ((col, row, val), (col, row, x))
    return _operands[(n, h)]


_oracle_steps = {}


def oracle_steps(O, n, h, thr, steps):
    """[(sigma, sorted triplets of X) per step] of the oracle in FMA mode (trace -> sigma, X2 = X X with the threshold, X <- 2 X - X2
    through ScaleMatrix / IncrementMatrix or X <- X2); once per shape"""
    key = (n, h, thr, steps)
    if key not in _oracle_steps:
        assert O.get_fma()
        Xo = O.Mat.from_triplets(n, n, *operands(n, h)[1])
        seq = []
        for it in range(steps):
            sigma = -1.0 if (n / 2.0 - O.trace(Xo)) < 0.0 else 1.0
            X2o = O.ps_multiply(Xo, Xo, None, 1.0, 0.0, thr)
            if sigma > 0.0:
                O.scale(Xo, 2.0)
                Xo = O.increment(X2o, Xo, -1.0, thr)
            else:
                Xo = X2o
            trip = srt(Xo.triplets())
            assert np.all(trip[2] != 0.0)   # (no stored zero: the slab form could not hold it)
            seq.append((sigma, trip))
        assert {s for s, _ in seq} == {-1.0, 1.0}   # (both fused epilogues)
        _oracle_steps[key] = seq
    return _oracle_steps[key]


def fused_and_launches(nt):
    f = nt.fusion_counts()
    return f["square"] + f["update"], f["repeated"], nt.last_tile_launch()["launches"]


def run_steps(nt, n, h, thr, steps, rows):
    """`steps` TRS2 steps from X0 under the options as they stand -> ([(sigma, energy, trace, triplets of X, record of the step's
    launch)], X0 came from compressed columns); asserts that every step was ONE fused step on ONE launch of the tile kernel and
    none was repeated"""
    h_trip, x_trip = operands(n, h)
    H = nt.Matrix_ps.from_triplets(n, *h_trip)
    X = nt.Matrix_ps.from_triplets(n, *x_trip)
    X2 = nt.Matrix_ps(n)
    from_columns = takes_columns(n, h, rows)
    if not from_columns:
        # (unreachable from compressed columns by design -- the line quoted above: the step runs, unfused, on no tile kernel)
        nt.reset_spgemm_accum()
        c0 = fused_and_launches(nt)
        nt.trs2_step(X, X2, H, n / 2.0, thr, None)
        assert fused_and_launches(nt) == c0 and c0[2] == 0, (c0, fused_and_launches(nt), nt.last_tile_launch())
        X0 = nt.Matrix_ps.from_triplets(n, *x_trip)
        I = nt.Matrix_ps(n)
        I.FillIdentity()
        X, X2 = nt.Matrix_ps(n), nt.Matrix_ps(n)
        with nt.solver_session(False):
            p0 = nt.slab_algebra_counts()
            X.Gemm(I, X0, None, 1.0, 0.0, 0.0)
            p1 = nt.slab_algebra_counts()
        assert p1["products"] - p0["products"] == 1 and p1["refusals"] == p0["refusals"], (p0, p1)
        Y = nt.Matrix_ps(n)
        nt.lib.CopyMatrix_ps_wrp(X.ih, Y.ih)
        exact(Y.triplets(), x_trip, "I X0 = X0, n=%d h=%d" % (n, h))
    nt.reset_spgemm_accum()
    assert nt.last_tile_launch()["launches"] == 0
    log, tr = [], None
    for it in range(steps):
        c0 = fused_and_launches(nt)
        sigma, energy, tr = nt.trs2_step(X, X2, H, n / 2.0, thr, tr)
        c1, rec = fused_and_launches(nt), nt.last_tile_launch()
        assert c1[1] == c0[1], (it, c0, c1)
        assert c1[0] - c0[0] == 1 and c1[2] - c0[2] == 1, (it, c0, c1, rec)
        Y = nt.Matrix_ps(n)   # (read from a copy: any other entry point packs the matrix it is given, and the next step on X
        nt.lib.CopyMatrix_ps_wrp(X.ih, Y.ih)   # would start from compressed columns; CopyMatrix leaves a slab-form source as it is)
        log.append((sigma, energy, tr, Y.triplets(), rec))
    return log, from_columns


def check_steps(log, from_columns, seq, what, rows, waves, off32, bbuf, runs_only, n, h):
    """the record of every step names the path the options ask for, and the iterates are the oracle's"""
    first_from_runs = FIRST_STEP_FROM_RUNS if from_columns else 0
    for it, ((sigma, energy, trace, trip, rec), (sigma_o, trip_o)) in enumerate(zip(log, seq)):
        tag = "%s step %d %r" % (what, it, rec)
        assert sigma == sigma_o, tag
        assert rec["epi"] == (2 if sigma > 0.0 else 1), tag
        assert rec["rows"] == rows and rec["labelled"] == 0, tag
        assert rec["nw"] == waves if waves else rec["nw"] in (4, 8), tag
        assert rec["off32"] == want_off32(off32, rows, rec["nw"]), tag
        # (an iterate that came out of the session product carries runs only whatever tile_runs_only says, until a step without
        # the option has written tiles)
        from_runs = it >= first_from_runs if runs_only != 0 else (not from_columns and it == 0)
        assert rec["bsrc"] == (BSRC_OF_BBUF[bbuf] if from_runs else 0), tag
        if (n, h) == (640, 190) or ((n, h) == (640, 186) and it == 0):
            assert rec["max_kn"] > 382, tag
        # (spgemm_tile_skips: "L.rows == 2 && !L.labelled && g.off32 && (g.nw == 4 || g.nw == 8)"; the step from compressed columns
        # passes no maxima)
        assert rec["skip"] == (1 if ((it > 0 or not from_columns) and rows == 2 and rec["off32"] == 1) else 0), tag
        exact(trip, trip_o, "%s step %d vs oracle" % (what, it))


def same_sums(log, first, what):
    for it, (a, b) in enumerate(zip(log, first)):
        assert a[1] == b[1] and a[2] == b[2], "%s step %d: energy %r vs %r, trace %r vs %r" % (what, it, a[1], b[1], a[2], b[2])


@pytest.mark.parametrize("rows,waves", GEOMETRIES)
@pytest.mark.parametrize("n,h,thr,steps", STEP_SHAPES)
def test_fused_steps_vs_oracle(nt, fma, n, h, thr, steps, rows, waves):
    """EPI 1 and EPI 2 at one geometry, the right operand from its runs in all three ways and from prepared tiles, with 32-bit
    offsets and with 64-bit addresses: every step on the path it names (the record), sigma and the iterate equal to the oracle's
    bit for bit after every step, energy and trace equal as floats across the settings"""
    seq = oracle_steps(fma, n, h, thr, steps)
    first, seen = None, set()
    for off32, bbuf, runs_only in SETTINGS:
        configure(nt, rows, waves, off32, bbuf, runs_only)
        log, from_columns = run_steps(nt, n, h, thr, steps, rows)
        what = "n=%d h=%d R=%d NW=%d off32=%d bbuf=%d runs_only=%d from_columns=%d" % (n, h, rows, waves, off32, bbuf, runs_only, from_columns)
        print(what, "max_kn", [s[4]["max_kn"] for s in log], "bsrc", [s[4]["bsrc"] for s in log], "skip", [s[4]["skip"] for s in log],
              "energy", [s[1] for s in log])
        check_steps(log, from_columns, seq, what, rows, waves, off32, bbuf, runs_only, n, h)
        first = first or log
        same_sums(log, first, what)
        seen |= {(s[4]["epi"], s[4]["off32"], s[4]["bsrc"]) for s in log}
    # (what the loop is for: both epilogues; with and without 32-bit offsets where the geometry has them, from all four sources)
    print("reached <EPI, NW %d, R %d, LAB 0>: (epi, off32, bsrc)" % (waves, rows), sorted(seen))
    offs = (0, 1) if rows <= 2 else (0,)
    assert {e for e, _, _ in seen} == {1, 2}, sorted(seen)
    assert {(o, b) for _, o, b in seen} == {(o, b) for o in offs for b in (0, 1, 2, 3)}, sorted(seen)


@pytest.mark.parametrize("n,h,thr,steps", STEP_SHAPES)
def test_fused_steps_without_the_plan_left_behind(nt, fma, n, h, thr, steps):
    """default geometry (two rows per lane; four or eight waves by the LDS a block needs) with plan_ahead = 0: every step makes its
    own plan and reads it back before the launch"""
    seq = oracle_steps(fma, n, h, thr, steps)
    first = None
    for off32, bbuf, runs_only in SETTINGS:
        configure(nt, 2, 0, off32, bbuf, runs_only, plan_ahead=0)
        log, from_columns = run_steps(nt, n, h, thr, steps, 2)
        what = "n=%d h=%d plan_ahead=0 off32=%d bbuf=%d runs_only=%d from_columns=%d" % (n, h, off32, bbuf, runs_only, from_columns)
        print(what, "nw", [s[4]["nw"] for s in log], "max_kn", [s[4]["max_kn"] for s in log])
        check_steps(log, from_columns, seq, what, 2, 0, off32, bbuf, runs_only, n, h)
        first = first or log
        same_sums(log, first, what)


_sums = {}


def geometry_sums(nt, n, h, thr, steps):
    """{(tile_rows, tile_waves, plan_ahead): ([energy per step], [trace per step])} at the default tile_off32 / tile_bbuf /
    tile_runs_only, the default geometry with and without plan_ahead first; once per shape"""
    key = (n, h, thr, steps)
    if key not in _sums:
        out = {}
        for rows, waves, ahead in [(2, 0, 1), (2, 0, 0)] + [(r, w, 1) for r, w in GEOMETRIES]:
            configure(nt, rows, waves, 1, 2, 1, plan_ahead=ahead)
            log, _ = run_steps(nt, n, h, thr, steps, rows)
            out[(rows, waves, ahead)] = ([s[1] for s in log], [s[2] for s in log])
            print("n=%d h=%d R=%d NW=%d plan_ahead=%d" % (n, h, rows, waves, ahead), "energy", out[(rows, waves, ahead)][0],
                  "trace", out[(rows, waves, ahead)][1])
        _sums[key] = out
    return _sums[key]


@pytest.mark.parametrize("n,h,thr,steps", STEP_SHAPES)
def test_energy_and_trace_do_not_depend_on_the_geometry(nt, fma, n, h, thr, steps):
    """energy and trace of every step equal as floats across the six geometries and plan_ahead = 0 (across tile_off32, tile_bbuf
    and tile_runs_only: inside the cases above).  The epilogue adds a tile's terms of dot(X, D) per lane and per tile of 16 R
    rows, so with one and four rows per lane the kernel adds the energy once more in the order of two (spgemm_tile.hip ESUM2):
    without that pass the energies differ in their last place between tile_rows 1, 2 and 4."""
    sums = geometry_sums(nt, n, h, thr, steps)
    ref = sums[(2, 0, 1)]
    for key, (energy, trace) in sums.items():
        print(key, "energy - energy(default), per step:", [a - b for a, b in zip(energy, ref[0])])
    for key, (energy, trace) in sums.items():
        assert trace == ref[1], (key, trace, ref[1])
        assert energy == ref[0], (key, energy, ref[0])


# ------------------------------------------------------------------ B. session products
_products = {}


def holes_pair(n, h, holes, seed):
    """two banded matrices with random holes, the diagonal kept (tests/test_gpu_fma.py holes_pair with the shifts above)"""
    rng = np.random.default_rng(seed)
    mats = []
    for t in range(2):
        col, row, val = banded_triplets(n, h, shift=PRODUCT_SHIFTS[t])
        keep = (rng.random(len(val)) >= holes) | (col == row)
        mats.append((col[keep], row[keep], val[keep] * (1.0 + 0.01 * t)))
    return mats


def product_case(O, n, h, holes, thr, alpha):
    """(the two operands, alpha A B and alpha A A of the oracle in FMA mode); once per case"""
    key = (n, h, holes, thr, alpha)
    if key not in _products:
        assert O.get_fma()
        mats = holes_pair(n, h, holes, n + h)
        for m in mats:
            assert np.all(m[2] != 0.0)   # (a stored zero would turn the operand into a read-only view)
            for a in m:
                a.setflags(write=False)
        Ao, Bo = O.Mat.from_triplets(n, n, *mats[0]), O.Mat.from_triplets(n, n, *mats[1])
        want = [srt(O.ps_multiply(Ao, Yo, None, alpha, 0.0, thr).triplets()) for Yo in (Bo, Ao)]
        _products[key] = (mats, want)
    return _products[key]


@pytest.mark.parametrize("rows,waves", GEOMETRIES)
@pytest.mark.parametrize("n,h,holes,thr,alpha", PRODUCT_CASES)
def test_session_products_vs_oracle(nt, fma, n, h, holes, thr, alpha, rows, waves):
    """EPI 0 with the right operand from its runs, as the solver loops multiply inside their sessions (kernels.hip slab_multiply):
    A * B and A * A at one geometry, the runs read in all three ways, with 32-bit offsets and with 64-bit addresses -- bit for bit
    the oracle's product.  (h >= 4: a thinner operand goes to the gather kernels of spgemm_thin.hip, not to the tile kernel.)"""
    mats, want = product_case(fma, n, h, holes, thr, alpha)
    seen = set()
    for off32, bbuf, _ in RUN_SETTINGS:
        configure(nt, rows, waves, off32, bbuf, 1)
        A = nt.Matrix_ps.from_triplets(n, *mats[0])
        B = nt.Matrix_ps.from_triplets(n, *mats[1])
        nt.reset_spgemm_accum()
        for Y, w, tag in ((B, want[0], "A*B"), (A, want[1], "A*A")):
            what = "%s n=%d h=%d R=%d NW=%d off32=%d bbuf=%d" % (tag, n, h, rows, waves, off32, bbuf)
            with nt.solver_session(False):
                c0, l0 = nt.slab_algebra_counts(), nt.last_tile_launch()["launches"]
                Cm = nt.Matrix_ps(n)
                Cm.Gemm(A, Y, None, alpha, 0.0, thr)
                c1, rec, thin = nt.slab_algebra_counts(), nt.last_tile_launch(), nt.last_spgemm_thin()
                got = Cm.triplets()
            print(what, rec)
            assert c1["products"] - c0["products"] == 1 and c1["refusals"] == c0["refusals"], (what, c0, c1)
            # (SpgemmStats::thin of the last product, which the library reports through last_spgemm_thin())
            assert thin == 0 and rec["launches"] - l0 == 1, (what, thin, rec)
            assert rec["epi"] == 0 and rec["rows"] == rows and rec["nw"] == waves and rec["labelled"] == 0 and rec["skip"] == 0, (what, rec)
            assert rec["off32"] == want_off32(off32, rows, waves) and rec["bsrc"] == BSRC_OF_BBUF[bbuf], (what, rec)
            if (n, h) == (640, 190):
                assert rec["max_kn"] > 382, (what, rec)   # (the pair path's fallback inside the kernel, the tail loop)
            exact(got, w, what)
            seen.add((rec["off32"], rec["bsrc"]))
    assert seen == {(o, b) for o in ((0, 1) if rows <= 2 else (0,)) for b in (1, 2, 3)}, sorted(seen)


# ------------------------------------------------------------------ C. the label-aware instantiation
_lab = {}


def lab_operand():
    if "h" not in _lab:
        _lab["h"] = permuted_banded_triplets(LAB_N, LAB_H, LAB_SEED)
        for a in _lab["h"]:
            a.setflags(write=False)
    return _lab["h"]


def lab_solve(nt):
    """TRS2, LAB_ITERS fixed iterations on the relabelled band -> (sigma sequence, entry counts, sorted triplets of the density,
    fused steps, the record of the last launch)"""
    n = LAB_N
    H = nt.Matrix_ps.from_triplets(n, *lab_operand())
    ISQ = nt.Matrix_ps(n)
    ISQ.FillIdentity()
    p = nt.SolverParameters()
    p.SetConvergeDiff(1e-30)
    p.SetThreshold(LAB_THR)
    p.SetMaxIterations(LAB_ITERS)
    p.SetMonitorConvergence(False)
    K = nt.Matrix_ps(n)
    nt.reset_spgemm_accum()
    f0 = nt.fusion_counts()
    nt.DensityMatrixSolvers.TRS2(H, ISQ, n / 2.0, K, p)
    f1, rec, tr = nt.fusion_counts(), nt.last_tile_launch(), nt.solver_trace()
    assert tr["iterations"] == LAB_ITERS and f1["repeated"] == f0["repeated"], (tr["iterations"], f0, f1)
    fused = f1["square"] + f1["update"] - f0["square"] - f0["update"]
    return np.asarray(tr["sigma"]), np.asarray(tr["nnz"]), srt(K.triplets()), fused, rec


def lab_default(nt):
    if "default" not in _lab:
        configure(nt, 2, 0, 1, 2, 1)
        _lab["default"] = lab_solve(nt)
    return _lab["default"]


def check_lab_record(fused, rec, rows, waves, off32, bbuf, what):
    # (every iteration was a fused step on the label-aware kernel: a band order was found at this size)
    assert fused == LAB_ITERS and rec["launches"] == LAB_ITERS, (what, fused, rec)
    assert rec["labelled"] == 1 and rec["epi"] in (1, 2) and rec["rows"] == rows and rec["skip"] == 0, (what, rec)
    assert rec["nw"] == waves if waves else rec["nw"] in (4, 8), (what, rec)
    # (the last of the eight steps: the iterate has carried runs only since the second)
    assert rec["off32"] == want_off32(off32, rows, rec["nw"]) and rec["bsrc"] == BSRC_OF_BBUF[bbuf], (what, rec)


def test_label_aware_default_run_vs_oracle(nt, fma):
    """n = 1024, halfband 24, seed 7: the default run against the oracle's solve of the same relabelled matrix in FMA mode --
    sigma of every iteration, the density with the same pattern and values to 1e-13 (the label-aware kernel walks k in position
    order: the bound tests/test_gpu_scale.py states for this path)"""
    O = fma
    sigma, nnz, trip, fused, rec = lab_default(nt)
    print("default", rec, "sigma", sigma, "nnz", nnz)
    check_lab_record(fused, rec, 2, 0, 1, 2, "default")
    Ho = O.Mat.from_triplets(LAB_N, LAB_N, *lab_operand())
    Ko, e_o, mu_o, tro = O.density("trs2", Ho, O.Mat.identity(LAB_N), LAB_N / 2.0,
                                   O.params(converge_diff=1e-30, max_iterations=LAB_ITERS, threshold=LAB_THR, monitor_convergence=False))
    assert tro["iterations"] == LAB_ITERS and np.array_equal(sigma, np.asarray(tro["sigma"]))
    w = srt(Ko.triplets())
    assert len(trip[2]) == len(w[2]) and np.array_equal(trip[0], w[0]) and np.array_equal(trip[1], w[1])
    assert np.abs(trip[2] - w[2]).max() <= 1e-13


@pytest.mark.parametrize("rows,waves", LAB_GEOMETRIES)
def test_label_aware_steps_equal_the_default_run(nt, fma, rows, waves):
    """LAB at one geometry, the right operand from its runs in all three ways, with 32-bit offsets and with 64-bit addresses:
    sigma sequence, entry counts per iteration and the density's triplets equal to the default run bit for bit"""
    sigma0, nnz0, trip0, _, _ = lab_default(nt)
    for off32, bbuf, _ in RUN_SETTINGS:
        configure(nt, rows, waves, off32, bbuf, 1)
        sigma, nnz, trip, fused, rec = lab_solve(nt)
        what = "LAB R=%d NW=%d off32=%d bbuf=%d" % (rows, waves, off32, bbuf)
        print(what, rec)
        check_lab_record(fused, rec, rows, waves, off32, bbuf, what)
        assert np.array_equal(sigma, sigma0) and np.array_equal(nnz, nnz0), (what, sigma, sigma0, nnz, nnz0)
        exact(trip, trip0, what)
