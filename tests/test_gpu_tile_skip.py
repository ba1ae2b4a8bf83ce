"""GPU: the tile skip of the MFMA tile kernel (option tile_skip, spgemm_tile.hip).  An iterate in slab form carries the largest
modulus of every 32 slots (SlabForm::amax); before the kernel loads anything for a tile of 32 rows x 16 columns it bounds every
entry of the tile by  sum_k max|A(tile rows, k)| * max|B(k, block columns)|  and skips the tile when the bound, inflated by
2^-30, stays at or below the threshold (and, in the update step, no column of the block has a row of X in the tile).  Such a tile
stores nothing in the unskipped kernel either, so the option may not change ONE BIT of any result: every case here runs the
same TRS2 steps (ntpoly_amd_trs2_step, what bench.py times) with the option on and off and compares sigma, energy, trace and
the iterate after every step for equality, and once against the oracle's FMA mode.  FMA arithmetic throughout (the tile kernel).

Shapes: N = 1024, halfband 24, threshold 1e-8 (a numpy restatement of the step finds 1-5 skippable tiles per block in
iterations 3-10, interior and edge blocks) and N = 777, halfband 12, threshold 1e-6 (ragged last block, a dimension that is no
multiple of the tile height)."""
import numpy as np
import pytest

from gen import banded_triplets

pytestmark = pytest.mark.gpu

SHAPES = [(1024, 24, 1e-8), (777, 12, 1e-6)]
STEPS = 10


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
    yield O
    O.set_fma(False)
    nt.set_option("spgemm_fma", 0)
    nt.set_option("tile_skip", 1)
    nt.set_option("tile_waves", 0)


def srt(t):
    c, r, v = t
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def exact(got, want, what, nan_ok=False):
    g, w = srt(got), srt(want)
    assert len(g[2]) == len(w[2]), "%s: %d vs %d entries" % (what, len(g[2]), len(w[2]))
    assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), what + ": pattern differs"
    assert np.array_equal(g[2], w[2], equal_nan=nan_ok), "%s: values differ" % what


def same_float(a, b, nan_ok=False):
    return a == b or (nan_ok and np.isnan(a) and np.isnan(b))


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


def thinned(trip, frac, seed):
    col, row, val = trip
    rng = np.random.default_rng(seed)
    keep = (rng.random(len(val)) >= frac) | (col == row)
    return col[keep], row[keep], val[keep]


def run_steps(nt, n, h_trip, x_trip, thr, steps, skip, waves=0, mutate_at=None, mutate=None):
    """`steps` TRS2 steps from X0 -> ([(sigma, energy, trace, triplets of X, tile_skip_counts so far) per step], tile_skip_counts,
    fused steps repeated)"""
    nt.set_option("tile_skip", skip)
    nt.set_option("tile_waves", waves)
    H = nt.Matrix_ps.from_triplets(n, *h_trip)
    X = nt.Matrix_ps.from_triplets(n, *x_trip)
    X2 = nt.Matrix_ps(n)
    nt.reset_spgemm_accum()
    f0 = nt.fusion_counts()
    log, tr = [], None
    for it in range(steps):
        if mutate_at is not None and it == mutate_at:
            mutate(nt, X, n)
            tr = None
        sigma, energy, tr = nt.trs2_step(X, X2, H, n / 2.0, thr, tr)
        Y = nt.Matrix_ps(n)   # (read from a copy: any other entry point packs the matrix it is given, and the next step on X
        nt.lib.CopyMatrix_ps_wrp(X.ih, Y.ih)   # would start from compressed columns; CopyMatrix leaves a slab-form source as it is)
        log.append((sigma, energy, tr, Y.triplets(), nt.tile_skip_counts()))
    counts = nt.tile_skip_counts()
    return log, counts, nt.fusion_counts()["repeated"] - f0["repeated"]


def assert_same_run(on, off, what, nan_ok=False):
    assert len(on) == len(off)
    for it, (a, b) in enumerate(zip(on, off)):
        for q, name in enumerate(("sigma", "energy", "trace")):
            assert same_float(a[q], b[q], nan_ok), "%s step %d: %s %r vs %r" % (what, it, name, a[q], b[q])
        exact(a[3], b[3], "%s step %d" % (what, it), nan_ok)


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("n,h,thr", SHAPES)
def test_steps_are_bit_identical_with_and_without_the_skip(nt, fma, n, h, thr, waves):
    """ten steps from X0: sigma, energy, trace equal as floats and the iterate equal bit for bit after every step; both sigma
    signs occur (X*X alone and 2X - X*X: both fused epilogues); tiles are skipped with the option on, none with it off, and no
    fused step is repeated"""
    h_trip, x_trip = operands(n, h)
    on, c_on, rep_on = run_steps(nt, n, h_trip, x_trip, thr, STEPS, 1, waves)
    off, c_off, rep_off = run_steps(nt, n, h_trip, x_trip, thr, STEPS, 0, waves)
    print("n=%d waves=%d: tiles tested / skipped %r (option off: %r), sigma %r" % (n, waves, c_on, c_off, [s[0] for s in on]))
    assert_same_run(on, off, "n=%d waves=%d" % (n, waves))
    assert {s[0] for s in on} == {-1.0, 1.0}, [s[0] for s in on]
    assert c_on[1] > 0 and c_on[0] >= c_on[1], c_on
    assert c_off == (0, 0), c_off
    assert rep_on == 0 and rep_off == 0


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("n,h,thr", SHAPES)
def test_steps_equal_the_oracle(nt, fma, n, h, thr, waves):
    """the same ten steps spelled with the oracle's calls in FMA mode (trace -> sigma, X2 = X X with the threshold, X <- 2 X - X2
    through ScaleMatrix / IncrementMatrix or X <- X2): pattern and values bit for bit after every step, option on"""
    O = fma
    h_trip, x_trip = operands(n, h)
    on, c_on, _ = run_steps(nt, n, h_trip, x_trip, thr, STEPS, 1, waves)
    assert c_on[1] > 0, c_on
    Xo = O.Mat.from_triplets(n, n, *x_trip)
    for it in range(STEPS):
        sigma = -1.0 if (n / 2.0 - O.trace(Xo)) < 0.0 else 1.0
        X2o = O.ps_multiply(Xo, Xo, None, 1.0, 0.0, thr)
        if sigma > 0.0:
            O.scale(Xo, 2.0)
            Xo = O.increment(X2o, Xo, -1.0, thr)
        else:
            Xo = X2o
        assert on[it][0] == sigma, (it, on[it][0], sigma)
        exact(on[it][3], Xo.triplets(), "n=%d step %d vs oracle" % (n, it))


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("thr", [0.0, 1e-12, 1e-5])
@pytest.mark.parametrize("n,h", [(1024, 24), (777, 12)])
def test_thresholds(nt, fma, n, h, thr, waves):
    """a threshold of zero (only a bound of exactly zero may skip), a tiny and a coarse one: identical with the option on and off"""
    h_trip, x_trip = operands(n, h)
    on, c_on, rep_on = run_steps(nt, n, h_trip, x_trip, thr, STEPS, 1, waves)
    off, c_off, rep_off = run_steps(nt, n, h_trip, x_trip, thr, STEPS, 0, waves)
    print("n=%d thr=%g waves=%d: tiles tested / skipped %r" % (n, thr, waves, c_on))
    assert_same_run(on, off, "n=%d thr=%g waves=%d" % (n, thr, waves))
    assert {s[0] for s in on} == {-1.0, 1.0}
    assert c_on[0] > 0 and c_off == (0, 0) and rep_on == rep_off
    if thr > 0.0:
        assert rep_on == 0


def _scale4(nt, X, n):
    X.Scale(4.0)


def _shift(nt, X, n):
    # (IncrementMatrix(Identity, X) as the solver loops make it inside their session: in place on the slab form, slab_add_diagonal;
    # the plain IncrementMatrix call merges into a NEW form instead)
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    with nt.solver_session(False):
        nt.increment_identity(I, X, 0.25)


@pytest.mark.parametrize("mutate", [_scale4, _shift], ids=["scale", "add_diagonal"])
@pytest.mark.parametrize("n,h,thr", SHAPES)
def test_in_place_changes_drop_the_maxima(nt, fma, n, h, thr, mutate):
    """the iterate is changed IN PLACE between two steps (scaled UP by 4, so that maxima kept from before would be
    underestimates and tiles with entries above the threshold would be skipped; its diagonal shifted): the following steps are
    identical with the option on and off.  The step right behind the change tests tiles: the iterate stayed in slab form (a
    packed one would start from compressed columns, without the test) and its maxima were made again"""
    h_trip, x_trip = operands(n, h)
    on, c_on, _ = run_steps(nt, n, h_trip, x_trip, thr, 6, 1, mutate_at=3, mutate=mutate)
    off, c_off, _ = run_steps(nt, n, h_trip, x_trip, thr, 6, 0, mutate_at=3, mutate=mutate)
    assert_same_run(on, off, "n=%d %s" % (n, mutate.__name__))
    assert c_on[1] > 0 and c_off == (0, 0), (c_on, c_off)
    assert on[3][4][0] > on[2][4][0], (on[2][4], on[3][4])


@pytest.mark.parametrize("n,h,thr", SHAPES)
def test_holes(nt, fma, n, h, thr):
    """X0 with 30 % of its off-diagonal entries removed: runs with holes -- the kernel zeroes the tiles of a run that nothing was
    stored in, and their maxima with them, and the next step reads those"""
    h_trip, x_trip = operands(n, h)
    x_trip = thinned(x_trip, 0.3, n + h)
    on, c_on, _ = run_steps(nt, n, h_trip, x_trip, thr, 5, 1)
    off, c_off, _ = run_steps(nt, n, h_trip, x_trip, thr, 5, 0)
    print("n=%d holes: tiles tested / skipped %r" % (n, c_on))
    assert_same_run(on, off, "n=%d holes" % n)
    assert c_on[0] > 0 and c_off == (0, 0), (c_on, c_off)


@pytest.mark.parametrize("n,h,thr", SHAPES)
def test_a_non_finite_operand(nt, fma, n, h, thr):
    """one Inf in X0: Inf * 0 in the bound is a NaN, and a NaN bound must not skip; entry for entry the same with the option on
    and off (NaN equal to NaN)"""
    h_trip, (col, row, x) = operands(n, h)
    x = x.copy()
    k = int(np.flatnonzero((col == n // 2) & (row == n // 2 + 3))[0])
    x[k] = np.inf
    on, c_on, _ = run_steps(nt, n, h_trip, (col, row, x), thr, 4, 1)
    off, c_off, _ = run_steps(nt, n, h_trip, (col, row, x), thr, 4, 0)
    print("n=%d Inf: tiles tested / skipped %r, fused steps %r" % (n, c_on, nt.fusion_counts()))
    assert_same_run(on, off, "n=%d Inf" % n, nan_ok=True)
    assert c_on[0] > 0 and c_off == (0, 0), (c_on, c_off)   # (the fused steps ran and tested tiles: "no skip" is not vacuous)
