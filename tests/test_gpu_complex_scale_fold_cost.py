"""GPU: what the complex ScaleAndFold passes cost the host (option complex_scale_fold; csrc/slab_extra.hip slab_saf_update_c and
slab_dot_trace_c behind engine.hpp ps_saf_update_step / ps_saf_dot_trace_step).  tests/test_gpu_fused_pass_cost.py pins the real
passes: a repeated fold update makes 2 waits of the host (the pass's one read-back of counts, slots, status and sums, and the
packing of the output for the caller), the scale branch's pass 1.  The complex fold update shares that scaffold (FreshSlabs) and
may cost no more; the complex scale-branch pass is one launch and one read-back.

As there, each diagnostic runs twice on the same matrices inside one session: the first call brings the operands into slab form,
the second is bracketed with exchange_stats()[2], which counts every wait of the host in the process.  The numbers are counts, so
there is no margin."""
import numpy as np
import pytest

from gen import banded_triplets

pytestmark = pytest.mark.gpu
N = 259   # (not a multiple of the 4 waves of a workgroup)
H = 6     # half-width of the band
OPTIONS = ("spgemm_fma", "slab_algebra", "complex_tile", "complex_sessions", "complex_scale_fold", "scale_fold_step")
REAL_UPDATE_WAITS = 2   # tests/test_gpu_fused_pass_cost.py WAITS["scale_fold_update"]
DOT_TRACE_WAITS = 1     # one pass, one read-back


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture()
def passes_on(nt):
    keep = {k: nt.get_option(k) for k in OPTIONS}
    for k in OPTIONS:
        nt.set_option(k, 1)
    yield
    for k, v in keep.items():
        nt.set_option(k, v)


def _operands(nt, cplx, count):
    """banded matrices of one kind that differ in their diagonals"""
    return [nt.Matrix_ps.from_triplets(N, *banded_triplets(N, H, complex_=cplx, shift=0.125 * k)) for k in range(count)]


def _books(nt):
    c = nt.slab_algebra_counts()
    return np.array([c[k] for k in sorted(c)])


def _twice(nt, call, outs):
    """the second call's host waits, and that it is the first call again: scalars, outputs, books"""
    read = lambda: [tuple(np.array(x) for x in m.triplets()) for m in outs]
    with nt.solver_session():
        c0 = _books(nt)
        first = call()
        c1 = _books(nt)
        first_outs = read()
        c2 = _books(nt)
        w0 = nt.exchange_stats()[2]
        second = call()
        waits = nt.exchange_stats()[2] - w0
        c3 = _books(nt)
        second_outs = read()
    assert first is not None, "the pass was gated or refused"
    assert second == first   # (the same scalars, bit for bit)
    for a, b in zip(first_outs, second_outs):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a[2]) > 0
    assert np.array_equal(c3 - c2, c1 - c0), "the books of the second call differ from the first's"
    return waits


def test_a_repeated_complex_fold_update_waits_no_more_than_the_real_one(nt, passes_on):
    waits = {}
    for cplx in (False, True):
        X, X2, WH = _operands(nt, cplx, 3)
        O = nt.Matrix_ps(N)
        c0, r0 = nt.complex_scale_fold_counts(), nt.scale_fold_step_counts()
        waits[cplx] = _twice(nt, lambda: nt.scale_fold_update_step(X, X2, -0.25, 1.5, WH, O), [O])
        c1, r1 = nt.complex_scale_fold_counts(), nt.scale_fold_step_counts()
        assert O.IsComplex() == cplx
        assert (c1["updates"] - c0["updates"], r1["updates"] - r0["updates"]) == ((2, 0) if cplx else (0, 2))
    print("host waits of the second fold update: real %d, complex %d" % (waits[False], waits[True]))
    assert waits[False] == REAL_UPDATE_WAITS
    assert waits[True] <= waits[False]


def test_the_complex_scale_branch_pass_waits_once(nt, passes_on):
    X, WH = _operands(nt, True, 2)
    c0 = nt.complex_scale_fold_counts()
    waits = _twice(nt, lambda: nt.scale_fold_dot_trace(X, WH), [])
    c1 = nt.complex_scale_fold_counts()
    print("host waits of the second dot-and-trace pass, complex: %d" % waits)
    assert c1["dot_traces"] - c0["dot_traces"] == 2 and c1["refused"] == c0["refused"]
    assert waits == DOT_TRACE_WAITS
