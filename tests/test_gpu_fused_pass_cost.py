"""GPU: what a fused slab pass costs the host (csrc/slab_extra.hip, the launchers of the TRS4, inverse-square-root, HPCP and
ScaleAndFold passes; engine.hpp ps_*_step).  Every pass that writes a fresh slab-form output reads its entry count, its slot count,
its status and its sums back in ONE wait of the host, and a traces-style pass reads its two sums in one: the other tests pin what
the passes compute, this one pins that the scaffold they share adds no wait, and that a pass repeated on the same operands is the
same pass -- the same scalars, the same outputs, the same books.

Each diagnostic runs twice on the same matrices inside one session.  The first call brings the operands into slab form; the second
is bracketed with exchange_stats()[2], which counts every wait of the host in the process.  The expected numbers are counts, so
there is no margin."""
import numpy as np
import pytest

from gen import banded_triplets

pytestmark = pytest.mark.gpu
N = 259   # (not a multiple of the 4 waves of a workgroup)
H = 6     # half-width of the band
OPTIONS = ("spgemm_fma", "slab_algebra", "complex_tile", "complex_sessions", "complex_trs4", "complex_hpcp", "hpcp_step", "isr_chain",
           "scale_fold_step")

# Host waits of the second call.  Not derived: measured once, with this file, on the commit before the launchers were folded onto
# one output builder (the last one that spelled the scaffold out in every launcher), and written down here.  They read as one wait
# per pass (a TRS4 chain step is two passes: the traces, the operand) and one per output packed for the caller.
WAITS = {
    "trs4_real": 3,
    "trs4_complex": 3,
    "isr_order5": 3,
    "isr_order3": 2,
    "hpcp_traces": 1,
    "hpcp_update_real": 3,
    "hpcp_update_complex": 3,
    "scale_fold_update": 2,
    "scale_fold_dot_trace": 1,
}


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


def _trs4(cplx):
    def make(nt):
        X, X2 = _operands(nt, cplx, 2)
        P = nt.Matrix_ps(N)
        return lambda: nt.trs4_chain_step(X, X2, 0.5, P), [P]
    return make


def _isr(order):
    def make(nt):
        X, X2 = _operands(nt, False, 2)
        O1, O2 = nt.Matrix_ps(N), nt.Matrix_ps(N)
        return lambda: nt.isr_chain_step(X, X2, order, 0.75, 0.625, 0.375, O1, O2), [O1, O2] if order == 5 else [O1]
    return make


def _hpcp_traces(nt):
    DDH, D2DH = _operands(nt, False, 2)
    return lambda: nt.hpcp_traces_step(DDH, D2DH), []


def _hpcp_update(cplx):
    def make(nt):
        D1, DDH, D2DH, WH = _operands(nt, cplx, 4)
        O, Hn = nt.Matrix_ps(N), nt.Matrix_ps(N)
        return lambda: nt.hpcp_update_step(D1, DDH, D2DH, 0.5, WH, O, Hn), [O, Hn]
    return make


def _saf_update(nt):
    X, X2, WH = _operands(nt, False, 3)
    O = nt.Matrix_ps(N)
    return lambda: nt.scale_fold_update_step(X, X2, -0.25, 1.5, WH, O), [O]


def _saf_dot_trace(nt):
    X, WH = _operands(nt, False, 2)
    return lambda: nt.scale_fold_dot_trace(X, WH), []


PASSES = {
    "trs4_real": _trs4(False),
    "trs4_complex": _trs4(True),
    "isr_order5": _isr(5),
    "isr_order3": _isr(3),
    "hpcp_traces": _hpcp_traces,
    "hpcp_update_real": _hpcp_update(False),
    "hpcp_update_complex": _hpcp_update(True),
    "scale_fold_update": _saf_update,
    "scale_fold_dot_trace": _saf_dot_trace,
}


def _books(nt):
    c = nt.slab_algebra_counts()
    return np.array([c[k] for k in sorted(c)])


def _read(outs):
    return [tuple(np.array(x) for x in m.triplets()) for m in outs]


@pytest.mark.parametrize("name", list(PASSES))
def test_second_call_costs_the_recorded_waits(nt, passes_on, name):
    call, outs = PASSES[name](nt)
    with nt.solver_session():
        c0 = _books(nt)
        first = call()
        c1 = _books(nt)
        first_outs = _read(outs)
        c2 = _books(nt)
        w0 = nt.exchange_stats()[2]
        second = call()
        waits = nt.exchange_stats()[2] - w0
        c3 = _books(nt)
        second_outs = _read(outs)
    print("host waits of the second call, %s: %d" % (name, waits))
    assert first is not None, "the pass was gated or refused"
    assert second == first   # (the same scalars, bit for bit)
    assert len(second_outs) == len(first_outs)
    for a, b in zip(first_outs, second_outs):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert len(a[2]) > 0
    assert np.array_equal(c3 - c2, c1 - c0), "the books of the second call differ from the first's"
    assert waits == WAITS[name]
