"""Complex TRS2 with the iterate kept in complex slab form (option complex_density, psmatrix.cpp complex_trs2_step): X*X on
the complex tile kernel, the update 2X - X*X by the complex merge of the slab algebra, the energy Re sum conj(X) D and the trace in
one pass (slab_extra.hip k_sa_dot_trace_c).  Against the same solve with the option off (the compressed-column path), against the
oracle's complex TRS2, against the real solve where every imaginary part is zero, and against the properties of a density
matrix.  A complex lattice keeps its iterate in complex block form instead.  Outside the option's conditions (unfused
arithmetic, complex_tile = 0, real operands, no block path for an operand without runs) nothing changes."""
import numpy as np
import pytest

from gen import banded_triplets, lattice_triplets

pytestmark = pytest.mark.gpu
N, H, THR = 8000, 40, 1e-8


@pytest.fixture(scope="module")
def nt():
    import ntpoly_amd as nt
    nt.init_comm()
    nt.ConstructGlobalProcessGrid(1, 1, 1)
    return nt


@pytest.fixture()
def fma(nt):
    from oracle import oracle_py as O
    keep = {k: nt.get_option(k) for k in ("spgemm_fma", "complex_tile", "complex_density", "complex_sessions")}
    nt.set_option("spgemm_fma", 1)
    nt.set_option("complex_tile", 1)
    nt.set_option("complex_sessions", 1)
    O.set_fma(True)
    yield O
    for k, v in keep.items():
        nt.set_option(k, v)
    O.set_fma(False)


def hermitian(trip, phase=0.1):
    """a Hermitian complex operand with the pattern and |values| of a real symmetric one: H(r, c) = v exp(i phase (r - c))"""
    c, r, v = trip
    return c, r, v * np.exp(1j * phase * (r.astype(np.float64) - c.astype(np.float64)))


def srt(t):
    c, r, v = (np.asarray(x) for x in t)
    o = np.lexsort((r, c))
    return c[o], r[o], v[o]


def close(got, want, n, thr, what, rel=1e-12):
    import scipy.sparse as sp
    G = sp.csr_matrix((got[2], (got[1] - 1, got[0] - 1)), shape=(n, n))
    W = sp.csr_matrix((want[2], (want[1] - 1, want[0] - 1)), shape=(n, n))
    scale = max(1.0, np.abs(want[2]).max())
    D = (G - W).tocoo()
    bad = np.abs(D.data) > rel * scale
    # entries present on one side only must sit at the threshold
    assert np.all(np.abs(D.data[bad]) <= thr * (1 + 1e-9) + rel * scale), "%s: max |d| = %g" % (what, np.abs(D.data).max())
    assert abs(G.nnz - W.nnz) <= max(8, 1e-5 * W.nnz), "%s: %d vs %d entries" % (what, G.nnz, W.nnz)


def params(nt, max_it=100, diff=1e-10):
    p = nt.SolverParameters()
    p.SetThreshold(THR)
    p.SetConvergeDiff(diff)
    p.SetMaxIterations(max_it)
    return p


def trs2(nt, n, trip, opt, **kw):
    nt.set_option("complex_density", opt)
    Hm = nt.Matrix_ps.from_triplets(n, *trip)
    I = nt.Matrix_ps(n)
    I.FillIdentity()
    K = nt.Matrix_ps(n)
    c0 = nt.complex_fusion_counts()
    energy, mu = nt.DensityMatrixSolvers.TRS2(Hm, I, n / 2.0, K, params(nt, **kw))
    c1 = nt.complex_fusion_counts()
    tr = nt.solver_trace()
    d = {k: c1[k] - c0[k] for k in c1}
    return dict(K=srt(K.triplets()), energy=energy, mu=mu, it=tr["iterations"], sigma=list(tr["sigma"]), e=np.asarray(tr["energy"]),
                counts=d)


@pytest.fixture(scope="module")
def banded(nt):
    return banded_triplets(N, H, complex_=True)


@pytest.fixture(scope="module")
def banded_runs(nt, banded):
    """the banded complex TRS2 with the option on and off (computed once for the module)"""
    import ntpoly_amd as ntm
    keep = {k: ntm.get_option(k) for k in ("spgemm_fma", "complex_tile", "complex_density", "complex_sessions")}
    ntm.set_option("spgemm_fma", 1)
    ntm.set_option("complex_tile", 1)
    ntm.set_option("complex_sessions", 1)
    try:
        on = trs2(ntm, N, banded, 1)
        off = trs2(ntm, N, banded, 0)
    finally:
        for k, v in keep.items():
            ntm.set_option(k, v)
    return on, off


def test_trs2_banded_on_vs_off(nt, fma, banded_runs):
    on, off = banded_runs
    assert on["it"] == off["it"] and on["sigma"] == off["sigma"]
    assert np.allclose(on["e"], off["e"], rtol=1e-11, atol=0.0)
    assert abs(on["energy"] - off["energy"]) <= 1e-11 * abs(off["energy"])
    close(on["K"], off["K"], N, THR, "density on vs off")
    # every step after the first ran in complex slab form; with the option off none did
    assert on["counts"]["square"] + on["counts"]["update"] >= on["it"] - 1
    assert on["counts"]["repeated"] == 0
    assert off["counts"] == dict(square=0, update=0, repeated=0)


def test_trs2_banded_vs_oracle(nt, fma, banded, banded_runs):
    O = fma
    on, _ = banded_runs
    Ho = O.Mat.from_triplets(N, N, *banded)
    Ko, e_o, mu_o, tro = O.density("trs2", Ho, O.Mat.identity(N), N / 2.0,
                                   O.params(converge_diff=1e-10, max_iterations=100, threshold=THR))
    assert on["it"] == len(tro["sigma"])
    # (the last step's sigma is the sign of trace(X) - nel once trace(X) has converged to nel: rounding decides it)
    assert list(on["sigma"])[:-1] == list(tro["sigma"])[:-1]
    assert abs(on["mu"] - mu_o) <= 1e-9
    assert abs(on["energy"] - e_o) <= 1e-11 * abs(e_o)
    # (the densities are not compared: the last step's sigma is rounding's choice, and X*X and 2X - X*X of a converged X keep
    # different entries at the threshold; test_trs2_banded_on_vs_off compares them with the compressed-column path)


def test_trs2_density_properties(nt, fma, banded_runs):
    """independent of any implementation: K is Hermitian, trace(K) = nel, K is idempotent to the convergence tolerance"""
    import scipy.sparse as sp
    on, _ = banded_runs
    c, r, v = on["K"]
    K = sp.csr_matrix((v, (r - 1, c - 1)), shape=(N, N))
    scale = np.abs(v).max()
    assert abs(K - K.conj().T).max() <= 1e-12 * max(1.0, scale)
    assert abs(K.diagonal().real.sum() - N / 2.0) <= 1e-8 * N
    assert np.abs(K.diagonal().imag).max() <= 1e-12
    R = K @ K - K
    assert (abs(R).max() if R.nnz else 0.0) <= 1e-6


def test_trs2_zero_imaginary_parts(nt, fma):
    """a real H stored as complex: the real solve's iterations and energies; every imaginary part of K exactly zero"""
    n, h = 4000, 30
    c, r, v = banded_triplets(n, h)
    cplx = trs2(nt, n, (c, r, v.astype(np.complex128)), 1)
    real = trs2(nt, n, (c, r, v), 1)
    assert cplx["it"] == real["it"] and cplx["sigma"] == real["sigma"]
    assert np.allclose(cplx["e"], real["e"], rtol=1e-11, atol=0.0)
    assert np.all(np.imag(cplx["K"][2]) == 0.0)
    assert cplx["counts"]["square"] + cplx["counts"]["update"] >= cplx["it"] - 1
    assert real["counts"] == dict(square=0, update=0, repeated=0)   # (real operands never count)


@pytest.mark.parametrize("which", ["spgemm_fma", "complex_tile"])
def test_outside_the_gates_bit_for_bit(nt, fma, which):
    """unfused arithmetic or complex_tile = 0: the option changes nothing, bit for bit"""
    n, h = 3000, 24
    trip = banded_triplets(n, h, complex_=True)
    nt.set_option(which, 0)
    a = trs2(nt, n, trip, 1, max_it=30)
    b = trs2(nt, n, trip, 0, max_it=30)
    assert a["counts"] == dict(square=0, update=0, repeated=0)
    assert a["it"] == b["it"] and a["sigma"] == b["sigma"] and list(a["e"]) == list(b["e"])
    for x, y in zip(a["K"], b["K"]):
        assert np.array_equal(x, y)


def test_trs2_lattice_in_block_form(nt, fma):
    """a complex operand without runs (a Hermitian 20^3 lattice, block_path = 2): every step after the first in complex block
    form (the complex tile products of the block path, the complex block merge, block_dot_trace), agreeing with option 0"""
    L = 20
    n = L ** 3
    trip = hermitian(lattice_triplets(L))
    keep = {k: nt.get_option(k) for k in ("block_path", "block_complex")}
    nt.set_option("block_path", 2)
    nt.set_option("block_complex", 1)
    try:
        a = trs2(nt, n, trip, 1, max_it=12, diff=1e-30)
        b = trs2(nt, n, trip, 0, max_it=12, diff=1e-30)
    finally:
        for k, v in keep.items():
            nt.set_option(k, v)
    assert a["counts"]["square"] + a["counts"]["update"] >= a["it"] - 1
    assert a["counts"]["repeated"] == 0
    assert b["counts"] == dict(square=0, update=0, repeated=0)
    assert a["it"] == b["it"] and a["sigma"] == b["sigma"]
    assert np.allclose(a["e"], b["e"], rtol=1e-11, atol=0.0)
    close(a["K"], b["K"], n, THR, "lattice density on vs off")


def test_lattice_outside_the_block_path_keeps_its_path(nt, fma):
    """block_path = 0: a complex lattice has neither runs nor block form -- declined once, solved as before, bit for bit"""
    L = 16
    n = L ** 3
    trip = hermitian(lattice_triplets(L))
    keep = nt.get_option("block_path")
    nt.set_option("block_path", 0)
    try:
        a = trs2(nt, n, trip, 1, max_it=12, diff=1e-30)
        b = trs2(nt, n, trip, 0, max_it=12, diff=1e-30)
    finally:
        nt.set_option("block_path", keep)
    assert a["counts"] == dict(square=0, update=0, repeated=0)
    assert a["it"] == b["it"] and list(a["e"]) == list(b["e"])
    for x, y in zip(a["K"], b["K"]):
        assert np.array_equal(x, y)
