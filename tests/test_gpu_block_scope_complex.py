"""GPU: complex operands without runs on several ranks, solved in the pattern's BLOCK order (csrc/band_scope.cpp, option
block_scope_complex; the panel products on the complex tile products of the block path, psmatrix.cpp multiply_panel ->
k_bs_numeric_c).  A complex Hermitian 20^3 lattice (no runs, no band) on 2 and 4 ranks: SignFunction, Invert and
InverseSquareRoot each run as one block-order solve on every rank, every panel product on the block path.  Ranks are processes
sharing the box's GPU over the shared-memory test transport (see test_gpu_panel_sessions_complex.py).

Against the one-rank solve on the caller's labels, the contract of the real lattice in test_gpu_multirank_big.py: the solve
in a block order is the reference's solve under its load balancer with that permutation -- the same iteration counts, entry
counts of every iterate and of the result within 1e-4 nnz + 8, values through sums within rtol 1e-8 / atol 1e-7."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "block_scope_complex_worker.py")
SOLVES = ("sign", "inv", "isq")


def run_world(world, tmp_path, mode="solves", extra=None):
    out = str(tmp_path / ("bsc%d_%s" % (world, uuid.uuid4().hex[:6])))
    name = "b%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name,
                   NTPOLY_AMD_SHM_MB="128", NTPOLY_AMD_SPGEMM_FMA="1")
        env.pop("NTPOLY_AMD_BLOCK_SCOPE_COMPLEX", None)
        env.update(extra or {})
        procs.append(subprocess.Popen([sys.executable, WORKER, out, mode], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      text=True))
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=600)
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


def total(parts, key):
    return np.sum(np.stack([p[key] for p in parts]), axis=0)


def assert_like_one_rank(parts, ref, tag):
    """the contract of a solve in a block order against the one-rank solve on the caller's labels"""
    for r, p in enumerate(parts):
        assert int(p[tag + "_iters"][0]) == int(ref[tag + "_iters"][0]), (tag, r, p[tag + "_iters"], ref[tag + "_iters"])
        assert np.allclose(p[tag + "_glob"], ref[tag + "_glob"], rtol=1e-8, atol=1e-7), (tag, r, p[tag + "_glob"], ref[tag + "_glob"])
    nnz_it, want_it = total(parts, tag + "_iter_nnz"), ref[tag + "_iter_nnz"]
    assert np.all(np.abs(nnz_it - want_it) <= 1e-4 * want_it + 8), (tag, nnz_it, want_it)
    nnz, want = int(total(parts, tag + "_nnz")[0]), int(ref[tag + "_nnz"][0])
    assert abs(nnz - want) <= 1e-4 * want + 8, (tag, nnz, want)
    assert np.allclose(total(parts, tag + "_sums"), ref[tag + "_sums"], rtol=1e-8, atol=1e-7), (tag, total(parts, tag + "_sums"), ref[tag + "_sums"])


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    return run_world(1, tmp_path_factory.mktemp("bscref"))[0]


@pytest.mark.parametrize("world", [2, 4])
def test_complex_lattice_solves_in_block_order(world, reference, tmp_path):
    parts = run_world(world, tmp_path)
    for tag in SOLVES:
        for r in range(world):
            solves, products = parts[r][tag + "_block_scope"]
            iters = int(parts[r][tag + "_iters"][0])
            print("world", world, "rank", r, tag, "iterations", iters, "block scope solves", solves, "block path products", products)
            # one solve in the block order, every panel product of it on the block path (at least one per iteration)
            assert solves == 1 and products >= iters, (tag, r, solves, products, iters)
            assert parts[r][tag + "_band_scope"][0] == 0, (tag, r)
        assert_like_one_rank(parts, reference, tag)


def test_one_rank_takes_no_scope(reference):
    """world 1 (no communicator): the complex session of one rank, no scope"""
    for tag in SOLVES:
        assert reference[tag + "_block_scope"].tolist() == [0, 0], tag


def test_complex_trs2_in_block_order(tmp_path):
    """a density solver wrapped by the scope (TRS2, the real identity as ISQ beside the complex H) on 2 ranks: one block-order
    solve, its products on the block path, the one-rank result under the same contract (sigma sequence equal, energies to 1e-8)"""
    ref = run_world(1, tmp_path, mode="trs2")[0]
    parts = run_world(2, tmp_path, mode="trs2")
    assert ref["trs2_block_scope"].tolist() == [0, 0]
    for r in range(2):
        solves, products = parts[r]["trs2_block_scope"]
        assert solves == 1 and products >= 6, (r, solves, products)
        assert np.array_equal(parts[r]["trs2_sigma"], ref["trs2_sigma"]), r
        assert np.allclose(parts[r]["trs2_energy"], ref["trs2_energy"], rtol=1e-8, atol=1e-7), (r, parts[r]["trs2_energy"], ref["trs2_energy"])
        assert np.allclose(parts[r]["trs2_scal"], ref["trs2_scal"], rtol=1e-8, atol=1e-7), (r, parts[r]["trs2_scal"], ref["trs2_scal"])
    assert_like_one_rank(parts, ref, "trs2")


def test_option_off_is_the_old_path(tmp_path):
    """block_scope_complex = 0 (set in the process, and through the environment in a fresh one): no block scope, the complex
    products go to the LDS hash as before -- the two runs give the same results"""
    extra = {"NTPOLY_AMD_BSC_SOLVES": "inv"}
    a = run_world(2, tmp_path, extra=dict(extra, NTPOLY_AMD_TEST_OPTIONS="block_scope_complex=0"))
    b = run_world(2, tmp_path, extra=dict(extra, NTPOLY_AMD_BLOCK_SCOPE_COMPLEX="0"))
    for r in range(2):
        for parts in (a, b):
            assert parts[r]["inv_block_scope"].tolist() == [0, 0], r
        assert int(a[r]["inv_iters"][0]) == int(b[r]["inv_iters"][0]), r
        assert np.array_equal(a[r]["inv_col"], b[r]["inv_col"]) and np.array_equal(a[r]["inv_row"], b[r]["inv_row"]), r
        assert np.allclose(a[r]["inv_val"], b[r]["inv_val"], rtol=0, atol=1e-12), r


def test_complex_band_keeps_the_band_scope(tmp_path):
    """a complex band under a random relabelling: the band search recovers it, the solve runs in the band scope, not the block
    scope"""
    parts = run_world(2, tmp_path, mode="band")
    for r in range(2):
        assert parts[r]["band_band_scope"][0] == 1, r
        assert parts[r]["band_block_scope"].tolist() == [0, 0], r


def test_complex_order_is_the_order_of_the_moduli(tmp_path):
    """the block order of a complex pattern is made from the moduli: a complex lattice and the real matrix with its pattern and
    |values| get the same positions and super-blocks, each in a fresh cache; asked again, the complex one finds it kept"""
    res = run_world(1, tmp_path, mode="order")[0]
    for tag in ("complex", "real", "again"):
        assert res["order_%s_ok" % tag][0] == 1, tag
    assert np.array_equal(res["order_complex_pos"], res["order_real_pos"])
    assert np.array_equal(res["order_again_pos"], res["order_real_pos"])
    assert res["order_complex_ns"][0] == res["order_real_ns"][0] == res["order_again_ns"][0]
