"""GPU: complex slab sessions on more than one rank (option complex_panels; psmatrix.cpp panel_slab_multiply on the complex tile
kernel).  The sign function (SignSolversModule.F90), the inverse (InverseSolversModule.F90:29-149), the square root and the
inverse square root (SquareRootSolversModule.F90:342-531) on a complex Hermitian band keep their iterates as complex column
panels in slab form; a product exchanges the complex runs of its left operand's halo.  Ranks are processes sharing the box's
GPU over the shared-memory test transport (see test_gpu_panel_sessions.py).  Against the one-rank solve: the same iteration
counts, the same patterns, values to 1e-10 (a column's products have the same bits whoever owns it)."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "complex_panel_session_worker.py")
LOOPS = ("sign", "inv", "sqrt", "isq")


def run_world(world, tmp_path, mode="loops", extra=None):
    out = str(tmp_path / ("cps%d_%s" % (world, uuid.uuid4().hex[:6])))
    name = "c%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name,
                   NTPOLY_AMD_SHM_MB="64", NTPOLY_AMD_SPGEMM_FMA="1")
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


def cat(parts, tag):
    return tuple(np.concatenate([p[tag + s] for p in parts]) for s in ("_col", "_row", "_val"))


def assert_same(parts, reference, tags, atol):
    for tag in tags:
        got = cat(parts, tag)
        want = tuple(reference[tag + s] for s in ("_col", "_row", "_val"))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), tag
        assert np.allclose(got[2], want[2], rtol=0, atol=atol), (tag, float(np.max(np.abs(got[2] - want[2]))))
        for r, p in enumerate(parts):
            assert int(p[tag + "_iters"][0]) == int(reference[tag + "_iters"][0]), (tag, r)


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    return run_world(1, tmp_path_factory.mktemp("cpsref"))[0]


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    return run_world(2, tmp_path_factory.mktemp("cps2"))


def check_panels(parts, reference, world):
    assert_same(parts, reference, LOOPS, 1e-10)
    for r in range(world):
        for loop in LOOPS:
            slab, declined, syncs = parts[r][loop + "_panel"]
            iters = int(parts[r][loop + "_iters"][0])
            print("world", world, "rank", r, loop, "iterations", iters, "complex panel products", slab, "declined", declined,
                  "host syncs inside", syncs, "slab ops", parts[r][loop + "_slab"])
            # every product of the loop ran on the complex tile kernel with its operands in slab form, on every rank ...
            assert slab >= iters and declined <= 1, (loop, r, slab, declined, iters)
            # ... at two host round trips each (exchange layout with the plan; entry count with "every rank took its panel")
            assert syncs <= 2 * slab + 8, (loop, r, syncs, slab)
            assert np.allclose(parts[r][loop + "_norms"], reference[loop + "_norms"], rtol=1e-9, atol=1e-12), loop


def test_complex_panel_sessions_two_ranks(two_ranks, reference):
    check_panels(two_ranks, reference, 2)


def test_complex_panel_sessions_four_ranks(reference, tmp_path):
    check_panels(run_world(4, tmp_path), reference, 4)


def test_one_rank_world_is_the_complex_session(reference):
    """world 1 (no communicator): the loops run in the complex session of one rank, no panel products"""
    for loop in LOOPS:
        assert int(reference[loop + "_panel"][0]) == 0 and int(reference[loop + "_panel"][1]) == 0, loop
        assert int(reference[loop + "_slab"][0]) >= int(reference[loop + "_iters"][0]), loop


@pytest.mark.parametrize("option", ["complex_panels", "complex_sessions"])
def test_complex_panels_off_is_the_old_path(option, two_ranks, tmp_path):
    """complex_panels = 0, and complex_sessions = 0: compressed columns across ranks, no complex panel product, the same results
    as the default run"""
    parts = run_world(2, tmp_path, extra={"NTPOLY_AMD_TEST_OPTIONS": option + "=0"})
    default = dict(two_ranks[0])
    for loop in LOOPS:
        default.update(zip((loop + s for s in ("_col", "_row", "_val")), cat(two_ranks, loop)))
    assert_same(parts, default, LOOPS, 1e-10)
    for r in range(2):
        for loop in LOOPS:
            assert int(parts[r][loop + "_panel"][0]) == 0, (option, loop, r)


def test_collective_refusal_does_not_hang(tmp_path):
    """dense columns in the panel of rank 1 of two: that rank's plan does not fit the complex tile kernel, so every rank packs
    and takes compressed columns for those products -- together, the loop goes on and ends with the one-rank result"""
    ref = run_world(1, tmp_path, mode="refuse")[0]
    parts = run_world(2, tmp_path, mode="refuse")
    assert_same(parts, ref, ("inv",), 1e-10)
    for r in range(2):
        slab, declined, _ = parts[r]["inv_panel"]
        print("refusal: rank", r, "complex panel products", slab, "declined", declined)
        assert declined > 0, (r, slab, declined)
    assert parts[0]["inv_panel"][1] == parts[1]["inv_panel"][1]   # (a collective decision: counted alike)


def test_forced_rccl_single_process_takes_complex_panels(tmp_path):
    """one process, a 1-rank RCCL communicator (every collective a real RCCL call): the loops at N = 32 768 take complex panel
    products and match the one-rank session without a communicator bit for bit (the same kernel on the same plan; the
    reductions of one rank are the values themselves)"""
    res = {}
    for force in ("1", "0"):
        out = str(tmp_path / ("single%s" % force))
        env = dict(os.environ, NTPOLY_AMD_FORCE_RCCL=force, NTPOLY_AMD_PANEL_N="32768", NTPOLY_AMD_SPGEMM_FMA="1")
        env.pop("NTPOLY_AMD_COMM", None)
        r = subprocess.run([sys.executable, WORKER, out, "single"], env=env, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        res[force] = dict(np.load(out + ".0.npz"))
    for loop in LOOPS:
        slab, declined, syncs = res["1"][loop + "_panel"]
        iters = int(res["1"][loop + "_iters"][0])
        print("forced RCCL", loop, "iterations", iters, "complex panel products", slab, "declined", declined, "host syncs", syncs)
        assert slab >= iters and declined <= 1, (loop, slab, declined, iters)
        assert int(res["0"][loop + "_panel"][0]) == 0, loop
        assert iters == int(res["0"][loop + "_iters"][0]), loop
        for s in ("_col", "_row", "_val"):
            assert np.array_equal(res["1"][loop + s], res["0"][loop + s]), (loop, s)
