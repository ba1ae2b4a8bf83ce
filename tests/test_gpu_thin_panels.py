"""GPU: the thin-operand gather kernels inside panel products (slab sessions on more than one rank; csrc/spgemm_thin.hip through
the halo of the left operand, psmatrix.cpp panel_slab_multiply).  The kernel of a product is chosen from the entry counts of
the WHOLE operands and the global dimension, so every rank takes the same one, and the one a single rank takes: complex
products are then bit for bit the one-rank products (the gather kernels and the complex tile kernel are different
arithmetics), real ones were already (both kernels compute the same FMA chain).  Ranks are processes sharing the box's GPU
over the shared-memory test transport (see test_gpu_panel_sessions.py); every child runs under `timeout`, two at a time."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "thin_panel_worker.py")
LOOPS = ("isq_c", "isq_r")
THIN = ("real_left", "real_right", "complex_left", "complex_right", "panel_real", "panel_complex")


def run_world(world, tmp_path, mode, extra=None):
    out = str(tmp_path / ("thin%d_%s" % (world, uuid.uuid4().hex[:6])))
    name = "t%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name,
                   NTPOLY_AMD_SHM_MB="64", NTPOLY_AMD_SPGEMM_FMA="1")
        env.update(extra or {})
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, WORKER, out, mode], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
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


def cat(parts, tag):
    return tuple(np.concatenate([p[tag + s] for p in parts]) for s in ("_col", "_row", "_val"))


def thin(part, tag):
    return dict(zip(THIN, (int(x) for x in part[tag + "_thin"])))


@pytest.fixture(scope="module")
def loops_one(tmp_path_factory):
    return run_world(1, tmp_path_factory.mktemp("thin1"), "loops")[0]


@pytest.fixture(scope="module")
def loops_two(tmp_path_factory):
    return run_world(2, tmp_path_factory.mktemp("thin2"), "loops")


def test_loops_take_thin_panel_products_on_every_rank(loops_one, loops_two, tmp_path):
    """InverseSquareRoot, complex and real, n = 4096, two ranks against one: the same patterns, values to 1e-10, the same
    iteration counts; thin panel products on every rank and the same number on both (a collective decision); no more declined
    panel products than with the thin kernels off (thin_left = 0), host round trips per panel product as before."""
    off = run_world(2, tmp_path, "loops", extra={"NTPOLY_AMD_TEST_OPTIONS": "thin_left=0"})
    for loop, panel_key, sides in (("isq_c", "panel_complex", ("complex_left", "complex_right")),
                                   ("isq_r", "panel_real", ("real_left", "real_right"))):
        got = cat(loops_two, loop)
        want = tuple(loops_one[loop + s] for s in ("_col", "_row", "_val"))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), loop
        assert np.allclose(got[2], want[2], rtol=0, atol=1e-10), (loop, float(np.max(np.abs(got[2] - want[2]))))
        one = thin(loops_one, loop)
        print(loop, "one rank: iterations", int(loops_one[loop + "_iters"][0]), "thin products", one)
        assert one[panel_key] == 0 and sum(one[s] for s in sides) >= 1, one
        for r in range(2):
            t, t_off = thin(loops_two[r], loop), thin(off[r], loop)
            slab, declined, syncs = (int(x) for x in loops_two[r][loop + "_panel"])
            print(loop, "rank", r, "iterations", int(loops_two[r][loop + "_iters"][0]), "panel products", slab, "declined", declined,
                  "host syncs", syncs, "thin", t, "| thin_left = 0: declined", int(off[r][loop + "_panel"][1]), "thin", t_off)
            assert int(loops_two[r][loop + "_iters"][0]) == int(loops_one[loop + "_iters"][0]), (loop, r)
            assert t[panel_key] >= 1 and t[panel_key] == sum(t[s] for s in sides), (loop, r, t)
            assert t == thin(loops_two[0], loop), (loop, r, t)
            # (one rank and two take the same kernel for the same product)
            assert sum(t[s] for s in sides) == sum(one[s] for s in sides), (loop, t, one)
            assert sum(t_off.values()) == 0, (loop, r, t_off)
            assert declined <= int(off[r][loop + "_panel"][1]), (loop, r, declined)
            assert syncs <= 2 * slab + 8, (loop, r, syncs, slab)
        got_off = cat(off, loop)
        assert np.array_equal(got_off[0], want[0]) and np.array_equal(got_off[1], want[1]), loop + " with thin_left = 0"


def test_thin_panel_products_are_the_one_rank_products(tmp_path):
    """C = -0.5 T B and C = -0.5 B T, complex, T thin with columns of 65, 130 and 200 entries, all of them in the panel of rank 1
    of two -- the case the complex right-hand kernel takes every column for (a hand-back on one rank alone would change the
    last bits of that rank's columns): bit for bit the one-rank products, nothing hangs, nothing is declined"""
    one = run_world(1, tmp_path, "products")[0]
    two = run_world(2, tmp_path, "products")
    for tag, side in (("tb", "complex_left"), ("bt", "complex_right")):
        t1 = thin(one, tag)
        assert t1[side] == 1 and t1["panel_complex"] == 0, (tag, t1)
        got = cat(two, tag)
        want = tuple(one[tag + s] for s in ("_col", "_row", "_val"))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), tag
        assert np.array_equal(got[2].real, want[2].real) and np.array_equal(got[2].imag, want[2].imag), tag
        for r in range(2):
            t = thin(two[r], tag)
            print(tag, "rank", r, "panel", two[r][tag + "_panel"], "thin", t)
            assert t[side] == 1 and t["panel_complex"] == 1, (tag, r, t)
            assert int(two[r][tag + "_panel"][0]) == 1 and int(two[r][tag + "_panel"][1]) == 0, (tag, r)
