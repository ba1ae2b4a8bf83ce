"""GPU, two ranks sharing the GPU over the shared-memory test transport: a complex input with STORED ZEROS enters a panel
session as a read-only view (option stored_zero_views; psmatrix.cpp panel_slab_multiply: a rank whose panel is a view reports
"in slab form", the halo carries the runs as they are) -- Chebyshev of degree 8 on the generator's band (n = 2048, h = 24,
zeros at (500, 500) and (1500, 1500): one in each rank's panel) equals the one-rank result bit for bit."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "stored_zero_view_panel_worker.py")


def run_world(world, tmp_path):
    out = str(tmp_path / ("szv%d_%s" % (world, uuid.uuid4().hex[:6])))
    name = "q%s" % uuid.uuid4().hex[:12]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", NTPOLY_AMD_COMM="shm:" + name, NTPOLY_AMD_SHM_MB="64")
        procs.append(subprocess.Popen([sys.executable, WORKER, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=180)   # (one small evaluation and the start of a process: seconds)
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


def test_two_ranks_with_view_panels_equal_one_rank_bit_for_bit(tmp_path):
    one = run_world(1, tmp_path)[0]
    two = run_world(2, tmp_path)
    got = tuple(np.concatenate([p[s] for p in two]) for s in ("col", "row", "val"))
    assert len(got[2]) == len(one["val"]) and np.array_equal(got[0], one["col"]) and np.array_equal(got[1], one["row"]), "pattern"
    assert np.array_equal(got[2].real, one["val"].real) and np.array_equal(got[2].imag, one["val"].imag), "values"
    print("one rank: views", one["view"], "slab", one["slab"], "panel", one["panel"])
    assert one["view"][0] >= 1 and one["view"][1] >= 7 and one["panel"][0] == 0, (one["view"], one["panel"])
    for r, p in enumerate(two):
        print("rank", r, "views (built, products, taken, declined)", p["view"], "slab", p["slab"], "panel (slab, declined)", p["panel"])
        assert int(p["stored_zeros"]) == 1, (r, p["stored_zeros"])       # (each panel holds one of the two stored zeros)
        assert p["view"][0] >= 1 and p["view"][1] >= 7, (r, p["view"])   # built, products
        assert p["panel"][0] >= 7 and p["panel"][1] == 0, (r, p["panel"])
        # the caller's panel reads back with its stored zero
        assert len(p["in_val"]) == len(p["want_in_val"]) and np.array_equal(p["in_val"], p["want_in_val"]), r
