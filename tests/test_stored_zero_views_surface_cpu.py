"""CPU: the surface of option stored_zero_views (read-only slab views of operands that store zeros) -- the
option through the C ABI and host.py, its environment variable in a fresh process, and the counters' entry point in the
library and in include/.  No GPU: nothing here launches a kernel."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION = "stored_zero_views"


def _fresh(code, **env):
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    return r.stdout.strip().splitlines()[-1]


def test_option_round_trips_through_the_c_abi_and_host():
    import ntpoly_amd as nt
    lib = nt.lib
    lib.ntpoly_amd_get_option.restype = C.c_int
    before = nt.get_option(OPTION)
    try:
        for v in (0, 1):
            lib.ntpoly_amd_set_option(OPTION.encode(), C.byref(C.c_int(v)))
            assert int(lib.ntpoly_amd_get_option(OPTION.encode())) == v == nt.get_option(OPTION)
        nt.set_option(OPTION, 0)
        assert int(lib.ntpoly_amd_get_option(OPTION.encode())) == 0
    finally:
        nt.set_option(OPTION, before)
    assert nt.get_option(OPTION) == before


def test_default_and_environment_variable_in_a_fresh_process():
    code = "import ntpoly_amd as nt; print(nt.get_option('%s'))" % OPTION
    env = {k: v for k, v in os.environ.items() if k != "NTPOLY_AMD_STORED_ZERO_VIEWS"}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, PYTHONPATH=ROOT), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "1", r.stdout
    assert _fresh(code, NTPOLY_AMD_STORED_ZERO_VIEWS="0") == "0"
    assert _fresh(code, NTPOLY_AMD_STORED_ZERO_VIEWS="1") == "1"


def test_view_counters_are_exported_declared_and_read():
    import ntpoly_amd as nt
    assert hasattr(nt.lib, "ntpoly_amd_slab_view_counts")
    assert "ntpoly_amd_slab_view_counts" in nt.capi.exported_symbols()
    text = open(os.path.join(ROOT, "include", "ntpoly_amd.h")).read()
    assert re.search(r"^void ntpoly_amd_slab_view_counts\(long long out\[4\]\);", text, re.M), "declaration in include/ntpoly_amd.h"
    out = (C.c_longlong * 4)(-1, -1, -1, -1)
    nt.lib.ntpoly_amd_slab_view_counts(out)
    got = nt.slab_view_counts()
    assert list(got) == ["built", "products", "taken", "declined"]
    assert [got[k] for k in got] == list(out) and all(v >= 0 for v in out)
