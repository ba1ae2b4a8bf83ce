"""CPU: the surface of option stored_zero_views (read-only slab views of operands that store zeros) -- the
option through the C ABI and host.py, its environment variable in a fresh process, and the counters' entry point in the
library and in include/.  No GPU: nothing here launches a kernel."""
import ctypes as C
import re

import surface_checks as S

OPTION = "stored_zero_views"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION)


def test_default_and_environment_variable_in_a_fresh_process():
    S.check_default_and_environment(OPTION, 1)


def test_view_counters_are_exported_declared_and_read():
    import ntpoly_amd as nt
    assert hasattr(nt.lib, "ntpoly_amd_slab_view_counts")
    assert "ntpoly_amd_slab_view_counts" in nt.capi.exported_symbols()
    assert re.search(r"^void ntpoly_amd_slab_view_counts\(long long out\[4\]\);", S.src("include", "ntpoly_amd.h"), re.M), "declaration in include/ntpoly_amd.h"
    out = (C.c_longlong * 4)(-1, -1, -1, -1)
    nt.lib.ntpoly_amd_slab_view_counts(out)
    got = nt.slab_view_counts()
    assert list(got) == ["built", "products", "taken", "declined"]
    assert [got[k] for k in got] == list(out) and all(v >= 0 for v in out)
