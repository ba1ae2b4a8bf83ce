"""CPU: the surface of option slab_transpose (the transpose of a slab form and PolarDecomposition in a slab session; DESIGN.md
section 3) -- the option through the C ABI and host.py, its environment variable in a fresh process, the counters and the
diagnostic entry point in the library and in include/.  No GPU: nothing here launches a kernel."""
import re

import surface_checks as S

OPTION = "slab_transpose"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION, (0, 1, 2))


def test_default_and_environment_variable_in_a_fresh_process():
    S.check_default_and_environment(OPTION, S.documented_default(OPTION), (0, 1, 2))


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, ("ntpoly_amd_slab_transpose_counts", "ntpoly_amd_slab_transpose("))


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has transposed nothing has counted nothing
    S.check_counters("slab_transpose", 4, ["transposes", "conjugates", "refused", "polar_sessions"])


def test_diagnostic_entry_is_exported_and_declared():
    import ntpoly_amd as nt
    assert hasattr(nt.lib, "ntpoly_amd_slab_transpose") and callable(nt.slab_transpose)
    assert "ntpoly_amd_slab_transpose" in nt.capi.exported_symbols()
    text = S.src("include", "ntpoly_amd.h")
    assert re.search(r"^int ntpoly_amd_slab_transpose\(const int\* ih_A, int\* ih_AT, const int\* conjugate\);", text, re.M)
