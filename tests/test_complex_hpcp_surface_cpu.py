"""CPU: the surface of option complex_hpcp (the complex HPCP loop in a complex slab session: the two traces in one pass, the update,
the energy and the next DH in another) -- the option through the C ABI and host.py, its environment variable
in a fresh process, the counters and the diagnostic entry point in the library and in include/.  No GPU: nothing here launches a
kernel."""
import re

import surface_checks as S

OPTION = "complex_hpcp"
ENTRY_POINTS = ("ntpoly_amd_complex_hpcp_counts", "ntpoly_amd_hpcp_traces_step")


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION)


def test_default_and_environment_variable_in_a_fresh_process():
    assert S.documented_default(OPTION) == 0
    S.check_default_and_environment(OPTION, 0)


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, ENTRY_POINTS)


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has solved nothing has fused nothing and refused nothing
    S.check_counters("complex_hpcp", 3, ["traces", "updates", "refused"])


def test_diagnostic_is_exported_and_declared():
    import ntpoly_amd as nt
    text = S.src("include", "ntpoly_amd.h")
    assert hasattr(nt.lib, "ntpoly_amd_hpcp_traces_step") and callable(nt.hpcp_traces_step)
    assert "ntpoly_amd_hpcp_traces_step" in nt.capi.exported_symbols()
    assert re.search(r"^int ntpoly_amd_hpcp_traces_step\(const int\* ih_DDH, const int\* ih_D2DH, double out\[2\]\);", text, re.M)
