"""CPU: the surface of option power_vector (PowerBounds on one vector) -- the option through the C ABI and
host.py, its environment variable in a fresh process, the counters and the diagnostic entry point in the library and in
include/.  No GPU: nothing here launches a kernel."""
import re

import surface_checks as S

OPTION = "power_vector"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION, (0, 1))


def test_default_and_environment_variable_in_a_fresh_process():
    S.check_default_and_environment(OPTION, S.documented_default(OPTION), (0, 1))


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, ("ntpoly_amd_power_vector_counts", "ntpoly_amd_power_vector_step("))


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has bounded nothing has counted nothing
    S.check_counters("power_vector", 3, ["solves", "steps", "refused"])


def test_diagnostic_entry_is_exported_and_declared():
    import ntpoly_amd as nt
    assert hasattr(nt.lib, "ntpoly_amd_power_vector_step") and callable(nt.power_vector_step)
    assert "ntpoly_amd_power_vector_step" in nt.capi.exported_symbols()
    text = S.src("include", "ntpoly_amd.h")
    assert re.search(r"^int ntpoly_amd_power_vector_step\(const int\* ih_A, const double\* x, double\* y, const double\* threshold, "
                     r"double out\[3\]\);", text, re.M)
