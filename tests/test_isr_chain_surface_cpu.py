"""CPU: the surface of option isr_chain (the polynomial chain of the Taylor square-root step in one pass over the slab-form
iterate and its square) -- the option through the C ABI and host.py, its environment variable in a fresh
process, the counters and the diagnostic step entry point in the library and in include/.  No GPU: nothing here launches a
kernel."""
import re

import surface_checks as S

OPTION = "isr_chain"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION)


def test_default_and_environment_variable_in_a_fresh_process():
    S.check_default_and_environment(OPTION, S.documented_default(OPTION))


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, ("ntpoly_amd_isr_chain_counts", "ntpoly_amd_isr_chain_step"))


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has solved nothing has fused nothing and refused nothing
    S.check_counters("isr_chain", 3, ["order5", "order3", "refused"])


def test_diagnostic_step_is_exported_and_declared():
    import ntpoly_amd as nt
    assert hasattr(nt.lib, "ntpoly_amd_isr_chain_step") and callable(nt.isr_chain_step)
    assert "ntpoly_amd_isr_chain_step" in nt.capi.exported_symbols()
    text = S.src("include", "ntpoly_amd.h")
    assert re.search(r"^int ntpoly_amd_isr_chain_step\(const int\* ih_X, const int\* ih_X2, const int\* order, const double\* a, "
                     r"const double\* b, const double\* c, int\* ih_Out1, int\* ih_Out2\);", text, re.M)
