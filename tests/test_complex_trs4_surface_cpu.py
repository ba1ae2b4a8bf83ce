"""CPU: the surface of option complex_trs4 (the complex TRS4 loop in a complex slab session: traces, operand and energy from one
pass each over the loop's slab-form matrices) -- the option through the C ABI and host.py, its environment
variable in a fresh process, the counters and the two diagnostic entry points in the library and in include/.  No GPU: nothing
here launches a kernel."""
import re

import surface_checks as S

OPTION = "complex_trs4"
ENTRY_POINTS = ("ntpoly_amd_complex_trs4_counts", "ntpoly_amd_trs4_chain_step", "ntpoly_amd_trs4_energy")


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION)


def test_default_and_environment_variable_in_a_fresh_process():
    S.check_default_and_environment(OPTION, S.documented_default(OPTION))


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, ENTRY_POINTS)


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has solved nothing has fused nothing and refused nothing
    S.check_counters("complex_trs4", 4, ["traces", "operands", "energies", "refused"])


def test_diagnostics_are_exported_and_declared():
    import ntpoly_amd as nt
    text = S.src("include", "ntpoly_amd.h")
    assert hasattr(nt.lib, "ntpoly_amd_trs4_chain_step") and callable(nt.trs4_chain_step)
    assert "ntpoly_amd_trs4_chain_step" in nt.capi.exported_symbols()
    assert re.search(r"^int ntpoly_amd_trs4_chain_step\(const int\* ih_X, const int\* ih_X2, const double\* sigma, int\* ih_P, "
                     r"double\* trace_fx, double\* trace_gx\);", text, re.M)
    assert hasattr(nt.lib, "ntpoly_amd_trs4_energy") and callable(nt.trs4_energy)
    assert "ntpoly_amd_trs4_energy" in nt.capi.exported_symbols()
    assert re.search(r"^int ntpoly_amd_trs4_energy\(const int\* ih_X, const int\* ih_WH, double\* energy\);", text, re.M)
