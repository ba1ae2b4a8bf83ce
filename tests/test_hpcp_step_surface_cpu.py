"""CPU: the surface of option hpcp_step (HPCP purification with its two traces and its update in one pass each over the slab-form
matrices of the loop) -- the option through the C ABI and host.py, its environment variable in a fresh
process, the counters and the diagnostic update entry point in the library and in include/.  No GPU: nothing here launches a
kernel."""
import re

import surface_checks as S

OPTION = "hpcp_step"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION)


def test_default_and_environment_variable_in_a_fresh_process():
    S.check_default_and_environment(OPTION, S.documented_default(OPTION))


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, ("ntpoly_amd_hpcp_step_counts", "ntpoly_amd_hpcp_update_step"))


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has solved nothing has fused nothing and refused nothing
    S.check_counters("hpcp_step", 3, ["traces", "updates", "refused"])


def test_diagnostic_update_is_exported_and_declared():
    import ntpoly_amd as nt
    assert hasattr(nt.lib, "ntpoly_amd_hpcp_update_step") and callable(nt.hpcp_update_step)
    assert "ntpoly_amd_hpcp_update_step" in nt.capi.exported_symbols()
    text = S.src("include", "ntpoly_amd.h")
    assert re.search(r"^int ntpoly_amd_hpcp_update_step\(const int\* ih_D1, const int\* ih_DDH, const int\* ih_D2DH, const double\* sigma, "
                     r"const int\* ih_WH, int\* ih_D1out, int\* ih_DHout, double\* energy\);", text, re.M)
