"""CPU: the surface of option pm_session (PM purification with its iterate kept in slab form and the stored zeros carried in a
per-panel list) -- the option through the C ABI and host.py, its environment variable in a fresh process,
the counters and the diagnostic step entry point in the library and in include/.  No GPU: nothing here launches a kernel."""
import re

import surface_checks as S

OPTION = "pm_session"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION)


def test_default_and_environment_variable_in_a_fresh_process():
    S.check_default_and_environment(OPTION, 1)


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION)


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has solved nothing has fused nothing, carried nothing and left nothing
    S.check_counters("pm_session", 4, ["sigma", "updates", "zeros", "left"])


def test_diagnostic_step_is_exported_and_declared():
    import ntpoly_amd as nt
    assert hasattr(nt.lib, "ntpoly_amd_pm_fused_step") and callable(nt.pm_fused_step)
    assert "ntpoly_amd_pm_fused_step" in nt.capi.exported_symbols()
    text = S.src("include", "ntpoly_amd.h")
    assert re.search(r"^int ntpoly_amd_pm_fused_step\(const int\* ih_X, const int\* ih_Z, const int\* ih_X2, const int\* ih_X3, ", text, re.M)
