"""CPU: the surface of option complex_pm (the complex PM loop in a complex slab session: sigma's trace and dot in one pass, the
scaling and both merges in another, stored (0, 0) entries carried in a row list) -- the option through the C
ABI and host.py, its environment variable in a fresh process, the counters in the library and in include/, the diagnostic's
signature as it was.  No GPU: nothing here launches a kernel."""
import re

import surface_checks as S

OPTION = "complex_pm"
COUNTS = "ntpoly_amd_complex_pm_counts"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION)


def test_default_and_environment_variable_in_a_fresh_process():
    assert S.documented_default(OPTION) == 0
    S.check_default_and_environment(OPTION, 0)


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, (COUNTS,))


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has solved nothing has fused nothing and left nothing; the real loop's books are a different array
    got = S.check_counters("complex_pm", 4, ["sigma", "updates", "zeros", "left"])
    assert S.fresh()["counters"]["pm_session"]["keys"] == got["keys"]


def test_the_diagnostic_keeps_its_signature():
    """complex operands come through the entry point the real loop has: nothing about it changes in the header"""
    text = S.src("include", "ntpoly_amd.h")
    assert re.search(r"^int ntpoly_amd_pm_fused_step\(const int\* ih_X, const int\* ih_Z, const int\* ih_X2, const int\* ih_X3, "
                     r"const double\* a1, const double\* a2, const double\* a3, const double\* thr, int\* ih_Out, int\* ih_Zout, "
                     r"double\* sc\);", text, re.M)
