"""CPU: the surface of option complex_scale_fold (the complex ScaleAndFold loop in a complex slab session: the fold update, the
energy and the next trace in one pass, the scale branch's energy and trace in one) -- the option through the C
ABI and host.py, its environment variable in a fresh process, the counters in the library and in include/, the two diagnostics'
signatures as they were.  No GPU: nothing here launches a kernel."""
import re

import surface_checks as S

OPTION = "complex_scale_fold"
COUNTS = "ntpoly_amd_complex_scale_fold_counts"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION)


def test_default_and_environment_variable_in_a_fresh_process():
    assert S.documented_default(OPTION) == 0
    S.check_default_and_environment(OPTION, 0)


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, (COUNTS,))


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has solved nothing has fused nothing and refused nothing
    S.check_counters("complex_scale_fold", 3, ["updates", "dot_traces", "refused"])


def test_the_diagnostics_keep_their_signatures():
    """complex operands come through the entry points the real loop has: nothing about them changes in the header"""
    text = S.src("include", "ntpoly_amd.h")
    assert re.search(r"^int ntpoly_amd_scale_fold_update_step\(const int\* ih_X, const int\* ih_X2, const double\* a, const double\* b, "
                     r"const int\* ih_WH, int\* ih_Xout, double\* dot, double\* trace\);", text, re.M)
    assert re.search(r"^int ntpoly_amd_scale_fold_dot_trace\(const int\* ih_X, const int\* ih_WH, double\* dot, double\* trace\);", text, re.M)
