"""CPU: the surface of option purify_session (PurificationExtrapolate in a slab session, everything behind an iteration's two products
in one pass) -- the option through the C ABI and host.py, its environment variable in a fresh process, the
counters and the diagnostic entry point in the library and in include/, and the solver itself in host.py's GeometryOptimization.
No GPU: nothing here launches a kernel."""
import inspect
import re

import surface_checks as S

OPTION = "purify_session"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION, values=(0, 1, 2))


def test_default_and_environment_variable_in_a_fresh_process():
    S.check_default_and_environment(OPTION, S.documented_default(OPTION), values=(0, 1, 2))


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, ("ntpoly_amd_purify_session_counts", "ntpoly_amd_purify_tail_step"))


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has solved nothing has fused nothing and refused nothing
    S.check_counters("purify_session", 4, ["solves", "fold_passes", "plain_passes", "refused"])


def test_diagnostic_is_exported_and_declared():
    import ntpoly_amd as nt
    text = S.src("include", "ntpoly_amd.h")
    assert hasattr(nt.lib, "ntpoly_amd_purify_tail_step") and callable(nt.purify_tail_step)
    assert "ntpoly_amd_purify_tail_step" in nt.capi.exported_symbols()
    assert re.search(r"^int ntpoly_amd_purify_tail_step\(const int\* ih_D, const int\* ih_N, const int\* ih_S, const int\* fold, "
                     r"int\* ih_Nout, double\* norm, double\* next_trace\);", text, re.M)
    assert list(inspect.signature(nt.purify_tail_step).parameters) == ["D", "N", "S", "fold", "Nout"]


def test_host_mirrors_the_reference_class_surface():
    """GeometryOptimization.PurificationExtrapolate, its arguments in the order of the reference's C++ declaration"""
    import ntpoly_amd as nt
    f = nt.GeometryOptimization.PurificationExtrapolate
    assert callable(f)
    assert list(inspect.signature(f).parameters) == ["PreviousDensity", "Overlap", "trace", "NewDensity", "solver_parameters"]
    assert hasattr(nt.lib, "PurificationExtrapolate_wrp")
