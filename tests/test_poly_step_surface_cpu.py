"""CPU: the surface of option poly_step (the real Chebyshev / Hermite step in one pass, ComputeExponential's squarings in a slab
session) -- the option through the C ABI and host.py, its environment variable in a fresh process, the
counters and the diagnostic entry point in the library and in include/.
No GPU: nothing here launches a kernel."""
import inspect
import re

import surface_checks as S

OPTION = "poly_step"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION, values=(0, 1, 2))


def test_default_and_environment_variable_in_a_fresh_process():
    S.check_default_and_environment(OPTION, S.documented_default(OPTION), values=(0, 1, 2))


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, ("ntpoly_amd_poly_step_counts", "ntpoly_amd_poly_step"))


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has evaluated nothing has fused nothing and refused nothing
    S.check_counters("poly_step", 3, ["exp_sessions", "steps", "refused"])


def test_diagnostic_is_exported_and_declared():
    import ntpoly_amd as nt
    text = S.src("include", "ntpoly_amd.h")
    assert hasattr(nt.lib, "ntpoly_amd_poly_step") and callable(nt.poly_step)
    assert "ntpoly_amd_poly_step" in nt.capi.exported_symbols()
    assert re.search(r"^int ntpoly_amd_poly_step\(const int\* ih_P, const int\* ih_Tkm2, const int\* ih_R, const double\* a, "
                     r"const double\* c, int\* ih_TkOut, int\* ih_ROut\);", text, re.M)
    assert list(inspect.signature(nt.poly_step).parameters) == ["P", "Tkm2", "R", "a", "c", "TkOut", "ROut"]
