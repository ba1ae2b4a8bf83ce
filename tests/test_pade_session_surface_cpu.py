"""CPU: the surface of option pade_session (ComputeExponentialPade in a slab session, each of its two groups of merges in one pass;
DESIGN.md section 3) -- the option through the C ABI and host.py, its environment variable in a fresh process, the counters and the
diagnostic entry point in the library and in include/, and the solver itself in host.py's ExponentialSolvers.
No GPU: nothing here launches a kernel."""
import inspect
import re

import surface_checks as S

OPTION = "pade_session"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION, values=(0, 1, 2))


def test_default_and_environment_variable_in_a_fresh_process():
    S.check_default_and_environment(OPTION, S.documented_default(OPTION), values=(0, 1, 2))


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, ("ntpoly_amd_pade_session_counts", "ntpoly_amd_pade_chain_step"))


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has solved nothing has fused nothing and refused nothing
    S.check_counters("pade_session", 4, ["solves", "sum_passes", "pair_passes", "refused"])


def test_diagnostic_is_exported_and_declared():
    import ntpoly_amd as nt
    text = S.src("include", "ntpoly_amd.h")
    assert hasattr(nt.lib, "ntpoly_amd_pade_chain_step") and callable(nt.pade_chain_step)
    assert "ntpoly_amd_pade_chain_step" in nt.capi.exported_symbols()
    assert re.search(r"^int ntpoly_amd_pade_chain_step\(const int\* ih_Base, const int\* ih_A1, const int\* ih_A2, const int\* ih_A3, "
                     r"const int\* n_addends, const double\* scales, const double\* coeffs, int\* ih_Out1, int\* ih_Out2\);", text, re.M)
    assert list(inspect.signature(nt.pade_chain_step).parameters) == ["Base", "addends", "scales", "coeffs", "Out1", "Out2"]


def test_host_mirrors_the_reference_class_surface():
    """ExponentialSolvers.ComputeExponentialPade, its arguments in the order of the reference's C++ declaration"""
    import ntpoly_amd as nt
    f = nt.ExponentialSolvers.ComputeExponentialPade
    assert callable(f)
    assert list(inspect.signature(f).parameters) == ["InputMat", "OutputMat", "solver_parameters"]
    assert hasattr(nt.lib, "ComputeExponentialPade_wrp")
