"""CPU: the surface of option scale_fold_step (ScaleAndFold with the fold update, the energy and the next step's trace in one pass
over the slab-form matrices of the loop) -- the option through the C ABI and host.py, its environment variable
in a fresh process, the counters and the two diagnostic entry points in the library and in include/, and the solver itself in
host.py's DensityMatrixSolvers.  No GPU: nothing here launches a kernel."""
import inspect
import re

import surface_checks as S

OPTION = "scale_fold_step"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION)


def test_default_and_environment_variable_in_a_fresh_process():
    S.check_default_and_environment(OPTION, S.documented_default(OPTION))


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, ("ntpoly_amd_scale_fold_step_counts", "ntpoly_amd_scale_fold_update_step", "ntpoly_amd_scale_fold_dot_trace"))


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has solved nothing has fused nothing and refused nothing
    S.check_counters("scale_fold_step", 3, ["updates", "dot_traces", "refused"])


def test_diagnostics_are_exported_and_declared():
    import ntpoly_amd as nt
    text = S.src("include", "ntpoly_amd.h")
    assert hasattr(nt.lib, "ntpoly_amd_scale_fold_update_step") and callable(nt.scale_fold_update_step)
    assert "ntpoly_amd_scale_fold_update_step" in nt.capi.exported_symbols()
    assert re.search(r"^int ntpoly_amd_scale_fold_update_step\(const int\* ih_X, const int\* ih_X2, const double\* a, const double\* b, "
                     r"const int\* ih_WH, int\* ih_Xout, double\* dot, double\* trace\);", text, re.M)
    assert hasattr(nt.lib, "ntpoly_amd_scale_fold_dot_trace") and callable(nt.scale_fold_dot_trace)
    assert "ntpoly_amd_scale_fold_dot_trace" in nt.capi.exported_symbols()
    assert re.search(r"^int ntpoly_amd_scale_fold_dot_trace\(const int\* ih_X, const int\* ih_WH, double\* dot, double\* trace\);", text, re.M)


def test_host_mirrors_the_reference_class_surface():
    """DensityMatrixSolvers.ScaleAndFold, its arguments in the order of the reference's C++ declaration (the energy, an output
    reference there, is the return value here)"""
    import ntpoly_amd as nt
    fn = nt.DensityMatrixSolvers.ScaleAndFold
    assert callable(fn)
    assert list(inspect.signature(fn).parameters) == ["H", "ISQ", "trace", "Density", "homo", "lumo", "solver_parameters"]
    assert hasattr(nt.lib, "ScaleAndFold_wrp")
