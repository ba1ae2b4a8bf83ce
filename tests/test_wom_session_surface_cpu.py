"""CPU: the surface of option wom_session (WOM_GC / WOM_C in a slab session, the tail of a Heun trial and the canonical step's two
dots in one pass each) -- the option through the C ABI and host.py, its environment variable in a fresh
process, the counters and the two diagnostic entry points in the library and in include/, and the solvers themselves in host.py's
FermiOperator.  No GPU: nothing here launches a kernel."""
import inspect
import re

import surface_checks as S

OPTION = "wom_session"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION, values=(0, 1, 2))


def test_default_and_environment_variable_in_a_fresh_process():
    S.check_default_and_environment(OPTION, S.documented_default(OPTION), values=(0, 1, 2))


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, ("ntpoly_amd_wom_session_counts", "ntpoly_amd_wom_heun_step", "ntpoly_amd_wom_c_dots"))


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has solved nothing has fused nothing and refused nothing
    S.check_counters("wom_session", 4, ["solves", "heun_passes", "c_dot_passes", "refused"])


def test_diagnostics_are_exported_and_declared():
    import ntpoly_amd as nt
    text = S.src("include", "ntpoly_amd.h")
    assert hasattr(nt.lib, "ntpoly_amd_wom_heun_step") and callable(nt.wom_heun_step)
    assert "ntpoly_amd_wom_heun_step" in nt.capi.exported_symbols()
    assert re.search(r"^int ntpoly_amd_wom_heun_step\(const int\* ih_W, const int\* ih_K0, const int\* ih_K1, const int\* ih_RK1, "
                     r"const double\* step, const double\* threshold, int\* ih_RK2out, double\* err, double\* err2\);", text, re.M)
    assert list(inspect.signature(nt.wom_heun_step).parameters) == ["W", "K0", "K1", "RK1", "step", "threshold", "RK2out"]
    assert hasattr(nt.lib, "ntpoly_amd_wom_c_dots") and callable(nt.wom_c_dots)
    assert "ntpoly_amd_wom_c_dots" in nt.capi.exported_symbols()
    assert re.search(r"^int ntpoly_amd_wom_c_dots\(const int\* ih_X, const int\* ih_W, const int\* ih_XA, double out\[2\]\);", text, re.M)
    assert list(inspect.signature(nt.wom_c_dots).parameters) == ["X", "W", "XA"]


def test_host_mirrors_the_reference_class_surface():
    """FermiOperator.WOM_GC / WOM_C, their arguments in the order of the reference's C++ declaration (the energy, an output reference
    there, is the return value here)"""
    import ntpoly_amd as nt
    gc, c = nt.FermiOperator.WOM_GC, nt.FermiOperator.WOM_C
    assert callable(gc) and callable(c)
    assert list(inspect.signature(gc).parameters) == ["H", "ISQ", "Density", "chemical_potential", "inv_temp", "solver_parameters"]
    assert list(inspect.signature(c).parameters) == ["H", "ISQ", "Density", "trace", "inv_temp", "solver_parameters"]
    assert hasattr(nt.lib, "WOM_GC_wrp") and hasattr(nt.lib, "WOM_C_wrp")
