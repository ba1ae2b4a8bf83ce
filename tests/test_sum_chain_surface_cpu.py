"""CPU: the surface of option sum_chain (the scaled sum chains of Sine / Cosine, Paterson-Stockmeyer, the factorized Chebyshev
evaluation and the inverse-root iteration in one pass each) -- the option through the C ABI and host.py, its
environment variable in a fresh process, the counters and the diagnostic entry point in the library and in include/.
No GPU: nothing here launches a kernel."""
import inspect
import re

import surface_checks as S

OPTION = "sum_chain"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION, values=(0, 1))


def test_default_and_environment_variable_in_a_fresh_process():
    S.check_default_and_environment(OPTION, S.documented_default(OPTION), values=(0, 1))


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, ("ntpoly_amd_sum_chain_counts", "ntpoly_amd_sum_chain"))


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has evaluated nothing has fused nothing and refused nothing
    S.check_counters("sum_chain", 2, ["passes", "refused"])


def test_diagnostic_is_exported_and_declared():
    import ntpoly_amd as nt
    text = S.src("include", "ntpoly_amd.h")
    assert hasattr(nt.lib, "ntpoly_amd_sum_chain") and callable(nt.sum_chain)
    assert "ntpoly_amd_sum_chain" in nt.capi.exported_symbols()
    assert re.search(r"^int ntpoly_amd_sum_chain\(const int\* ih_Base, const double\* s, const int\* n_addends, const int\* const\* ih_addends, "
                     r"const double\* coeffs, const double\* post, int\* ih_Out\);", text, re.M)
    assert list(inspect.signature(nt.sum_chain).parameters) == ["Base", "s", "addends", "coeffs", "post", "Out"]
