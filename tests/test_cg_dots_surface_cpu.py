"""CPU: the surface of option cg_dots (CGSolver's traces from column dot passes) -- the option in the table,
through the C ABI and host.py, its environment variable in a fresh process, the counters and the diagnostic entry point in the
library (nm -D) and in include/.  No GPU: nothing here launches a kernel."""
import os
import re
import subprocess

import surface_checks as S

OPTION = "cg_dots"
SLOTS = ["solves", "passes", "refused", "not_formed"]


def test_option_and_counter_are_in_the_tables():
    assert [(n, e) for n, _, e in S.OPTIONS if n == OPTION] == [(OPTION, "ENV")]
    assert [(n, k) for n, k in S.COUNTERS if n == OPTION] == [(OPTION, 4)]


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION, (0, 1, 2))


def test_default_and_environment_variable_in_a_fresh_process():
    default = S.documented_default(OPTION)
    assert default in (0, 1)   # (2, the complex session, is never the default)
    S.check_default_and_environment(OPTION, default, (0, 1, 2))


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, ("ntpoly_amd_cg_dots_counts", "ntpoly_amd_cg_dots("))


def test_counters_are_exported_declared_and_zero_before_any_solve():
    import ntpoly_amd as nt
    S.check_counters(OPTION, 4, SLOTS)
    assert list(nt.host._COUNTERS[OPTION][0]) == SLOTS and len(nt.host._COUNTERS[OPTION][0]) == 4


def test_diagnostic_entry_is_exported_and_declared():
    import ntpoly_amd as nt
    assert hasattr(nt.lib, "ntpoly_amd_cg_dots") and callable(nt.cg_dots)
    assert "ntpoly_amd_cg_dots" in nt.capi.exported_symbols()
    lib = os.path.join(S.ROOT, "ntpoly_amd", "libntpoly_amd.so")
    names = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert re.search(r" T ntpoly_amd_cg_dots$", names, re.M) and re.search(r" T ntpoly_amd_cg_dots_counts$", names, re.M)
    text = S.src("include", "ntpoly_amd.h")
    assert re.search(r"^int ntpoly_amd_cg_dots\(const int\* ih_U, const int\* ih_V, double threshold, double\* diag_out, "
                     r"double\* trace_out\);", text, re.M)
