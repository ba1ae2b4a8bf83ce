"""CPU: the surface of option ghash_mfma_complex (complex products of the grouped LDS-hash kernel on the FP64 matrix cores, table
class 0) -- the option through the C ABI and host.py, its environment variable in a fresh process, the
per-path group counters and the cache drop, in the library and in include/.  No GPU: nothing here launches a kernel."""
import re

import surface_checks as S

OPTION = "ghash_mfma_complex"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION)


def test_default_and_environment_variable_in_a_fresh_process():
    S.check_default_and_environment(OPTION, 1)


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION)


def test_class_counters_are_exported_declared_and_zero_before_any_product():
    # a process that has multiplied nothing has finished no group on any path
    S.check_counters("ghash_class", 4, ["real_mfma", "real_vector", "complex_mfma", "complex_vector"])


def test_cache_drop_is_exported_declared_and_callable_without_a_gpu():
    import ntpoly_amd as nt
    assert "ntpoly_amd_drop_grouped_caches" in nt.capi.exported_symbols()
    text = S.src("include", "ntpoly_amd.h")
    assert re.search(r"^void ntpoly_amd_drop_grouped_caches\(\);", text, re.M), "declaration in include/ntpoly_amd.h"
    before = dict(nt.ghash_class_counts())
    nt.drop_grouped_caches()
    nt.drop_grouped_caches()   # (nothing kept: still nothing to forget)
    assert dict(nt.ghash_class_counts()) == before   # the counters are cumulative: a drop does not reset them
