"""CPU: the surface of option complex_sum_chain (the complex side of the scaled sum chains -- level 1: the inverse-root iteration in a
complex slab session; level 2: the chains of complex Sine / Cosine, Paterson-Stockmeyer, the factorized Chebyshev evaluation and the
inverse-root iteration in one pass each) -- the option through the C ABI and host.py, its environment variable
in a fresh process, its documentation and the counters in the library and in include/.  The diagnostic entry point is sum_chain's
own, whose signature tests/test_sum_chain_surface_cpu.py pins.  No GPU: nothing here launches a kernel."""
import surface_checks as S

OPTION = "complex_sum_chain"


def test_option_round_trips_through_the_c_abi_and_host():
    S.check_round_trip(OPTION, values=(0, 1, 2))


def test_default_and_environment_variable_in_a_fresh_process():
    assert S.documented_default(OPTION) == 0
    S.check_default_and_environment(OPTION, 0, values=(0, 1))
    assert S.fresh((("NTPOLY_AMD_COMPLEX_SUM_CHAIN", "2"),))["options"][OPTION] == 2
    assert S.fresh((("NTPOLY_AMD_COMPLEX_SUM_CHAIN", "2"),))["options"]["sum_chain"] == S.fresh()["options"]["sum_chain"]   # (independent)


def test_option_is_documented_where_a_caller_looks():
    S.check_documented(OPTION, ("ntpoly_amd_complex_sum_chain_counts", "ntpoly_amd_sum_chain"))
    for name in ("DESIGN.md", "README.md", "profiles/README.md"):
        assert "complex_sum_chain" in S.src(*name.split("/")), name


def test_counters_are_exported_declared_and_zero_before_any_solve():
    # a process that has solved nothing has opened no session, fused nothing and refused nothing
    S.check_counters("complex_sum_chain", 3, ["sessions", "passes", "refused"])
    import ntpoly_amd as nt
    assert list(nt.complex_sum_chain_counts()) == ["sessions", "passes", "refused"]
