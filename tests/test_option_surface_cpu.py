"""CPU: the registry of engine options and counters, walked table by table -- csrc/options.inc (every option: name, default,
whether NTPOLY_AMD_<NAME> sets it) and csrc/counters.inc (every counter array the C ABI exposes as ntpoly_amd_<name>_counts).  Every
option round-trips through the C ABI and host.py, reads its default in a fresh process and follows its environment variable
there; every counter is exported, declared with its length, zero before anything ran and named slot by slot by host.py.  The
per-feature surface tests (tests/test_*_surface_cpu.py) pin their own option's default, key list and documentation as literals
with the same checks (tests/surface_checks.py) and the same three child processes.  No GPU: nothing here launches a kernel."""
import re

import pytest

import surface_checks as S

OPTIONS, COUNTERS = S.OPTIONS, S.COUNTERS


def test_every_option_is_spelled_once():
    assert len({n for n, _, _ in OPTIONS}) == len(OPTIONS) >= 52 and len(dict(COUNTERS)) == len(COUNTERS) >= 21
    for name, _, _ in OPTIONS:
        S.check_registered_once(name)


@pytest.mark.parametrize("name", [n for n, _, _ in OPTIONS])
def test_option_round_trips_through_the_c_abi_and_host(name):
    S.check_round_trip(name, (0, 1, 2))


def test_defaults_in_a_fresh_process():
    assert S.fresh()["options"] == {n: v for n, v, _ in OPTIONS}


@pytest.mark.parametrize("value", [0, 1])
def test_environment_variables_in_a_fresh_process(value):
    """every ENV option follows NTPOLY_AMD_<NAME>, every NOENV option ignores a variable of that form"""
    got = S.fresh_all(value)["options"]
    for name, default, env in OPTIONS:
        assert got[name] == (value if env == "ENV" else default), name


def test_arithmetic_selector_overrides_the_integer_option():
    """NTPOLY_AMD_ARITHMETIC = fma | unfused is applied behind the table: it wins over NTPOLY_AMD_SPGEMM_FMA"""
    assert S.fresh((("NTPOLY_AMD_ARITHMETIC", "fma"), ("NTPOLY_AMD_SPGEMM_FMA", "0")))["options"]["spgemm_fma"] == 1
    assert S.fresh((("NTPOLY_AMD_ARITHMETIC", "unfused"), ("NTPOLY_AMD_SPGEMM_FMA", "1")))["options"]["spgemm_fma"] == 0


def test_documented_defaults_are_the_tables():
    """whatever INTEGRATION.md documents as `option` (default N ... states the table's default"""
    table = {n: v for n, v, _ in OPTIONS}
    documented = [(n, int(v)) for n, v in re.findall(r"`(\w+)` \(default (-?\d+)", S.src("INTEGRATION.md")) if n in table]
    assert len(documented) >= 35
    for name, default in documented:
        assert default == table[name], name


def test_every_counter_is_exported_declared_zero_and_named_by_host():
    import ntpoly_amd as nt
    assert {n for n, _ in COUNTERS} == set(nt.host._COUNTERS)
    for name, n in COUNTERS:
        keys, doc = nt.host._COUNTERS[name][:2]
        assert n == len(keys), name
        fn = getattr(nt, name + "_counts")
        assert callable(fn) and fn.__doc__ == doc, name
        if name == "tile_skip":   # (a tuple, as ever: no keys)
            assert S.check_counters(name, n, None)["kind"] == "tuple" and isinstance(fn(), tuple)
        else:
            S.check_counters(name, n, list(keys))
    assert dict(COUNTERS)["pm_session"] == 4   # (the array's fifth slot has an entry point of its own)
