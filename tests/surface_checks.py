"""Shared by the CPU surface tests (tests/test_*_surface_cpu.py, tests/test_option_surface_cpu.py): the two registry tables as the
sources spell them, ONE fresh child process per environment for the whole session (every test reads the same report), and the
checks that every feature's surface test makes of its option and its counters.  Not a test module: nothing here is collected."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def src(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# [(name, default, "ENV" | "NOENV")] of csrc/options.inc and [(name, N)] of csrc/counters.inc
OPTIONS = [(n, int(v), e) for n, v, e in re.findall(r"^NTP_OPTION\((\w+), (-?\d+), (ENV|NOENV)\)", src("ntpoly_amd", "csrc", "options.inc"), re.M)]
COUNTERS = [(n, int(k)) for n, k in re.findall(r"^NTP_COUNTER\((\w+), (\d+), \w+\)", src("ntpoly_amd", "csrc", "counters.inc"), re.M)]


def env_name(option):
    return "NTPOLY_AMD_" + option.upper()


# what a fresh process reports: every option through host.py, every counter raw (out pre-filled with -1) and through host.py
_CHILD = """
import ctypes as C, json, ntpoly_amd as nt
options = {n: nt.get_option(n) for n in %r}
counters = {}
for name, n in %r:
    out = (C.c_longlong * n)(*([-1] * n))
    getattr(nt.lib, "ntpoly_amd_%%s_counts" %% name)(out)
    got = getattr(nt, name + "_counts")()
    counters[name] = dict(raw=list(out), kind=type(got).__name__, keys=list(got) if isinstance(got, dict) else None,
                          values=list(got.values()) if isinstance(got, dict) else list(got))
print(json.dumps(dict(options=options, counters=counters)))
""" % ([n for n, _, _ in OPTIONS], COUNTERS)


@functools.lru_cache(maxsize=None)
def fresh(env_items=()):
    """the report of a child in whose environment no option variable (nor NTPOLY_AMD_ARITHMETIC) is set but the given ones"""
    drop = {env_name(n) for n, _, _ in OPTIONS} | {"NTPOLY_AMD_ARITHMETIC"}
    base = {k: v for k, v in os.environ.items() if k not in drop}
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env=dict(base, PYTHONPATH=ROOT, **dict(env_items)), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    return json.loads(r.stdout.strip().splitlines()[-1])


def fresh_all(value):
    """... with the variable of EVERY option's name set to value (an option without a variable must ignore it)"""
    return fresh(tuple((env_name(n), str(value)) for n, _, _ in OPTIONS))


def documented_default(option):
    """the default INTEGRATION.md states for the option: `option` (default N; `NTPOLY_AMD_OPTION`)"""
    m = re.search(r"`%s` \(default (-?\d+); `%s`\)" % (option, env_name(option)), src("INTEGRATION.md"))
    assert m, "INTEGRATION.md names the option, its default and its environment variable"
    return int(m.group(1))


def check_round_trip(option, values=(0, 1)):
    """through the C ABI and through host.py, both directions, the value found restored"""
    import ntpoly_amd as nt
    lib = nt.lib
    lib.ntpoly_amd_get_option.restype = C.c_int
    before = nt.get_option(option)
    try:
        for v in values:
            lib.ntpoly_amd_set_option(option.encode(), C.byref(C.c_int(v)))
            assert int(lib.ntpoly_amd_get_option(option.encode())) == v == nt.get_option(option)
        for v in reversed(values):
            nt.set_option(option, v)
            assert int(lib.ntpoly_amd_get_option(option.encode())) == v
    finally:
        nt.set_option(option, before)
    assert nt.get_option(option) == before


def check_default_and_environment(option, default, values=(0, 1)):
    """in fresh processes: the default without the variable, the variable's value with it"""
    assert fresh()["options"][option] == default
    for v in values:
        assert fresh_all(v)["options"][option] == v


def check_documented(option, entry_points=()):
    text = src("INTEGRATION.md")
    assert "`%s`" % option in text and "`%s`" % env_name(option) in text
    for name in entry_points:
        assert name in text, name
    check_registered_once(option)


def check_registered_once(option):
    """one entry of the option table is the whole registration (set, get and environment walk that table: the round trip and the
    fresh-process checks prove it): no second entry, no branch on the name in the C ABI"""
    assert len(re.findall(r"^NTP_OPTION\(%s," % option, src("ntpoly_amd", "csrc", "options.inc"), re.M)) == 1
    assert '"%s"' % option not in src("ntpoly_amd", "csrc", "wrp.cpp")


def check_counters(name, n, keys):
    """exported, declared as out[n], and in a process that has done nothing: every slot 0 (after a pre-fill with -1), host.py's
    dict under these keys in this order with the raw call's values.  Returns the fresh report of the counter"""
    import ntpoly_amd as nt
    symbol = "ntpoly_amd_%s_counts" % name
    assert hasattr(nt.lib, symbol)
    assert symbol in nt.capi.exported_symbols()
    assert re.search(r"^void %s\(long long out\[%d\]\);" % (symbol, n), src("include", "ntpoly_amd.h"), re.M), "declaration in include/ntpoly_amd.h"
    got = fresh()["counters"][name]
    assert got["keys"] == keys, got
    assert got["values"] == got["raw"] == [0] * n
    return got
