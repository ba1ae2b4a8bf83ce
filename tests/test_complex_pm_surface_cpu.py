"""CPU: the surface of option complex_pm (the complex PM loop in a complex slab session: sigma's trace and dot in one pass, the
scaling and both merges in another, stored (0, 0) entries carried in a row list) -- the option through the C
ABI and host.py, its environment variable in a fresh process, the counters in the library and in include/, the diagnostic's
signature as it was.  No GPU: nothing here launches a kernel."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION = "complex_pm"
ENV = "NTPOLY_AMD_COMPLEX_PM"
COUNTS = "ntpoly_amd_complex_pm_counts"


def _fresh(code, **env):
    base = {k: v for k, v in os.environ.items() if k != ENV}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(base, PYTHONPATH=ROOT, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    return r.stdout.strip().splitlines()[-1]


def _documented_default():
    """the default INTEGRATION.md states for the option: `complex_pm` (default N; ..."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"`%s` \(default (\d+); `%s`\)" % (OPTION, ENV), text)
    assert m, "INTEGRATION.md names the option, its default and its environment variable"
    return m.group(1)


def test_option_round_trips_through_the_c_abi_and_host():
    import ntpoly_amd as nt
    lib = nt.lib
    lib.ntpoly_amd_get_option.restype = C.c_int
    before = nt.get_option(OPTION)
    try:
        for v in (0, 1):
            lib.ntpoly_amd_set_option(OPTION.encode(), C.byref(C.c_int(v)))
            assert int(lib.ntpoly_amd_get_option(OPTION.encode())) == v == nt.get_option(OPTION)
        nt.set_option(OPTION, 0)
        assert int(lib.ntpoly_amd_get_option(OPTION.encode())) == 0
    finally:
        nt.set_option(OPTION, before)
    assert nt.get_option(OPTION) == before


def test_default_and_environment_variable_in_a_fresh_process():
    code = "import ntpoly_amd as nt; print(nt.get_option('%s'))" % OPTION
    assert _documented_default() == "0"
    assert _fresh(code) == _documented_default()
    assert _fresh(code, **{ENV: "0"}) == "0"
    assert _fresh(code, **{ENV: "1"}) == "1"


def test_option_is_documented_where_a_caller_looks():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`%s`" % OPTION in text and "`%s`" % ENV in text
    assert COUNTS in text
    wrp = open(os.path.join(ROOT, "ntpoly_amd", "csrc", "wrp.cpp")).read()
    assert wrp.count('"%s"' % OPTION) == 2   # (set_option and get_option)


def test_counters_are_exported_declared_and_zero_before_any_solve():
    import ntpoly_amd as nt
    assert hasattr(nt.lib, COUNTS)
    assert COUNTS in nt.capi.exported_symbols()
    text = open(os.path.join(ROOT, "include", "ntpoly_amd.h")).read()
    assert re.search(r"^void ntpoly_amd_complex_pm_counts\(long long out\[4\]\);", text, re.M), "declaration in include/ntpoly_amd.h"
    # a process that has solved nothing has fused nothing and left nothing; the real loop's books are a different array
    code = ("import ctypes as C, ntpoly_amd as nt\n"
            "out = (C.c_longlong * 4)(-1, -1, -1, -1)\n"
            "nt.lib.ntpoly_amd_complex_pm_counts(out)\n"
            "got = nt.complex_pm_counts()\n"
            "assert list(got) == ['sigma', 'updates', 'zeros', 'left'], got\n"
            "assert [got[k] for k in got] == list(out)\n"
            "assert list(nt.pm_session_counts()) == list(got)\n"
            "print(' '.join(str(v) for v in out))\n")
    assert _fresh(code) == "0 0 0 0"


def test_the_diagnostic_keeps_its_signature():
    """complex operands come through the entry point the real loop has: nothing about it changes in the header"""
    text = open(os.path.join(ROOT, "include", "ntpoly_amd.h")).read()
    assert re.search(r"^int ntpoly_amd_pm_fused_step\(const int\* ih_X, const int\* ih_Z, const int\* ih_X2, const int\* ih_X3, "
                     r"const double\* a1, const double\* a2, const double\* a3, const double\* thr, int\* ih_Out, int\* ih_Zout, "
                     r"double\* sc\);", text, re.M)
