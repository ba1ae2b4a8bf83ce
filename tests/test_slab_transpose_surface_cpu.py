"""CPU: the surface of option slab_transpose (the transpose of a slab form and PolarDecomposition in a slab session; DESIGN.md
section 3) -- the option through the C ABI and host.py, its environment variable in a fresh process, the counters and the
diagnostic entry point in the library and in include/.  No GPU: nothing here launches a kernel."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION = "slab_transpose"
ENV = "NTPOLY_AMD_SLAB_TRANSPOSE"


def _fresh(code, **env):
    base = {k: v for k, v in os.environ.items() if k != ENV}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(base, PYTHONPATH=ROOT, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    return r.stdout.strip().splitlines()[-1]


def _documented_default():
    """the default INTEGRATION.md states for the option: `slab_transpose` (default N; ..."""
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
        for v in (0, 1, 2):
            lib.ntpoly_amd_set_option(OPTION.encode(), C.byref(C.c_int(v)))
            assert int(lib.ntpoly_amd_get_option(OPTION.encode())) == v == nt.get_option(OPTION)
        for v in (2, 1, 0):
            nt.set_option(OPTION, v)
            assert int(lib.ntpoly_amd_get_option(OPTION.encode())) == v
    finally:
        nt.set_option(OPTION, before)
    assert nt.get_option(OPTION) == before


def test_default_and_environment_variable_in_a_fresh_process():
    code = "import ntpoly_amd as nt; print(nt.get_option('%s'))" % OPTION
    assert _fresh(code) == _documented_default()
    for v in ("0", "1", "2"):
        assert _fresh(code, **{ENV: v}) == v


def test_option_is_documented_where_a_caller_looks():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`%s`" % OPTION in text and "`%s`" % ENV in text
    assert "ntpoly_amd_slab_transpose_counts" in text and "ntpoly_amd_slab_transpose(" in text
    wrp = open(os.path.join(ROOT, "ntpoly_amd", "csrc", "wrp.cpp")).read()
    assert wrp.count('"%s"' % OPTION) == 2   # (set_option and get_option)


def test_counters_are_exported_declared_and_zero_before_any_solve():
    import ntpoly_amd as nt
    assert hasattr(nt.lib, "ntpoly_amd_slab_transpose_counts")
    assert "ntpoly_amd_slab_transpose_counts" in nt.capi.exported_symbols()
    text = open(os.path.join(ROOT, "include", "ntpoly_amd.h")).read()
    assert re.search(r"^void ntpoly_amd_slab_transpose_counts\(long long out\[4\]\);", text, re.M), "declaration in include/ntpoly_amd.h"
    # a process that has transposed nothing has counted nothing
    code = ("import ctypes as C, ntpoly_amd as nt\n"
            "out = (C.c_longlong * 4)(-1, -1, -1, -1)\n"
            "nt.lib.ntpoly_amd_slab_transpose_counts(out)\n"
            "got = nt.slab_transpose_counts()\n"
            "assert list(got) == ['transposes', 'conjugates', 'refused', 'polar_sessions'], got\n"
            "assert [got[k] for k in got] == list(out)\n"
            "print(' '.join(str(v) for v in out))\n")
    assert _fresh(code) == "0 0 0 0"


def test_diagnostic_entry_is_exported_and_declared():
    import ntpoly_amd as nt
    assert hasattr(nt.lib, "ntpoly_amd_slab_transpose") and callable(nt.slab_transpose)
    assert "ntpoly_amd_slab_transpose" in nt.capi.exported_symbols()
    text = open(os.path.join(ROOT, "include", "ntpoly_amd.h")).read()
    assert re.search(r"^int ntpoly_amd_slab_transpose\(const int\* ih_A, int\* ih_AT, const int\* conjugate\);", text, re.M)
