"""CPU: the surface of option ghash_mfma_complex (complex products of the grouped LDS-hash kernel on the FP64 matrix cores, table
class 0) -- the option through the C ABI and host.py, its environment variable in a fresh process, the
per-path group counters and the cache drop, in the library and in include/.  No GPU: nothing here launches a kernel."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION = "ghash_mfma_complex"
ENV = "NTPOLY_AMD_GHASH_MFMA_COMPLEX"
DEFAULT = "1"


def _fresh(code, **env):
    base = {k: v for k, v in os.environ.items() if k != ENV}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(base, PYTHONPATH=ROOT, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    return r.stdout.strip().splitlines()[-1]


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
    assert _fresh(code) == DEFAULT
    assert _fresh(code, **{ENV: "0"}) == "0"
    assert _fresh(code, **{ENV: "1"}) == "1"


def test_option_is_documented_where_a_caller_looks():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`%s`" % OPTION in text and "`%s`" % ENV in text
    wrp = open(os.path.join(ROOT, "ntpoly_amd", "csrc", "wrp.cpp")).read()
    assert wrp.count('"%s"' % OPTION) == 2   # (set_option and get_option)


def test_class_counters_are_exported_declared_and_zero_before_any_product():
    import ntpoly_amd as nt
    assert hasattr(nt.lib, "ntpoly_amd_ghash_class_counts")
    assert "ntpoly_amd_ghash_class_counts" in nt.capi.exported_symbols()
    text = open(os.path.join(ROOT, "include", "ntpoly_amd.h")).read()
    assert re.search(r"^void ntpoly_amd_ghash_class_counts\(long long out\[4\]\);", text, re.M), "declaration in include/ntpoly_amd.h"
    # a process that has multiplied nothing has finished no group on any path
    code = ("import ctypes as C, ntpoly_amd as nt\n"
            "out = (C.c_longlong * 4)(-1, -1, -1, -1)\n"
            "nt.lib.ntpoly_amd_ghash_class_counts(out)\n"
            "got = nt.ghash_class_counts()\n"
            "assert list(got) == ['real_mfma', 'real_vector', 'complex_mfma', 'complex_vector'], got\n"
            "assert [got[k] for k in got] == list(out)\n"
            "print(' '.join(str(v) for v in out))\n")
    assert _fresh(code) == "0 0 0 0"


def test_cache_drop_is_exported_declared_and_callable_without_a_gpu():
    import ntpoly_amd as nt
    assert "ntpoly_amd_drop_grouped_caches" in nt.capi.exported_symbols()
    text = open(os.path.join(ROOT, "include", "ntpoly_amd.h")).read()
    assert re.search(r"^void ntpoly_amd_drop_grouped_caches\(\);", text, re.M), "declaration in include/ntpoly_amd.h"
    before = dict(nt.ghash_class_counts())
    nt.drop_grouped_caches()
    nt.drop_grouped_caches()   # (nothing kept: still nothing to forget)
    assert dict(nt.ghash_class_counts()) == before   # the counters are cumulative: a drop does not reset them
