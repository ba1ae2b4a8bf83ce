"""CPU: the public surface of the thin-operand session kernels -- the counters, the diagnostic session hook and the option
thin_slab_complex -- is in the generated C header, in the ctypes layer, and (where the library is built) among the library's
symbols; the option's default is 1 in a fresh process wherever the library can be loaded."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ntpoly_amd_thin_slab_counts", "ntpoly_amd_session_begin", "ntpoly_amd_session_end")


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "ntpoly_amd.h")).read()
    assert re.search(r"^void ntpoly_amd_thin_slab_counts\(long long\* out\);", h, re.M)
    assert re.search(r"^void ntpoly_amd_session_begin\(const int\* complex_ok\);", h, re.M)
    assert re.search(r"^void ntpoly_amd_session_end\(\);", h, re.M)
    from ntpoly_amd import capi
    assert set(ENTRY_POINTS) <= set(capi.exported_symbols())


def test_ctypes_layer_and_option_name():
    src = open(os.path.join(ROOT, "ntpoly_amd", "host.py")).read()
    for name in ENTRY_POINTS:
        assert "lib.%s(" % name in src, name
    assert re.search(r"^def thin_slab_counts\(\):", src, re.M) and re.search(r"^def solver_session\(complex_ok=True\):", src, re.M)
    assert "finally:\n        lib.ntpoly_amd_session_end()" in src
    wrp = open(os.path.join(ROOT, "ntpoly_amd", "csrc", "wrp.cpp")).read()
    assert wrp.count('"thin_slab_complex"') == 2   # (set_option and get_option)


def test_library_exports_and_default():
    from ntpoly_amd import _build
    if not os.path.exists(_build.LIB):
        return   # (not built here: the header and the sources were checked above)
    code = ("import ctypes, sys; lib = ctypes.CDLL(sys.argv[1]); "
            "[getattr(lib, n) for n in sys.argv[2:]]; "
            "lib.ntpoly_amd_get_option.restype = ctypes.c_int; "
            "print('default', lib.ntpoly_amd_get_option(b'thin_slab_complex'), lib.ntpoly_amd_get_option(b'thin_left'))")
    env = {k: v for k, v in os.environ.items() if k != "NTPOLY_AMD_THIN_SLAB_COMPLEX"}
    r = subprocess.run([sys.executable, "-c", code, _build.LIB] + list(ENTRY_POINTS), capture_output=True, text=True, env=env)
    if r.returncode != 0 and "cannot open shared object" in r.stderr:
        return   # (the library's GPU runtime is not on this machine)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "default 1 1" in r.stdout, r.stdout
