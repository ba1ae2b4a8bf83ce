"""CPU: the public surface of the thin-operand session kernels -- the counters, the diagnostic session hook and the option
thin_slab_complex -- is in the generated C header, in the ctypes layer, and (where the library is built) among the library's
symbols; the option's default is 1 in a fresh process wherever the library can be loaded."""
import os
import re
import subprocess
import sys

import surface_checks as S

ROOT = S.ROOT
ENTRY_POINTS = ("ntpoly_amd_thin_slab_counts", "ntpoly_amd_session_begin", "ntpoly_amd_session_end")


def test_header_declares_the_entry_points():
    h = S.src("include", "ntpoly_amd.h")
    assert re.search(r"^void ntpoly_amd_thin_slab_counts\(long long out\[6\]\);", h, re.M)
    assert re.search(r"^void ntpoly_amd_session_begin\(const int\* complex_ok\);", h, re.M)
    assert re.search(r"^void ntpoly_amd_session_end\(\);", h, re.M)
    from ntpoly_amd import capi
    assert set(ENTRY_POINTS) <= set(capi.exported_symbols())


def test_ctypes_layer_and_option_name():
    import ntpoly_amd as nt
    src = S.src("ntpoly_amd", "host.py")
    for name in ENTRY_POINTS[1:]:
        assert "lib.%s(" % name in src, name
    # (thin_slab_counts is defined from host.py's counter table, which calls the entry point of that name)
    assert "thin_slab" in nt.host._COUNTERS and callable(nt.thin_slab_counts) and len(nt.thin_slab_counts()) == 6
    assert re.search(r"^def solver_session\(complex_ok=True\):", src, re.M)
    assert "finally:\n        lib.ntpoly_amd_session_end()" in src
    S.check_registered_once("thin_slab_complex")


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
