"""CPU: the public surface of the complex sessions of the polynomial and function families -- the option complex_poly_sessions
and the diagnostic entry point of the fused recurrence step -- is in the generated C header, in the ctypes layer, and (where
the library is built) among the library's symbols; wherever the library can be loaded the option reads back its default, 2, in
a fresh process and round-trips 0, 1 and 2 through the C ABI and through ntpoly_amd/host.py."""
import os
import re
import subprocess
import sys

import surface_checks as S

ROOT = S.ROOT
ENTRY_POINTS = ("ntpoly_amd_recurrence_step", "ntpoly_amd_recurrence_step_count")
OPTION = "complex_poly_sessions"
ENV = "NTPOLY_AMD_COMPLEX_POLY_SESSIONS"
src = S.src


def test_header_declares_the_entry_point():
    h = src("include", "ntpoly_amd.h")
    assert re.search(r"^int ntpoly_amd_recurrence_step\(const int\* ih_P, const int\* ih_Tkm2, int\* ih_Tk, int\* ih_R, "
                     r"const double\* a, const double\* c\);", h, re.M)
    assert re.search(r"^void ntpoly_amd_recurrence_step_count\(long long\* out\);", h, re.M)
    from ntpoly_amd import capi
    assert set(ENTRY_POINTS) <= set(capi.exported_symbols())


def test_option_in_every_layer():
    S.check_registered_once(OPTION)
    assert (OPTION, 2, "ENV") in S.OPTIONS   # (the table's entry: the field, its default, its environment variable)
    host = src("ntpoly_amd", "host.py")
    for name in ENTRY_POINTS:
        assert "lib.%s(" % name in host, name
    assert re.search(r"^def recurrence_step\(P, Tkm2, Tk, R, a, c\):", host, re.M)
    assert re.search(r"^def recurrence_step_count\(\):", host, re.M)
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert OPTION in src(doc), doc
    assert ENV in src("INTEGRATION.md")


def run_fresh(code, env):
    from ntpoly_amd import _build
    r = subprocess.run([sys.executable, "-c", code, _build.LIB], capture_output=True, text=True, env=env, cwd=ROOT)
    if r.returncode != 0 and "cannot open shared object" in r.stderr:
        return None   # (the library's GPU runtime is not on this machine)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_library_default_and_round_trip_through_the_c_abi():
    from ntpoly_amd import _build
    if not os.path.exists(_build.LIB):
        return   # (not built here: the header and the sources were checked above)
    code = ("import ctypes, sys; lib = ctypes.CDLL(sys.argv[1]); lib.ntpoly_amd_recurrence_step; lib.ntpoly_amd_recurrence_step_count; "
            "lib.ntpoly_amd_get_option.restype = ctypes.c_int; name = b'%s'; "
            "out = [lib.ntpoly_amd_get_option(name)]; "
            "[(lib.ntpoly_amd_set_option(name, ctypes.byref(ctypes.c_int(v))), out.append(lib.ntpoly_amd_get_option(name))) for v in (0, 1, 2)]; "
            "print('values', *out)") % OPTION
    env = {k: v for k, v in os.environ.items() if k != ENV}
    out = run_fresh(code, env)
    if out is None:
        return
    assert "values 2 0 1 2" in out, out
    out = run_fresh(code, dict(env, **{ENV: "1"}))   # (the environment variable, as its siblings)
    assert "values 1 0 1 2" in out, out


def test_round_trip_through_host_py():
    from ntpoly_amd import _build
    if not os.path.exists(_build.LIB):
        return
    code = ("import sys; sys.path.insert(0, %r)\n"
            "try:\n"
            "    import ntpoly_amd as nt\n"
            "except OSError as e:\n"
            "    print('no runtime', e); sys.exit(0)\n"
            "out = [nt.get_option(%r)]\n"
            "for v in (0, 1, 2):\n"
            "    nt.set_option(%r, v); out.append(nt.get_option(%r))\n"
            "assert callable(nt.recurrence_step) and nt.recurrence_step_count() == 0\n"
            "print('values', *out)\n") % (ROOT, OPTION, OPTION, OPTION)
    env = {k: v for k, v in os.environ.items() if k != ENV}
    out = run_fresh(code, env)
    if out is None or "no runtime" in out:
        return
    assert "values 2 0 1 2" in out, out
