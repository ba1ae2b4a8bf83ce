"""CPU: the option complex_density through the C ABI's option entry points (host only, no GPU): its default -- what a drop-in
caller gets -- a set / get round trip, and its environment selector NTPOLY_AMD_COMPLEX_DENSITY."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(code, env):
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout
    return r.stdout.strip().splitlines()[-1]


def test_complex_density_default_and_round_trip():
    env = dict(os.environ)
    env.pop("NTPOLY_AMD_COMPLEX_DENSITY", None)
    code = ("import ntpoly_amd as nt\n"
            "a = nt.get_option('complex_density')\n"
            "nt.set_option('complex_density', 0)\n"
            "b = nt.get_option('complex_density')\n"
            "nt.set_option('complex_density', 1)\n"
            "print(a, b, nt.get_option('complex_density'), nt.get_option('complex_sessions'))\n")
    assert _run(code, env) == "1 0 1 1"


def test_complex_density_environment():
    env = dict(os.environ, NTPOLY_AMD_COMPLEX_DENSITY="0")
    assert _run("import ntpoly_amd as nt; print(nt.get_option('complex_density'), nt.get_option('complex_sessions'))", env) == "0 1"


def test_complex_fusion_counts_entry_point():
    """the counters of complex TRS2 steps kept in slab form are exported and start at zero"""
    env = dict(os.environ)
    code = ("import ntpoly_amd as nt\n"
            "c = nt.complex_fusion_counts()\n"
            "print(c['square'], c['update'], c['repeated'])\n")
    assert _run(code, env) == "0 0 0"
