"""CPU: the option block_scope_complex through the C ABI's option entry points (host only, no GPU): its default -- what a drop-in
caller gets -- a set / get round trip, and its environment selector NTPOLY_AMD_BLOCK_SCOPE_COMPLEX."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(code, env):
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout
    return r.stdout.strip().splitlines()[-1]


def test_block_scope_complex_default_and_round_trip():
    env = dict(os.environ)
    env.pop("NTPOLY_AMD_BLOCK_SCOPE_COMPLEX", None)
    code = ("import ntpoly_amd as nt\n"
            "a = nt.get_option('block_scope_complex')\n"
            "nt.set_option('block_scope_complex', 0)\n"
            "b = nt.get_option('block_scope_complex')\n"
            "nt.set_option('block_scope_complex', 1)\n"
            "print(a, b, nt.get_option('block_scope_complex'), nt.get_option('block_scope'))\n")
    assert _run(code, env) == "1 0 1 1"


def test_block_scope_complex_environment():
    env = dict(os.environ, NTPOLY_AMD_BLOCK_SCOPE_COMPLEX="0")
    assert _run("import ntpoly_amd as nt; print(nt.get_option('block_scope_complex'), nt.get_option('block_scope'))", env) == "0 1"
