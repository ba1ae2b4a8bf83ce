"""CPU: the public surface of the tile launcher's record (csrc/spgemm_tile.hpp TileLaunchInfo, what tests/test_gpu_tile_paths.py
proves its paths with) -- the entry point is in the generated C header, in the ctypes layer and (where the library is built)
among the library's symbols; the Python function's docstring names the eight fields of the last launch; the record is filled
inside the launcher and its count is zeroed where the tile-skip counts are."""
import ast
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINT = "ntpoly_amd_last_tile_launch"
FIELDS = ("epi", "nw", "rows", "labelled", "off32", "bsrc", "max_kn", "skip")


def test_header_declares_the_entry_point():
    h = open(os.path.join(ROOT, "include", "ntpoly_amd.h")).read()
    assert re.search(r"^void ntpoly_amd_last_tile_launch\(long long\* out\);", h, re.M)
    from ntpoly_amd import capi
    assert ENTRY_POINT in set(capi.exported_symbols())


def test_ctypes_layer_and_docstring():
    src = open(os.path.join(ROOT, "ntpoly_amd", "host.py")).read()
    assert "lib.%s(" % ENTRY_POINT in src
    fn = [f for f in ast.parse(src).body if isinstance(f, ast.FunctionDef) and f.name == "last_tile_launch"]
    assert len(fn) == 1 and not fn[0].args.args
    doc = ast.get_docstring(fn[0])
    for name in ("launches",) + FIELDS:
        assert "`%s`" % name in doc, name
        assert '"%s"' % name in ast.get_source_segment(src, fn[0]), name   # (... and is a key of the dict it returns)


def test_record_is_filled_by_the_launcher_and_reset_with_the_skip_counts():
    hpp = open(os.path.join(ROOT, "ntpoly_amd", "csrc", "spgemm_tile.hpp")).read()
    m = re.search(r"struct TileLaunchInfo \{(.*?)\n\};", hpp, re.S)
    assert m and "TileLaunchInfo& last_tile_launch();" in hpp
    body = re.sub(r"//[^\n]*", "", m.group(1))
    for name in ("launches",) + FIELDS:
        assert re.search(r"\b%s\b" % name, body), name
    hip = open(os.path.join(ROOT, "ntpoly_amd", "csrc", "spgemm_tile.hip")).read()
    launcher = hip[hip.index("bool launch_spgemm_tile(const TileLaunch& L) {"):]
    assert "TileLaunchInfo& rec = last_tile_launch();" in launcher   # (behind the launch: from the values it used)
    assert launcher.index("hipLaunchKernelGGL") < launcher.index("TileLaunchInfo& rec = last_tile_launch();")
    wrp = open(os.path.join(ROOT, "ntpoly_amd", "csrc", "wrp.cpp")).read()
    reset = wrp[wrp.index("void ntpoly_amd_reset_spgemm_accum() {"):]
    reset = reset[:reset.index("\n}")]
    assert "tile_skip_counts()[0] = tile_skip_counts()[1] = 0;" in reset and "last_tile_launch().launches = 0;" in reset


def test_library_exports_the_entry_point():
    from ntpoly_amd import _build
    if not os.path.exists(_build.LIB):
        return   # (not built here: the header and the sources were checked above)
    code = ("import ctypes, sys; lib = ctypes.CDLL(sys.argv[1]); getattr(lib, sys.argv[2]); "
            "out = (ctypes.c_longlong * 9)(*([7] * 9)); lib.ntpoly_amd_last_tile_launch(out); print('record', list(out))")
    r = subprocess.run([sys.executable, "-c", code, _build.LIB, ENTRY_POINT], capture_output=True, text=True)
    if r.returncode != 0 and "cannot open shared object" in r.stderr:
        return   # (the library's GPU runtime is not on this machine)
    assert r.returncode == 0, r.stderr[-2000:]
    # (nothing launched yet: no launches, no instantiation, no source)
    assert "record [0, -1, 0, 0, 0, 0, -1, 0, 0]" in r.stdout, r.stdout
