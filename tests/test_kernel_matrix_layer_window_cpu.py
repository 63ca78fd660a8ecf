"""CPU: tests/kernel_matrix_layer_window.py is complete, the windowed layer kernel fits beside two sweep waves, and the window
function keeps its promises.

The key set of the matrix must equal the set of `__global__` instantiations hipcc compiles from
recgraph_amd/csrc/layer_window/rg_layer_window.hip (tools/kernel_resources.py report(): cross-compiled for gfx950, no GPU), and no
other file of that directory may hold a kernel without a matrix."""
import os
import subprocess
import sys

import kernel_matrix_layer_window as KW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recgraph_amd", "csrc")
DIR = os.path.join(CSRC, "layer_window")
_REPORT = []


def _report():
    if not _REPORT:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kernel_resources
        _REPORT.extend(kernel_resources.report("layer_window/rg_layer_window.hip"))
    return _REPORT


def test_the_matrix_has_exactly_the_compiled_instantiations():
    assert sorted(f for f in os.listdir(DIR) if f.endswith(".hip")) == ["rg_layer_window.hip"]
    names = [k["name"] for k in _report()]
    assert len(names) == len(set(names))
    compiled, keys = set(names), set(KW.MATRIX)
    assert compiled == keys, {"compiled without an entry": sorted(compiled - keys), "entries without a kernel": sorted(keys - compiled)}
    assert len(compiled) == 6


def test_the_windowed_kernel_fits_beside_two_sweep_waves():
    """Two sweep waves of 224 registers leave 64 of a SIMD's 512 (tests/test_kernel_resources.py): every instantiation takes at most
    64 and no scratch."""
    for k in _report():
        assert k["VGPRs"] <= 64 and k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs Spill"] == 0, k
        assert k["Occupancy [waves/SIMD]"] >= 8, k


def test_window_function(tmp_path):
    """tests/c/layer_window_check.cpp: n in {1, 63, 255, 256, 1000, 1023}, every start cell, both widths — the left edge is a multiple
    of the block width, monotone, inside [0, wpad - W], and the start cell is inside its row's window."""
    exe = tmp_path / "layer_window_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "c", "layer_window_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("layer window ok"), (r.stdout, r.stderr[-2000:])


def test_the_option_is_in_the_table():
    """layer_window: a row of the tuning table (RG_TUNING_OPTIONS, rg_host.hpp), default 256, clamped to [0, 256]."""
    from recgraph_amd import _lib, api
    lib = _lib.load()
    assert lib.rg_get_option(b"layer_window") == 256
    try:
        for v, exp in ((128, 128), (0, 0), (-5, 0), (1000, 256)):
            api.set_option("layer_window", v)
            assert lib.rg_get_option(b"layer_window") == exp
    finally:
        api.set_option("layer_window", 256)
