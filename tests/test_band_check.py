"""CPU: the band of a POA row as the kernels compute it (recgraph_amd/csrc/rg_band.hpp: band_simd of -m 0 SIMD, band_plain of
scalar -m 0 / -m 2) equals the oracle's set_ampl_for_row (utils.rs:17-98) — exhaustively on small reads and on 10^6 seeded
random cases up to 2^20 columns (tests/c/band_check.cpp), for the closed form the kernel runs and for the reference's loops
(-DRG_BAND_SIMD_LOOPS)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("defines", [[], ["-DRG_BAND_SIMD_LOOPS"]], ids=["closed_form", "loops"])
def test_band_functions_equal_set_ampl_for_row(tmp_path, defines):
    exe = tmp_path / "band_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + defines + ["-o", str(exe), os.path.join(ROOT, "tests", "c", "band_check.cpp"),
                                                                    os.path.join(ROOT, "oracle", "orc_common.cpp")])
    r = subprocess.run([str(exe), "1000000", "7"], capture_output=True, text=True, timeout=600)
    d = json.loads(r.stdout)
    assert d["band_simd"] == ("loops" if defines else "closed")
    assert d["exhaustive_cases"] > 3 * 10 ** 8 and d["random_cases"] == 10 ** 6
    assert r.returncode == 0 and d["exhaustive_bad_simd"] == d["exhaustive_bad_plain"] == 0, d
    assert d["random_bad_simd"] == d["random_bad_plain"] == 0, d
