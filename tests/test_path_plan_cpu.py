"""CPU: the plan of the pathwise driver (recgraph_amd/csrc/rg_path_plan.cpp: plan_pathwise) takes the routes the documents name
— which kernels, geometry, margins and list sizes for a given (parameters, graph sizes, longest read, options, pass) — and
refuses what the kernels cannot take (tests/c/plan_check.cpp, against the host-only sources: no GPU, no HIP)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_routes(tmp_path):
    csrc = os.path.join(ROOT, "recgraph_amd", "csrc")
    exe = tmp_path / "plan_check"
    srcs = [os.path.join(csrc, f) for f in ("rg_path_plan.cpp", "rg_steps.cpp", "rg_graph.cpp", "rg_gaf.cpp", "rg_reads.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", csrc, "-o", str(exe), os.path.join(ROOT, "tests", "c", "plan_check.cpp")] + srcs
                          + ["-lpthread"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "plan ok", (r.stdout, r.stderr[-4000:])
