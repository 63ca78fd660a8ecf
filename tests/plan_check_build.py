"""Builds and runs the host-only plan programs of tests/c/ (plan_check_common.hpp) against the library's host sources: g++, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recgraph_amd", "csrc")
HOST_SOURCES = ("rg_path_plan.cpp", "rg_steps.cpp", "rg_graph.cpp", "rg_gaf.cpp", "rg_reads.cpp")


def build(name, out_dir):
    """tests/c/<name>.cpp -> the path of the program, in out_dir."""
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "c", name + ".cpp")]
                          + [os.path.join(CSRC, f) for f in HOST_SOURCES] + ["-lpthread"])
    return exe


def run_ok(name, out_dir, ok_line):
    """Builds and runs a CHECK program: exit status 0 and its closing line, or the failed checks it printed."""
    r = subprocess.run([build(name, out_dir)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == ok_line, (r.stdout, r.stderr[-4000:])
