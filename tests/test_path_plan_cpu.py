"""CPU: the plan of the pathwise driver (recgraph_amd/csrc/rg_path_plan.cpp: plan_pathwise) takes the routes the documents name
— which kernels, geometry, margins and list sizes for a given (parameters, graph sizes, longest read, options, pass) — and
refuses what the kernels cannot take (tests/c/plan_check.cpp, against the host-only sources: no GPU, no HIP)."""
import plan_check_build


def test_plan_routes(tmp_path):
    plan_check_build.run_ok("plan_check", tmp_path, "plan ok")
