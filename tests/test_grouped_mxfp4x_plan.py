"""csrc/grouped_mxfp4x_plan.h on the CPU: tests/host/grouped_mxfp4x_plan_check.cpp, built and run outside Python"""
from test_mxfp4w_plan import run_host_check


def test_routes_gathered_sources_and_stage_layout(tmp_path):
    assert run_host_check(tmp_path, "grouped_mxfp4x_plan_check") == 19
