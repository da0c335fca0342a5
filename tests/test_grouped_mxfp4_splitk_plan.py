"""csrc/grouped_mxfp4_splitk_plan.h on the CPU: tests/host/grouped_mxfp4_splitk_plan_check.cpp, built and run outside Python"""
from test_mxfp4w_plan import run_host_check


def test_split_rule_chunks_workspace_staging_offsets_and_reduce(tmp_path):
    assert run_host_check(tmp_path, "grouped_mxfp4_splitk_plan_check") > 1000
