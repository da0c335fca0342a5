"""csrc/grouped_mxfp4_plan.h on the CPU: tests/host/grouped_mxfp4_plan_check.cpp, built and run outside Python"""
from test_mxfp4w_plan import run_host_check


def test_slots_gathered_staging_operand_k_maps_bounds_and_stores(tmp_path):
    assert run_host_check(tmp_path, "grouped_mxfp4_plan_check") > 100
