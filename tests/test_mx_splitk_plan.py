"""The plan of the split-K block-scaled GEMM (csrc/mx_splitk_plan.h) on the CPU: tests/host/mx_splitk_plan_check.cpp
replays the split rule and its chunks for every (ks, S) up to ks = 128 and gemm_mx_splitk's staging, operand k maps,
bounds and workspace stores for each MC and both weight formats; built and run as tests/test_mxfp4w_plan.py does,
outside Python."""
from test_mxfp4w_plan import run_host_check


def test_chunks_operand_k_maps_bounds_and_partial_stores(tmp_path):
    assert run_host_check(tmp_path, "mx_splitk_plan_check") > 5000
