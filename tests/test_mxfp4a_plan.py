"""The plan of the W4A8 GEMM (csrc/mxfp4a_plan.h) on the CPU: tests/host/mxfp4a_plan_check.cpp replays the W side of
gemm_mxfp4_mx (staging, swizzle, nibble and scale byte of every operand slot, bank slots of every ds_read_b128 phase,
C stores) and the route rule; built and run as tests/test_mxfp4w_plan.py does, outside Python."""
from test_mxfp4w_plan import run_host_check


def test_w_image_scale_bytes_bank_slots_and_routes(tmp_path):
    assert run_host_check(tmp_path, "mxfp4a_plan_check") > 400
