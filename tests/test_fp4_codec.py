"""The MXFP4 codec (csrc/fp4_codec.h) on the CPU: tests/host/fp4_codec_check.cpp checks all 16 codes in both nibble
positions, all 256 scale bytes, and the encoder's ties and saturation; built and run as tests/test_mxfp4w_plan.py's."""
from test_mxfp4w_plan import run_host_check


def test_decode_scales_and_encoder(tmp_path):
    assert run_host_check(tmp_path, "fp4_codec_check") > 256 * 3
