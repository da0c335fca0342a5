"""pli_hip.quantize_weight_fp8 on the CPU: per-output-row e4m3fn codes and fp32
scales, value = code * scale[row] (include/pli.h, the weight-only fp8 linear)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle.numerics import seeded_normal


@pytest.fixture(scope="module")
def w():
    a = seeded_normal((37, 200), 4100, "fp32").astype(np.float32)
    a[5] = 0.0                       # an all-zero row
    a[7] *= 0.05                     # a small row (its codes' values stay fp16 values: >= 2^-24 apart)
    a[9] *= 300.0                    # a large one
    a[11, 3] = 0.0
    return torch.from_numpy(a)


def test_codes_are_torchs_clamp_and_cast_and_scale_is_absmax_over_448(built_lib, w):
    import pli_hip
    codes, scale = pli_hip.quantize_weight_fp8(w)
    assert codes.dtype == torch.float8_e4m3fn and tuple(codes.shape) == tuple(w.shape)
    assert scale.dtype == torch.float32 and tuple(scale.shape) == (w.shape[0],)
    amax = w.abs().amax(dim=1)
    want_scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    assert torch.equal(scale, want_scale)
    want = (w.float() * (1.0 / want_scale)[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    assert torch.equal(codes.view(torch.uint8), want.view(torch.uint8))
    # bf16 / fp16 sources are quantised from their fp32 values
    for dt in (torch.bfloat16, torch.float16):
        c2, s2 = pli_hip.quantize_weight_fp8(w.to(dt))
        c3, s3 = pli_hip.quantize_weight_fp8(w.to(dt).float())
        assert torch.equal(c2.view(torch.uint8), c3.view(torch.uint8)) and torch.equal(s2, s3)


def test_zero_row_and_row_maximum(built_lib, w):
    import pli_hip
    codes, scale = pli_hip.quantize_weight_fp8(w)
    u = codes.view(torch.uint8)
    assert scale[5].item() == 1.0 and int(u[5].max()) == 0
    for j in range(w.shape[0]):
        if j == 5:
            continue
        i = int(w[j].abs().argmax())
        assert int(u[j, i]) == (0x7E if w[j, i] > 0 else 0xFE), "the row maximum maps to +-448"
    assert not bool(((u & 0x7F) == 0x7F).any()), "no NaN code"


def test_elementwise_error_bound(built_lib, w):
    """|w - w^| <= 2^-4 |w| + scale 2^-10: half an ulp of a 3-bit mantissa, half the subnormal step"""
    import pli_hip
    codes, scale = pli_hip.quantize_weight_fp8(w)
    deq = codes.float().double() * scale.double()[:, None]
    err = (w.double() - deq).abs()
    # the fp32 product w * (1 / scale) adds a relative 2^-23 or so before the rounding: far inside the slack of
    # a bound stated in exact arithmetic (1e-6 relative)
    bound = (2.0 ** -4) * w.double().abs() * (1 + 1e-6) + scale.double()[:, None] * 2.0 ** -10
    assert bool((err <= bound).all()), float((err - bound).max())


def test_non_finite_weights_raise(built_lib, w):
    import pli_hip
    for bad in (float("nan"), float("inf"), float("-inf")):
        v = w.clone()
        v[3, 4] = bad
        with pytest.raises(ValueError, match="non-finite"):
            pli_hip.quantize_weight_fp8(v)
    with pytest.raises(ValueError):
        pli_hip.quantize_weight_fp8(w[0])
    with pytest.raises(ValueError, match="scale"):
        pli_hip.quantize_weight_fp8(w, scale=torch.zeros(w.shape[0]))


def test_power_of_two_scales_give_16_bit_exact_values(built_lib, w):
    """quantised against power-of-two scales, the dequantised values are exactly representable in bf16 and fp16
    (a 4-bit significand times a power of two, inside both exponent ranges)"""
    import pli_hip
    amax = w.abs().amax(dim=1).clamp_min(1e-6)
    scale = torch.exp2(torch.ceil(torch.log2(amax / 448.0)))
    scale[5] = 1.0
    codes, s = pli_hip.quantize_weight_fp8(w, scale=scale)
    assert torch.equal(s, scale)
    want = (w * (1.0 / scale)[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    assert torch.equal(codes.view(torch.uint8), want.view(torch.uint8))
    deq = codes.float() * scale[:, None]
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(deq.to(dt).float(), deq), dt
    assert float((w - deq).abs().max()) <= float((w.abs() * 2.0 ** -4 + scale[:, None] * 2.0 ** -10).max())


def test_benchmark_gemv_fp8w_counts_fp8_bytes(built_lib):
    """ch03.benchmark_gemv_fp8w: benchmark_gemv's result type with the byte count m k + 4 m + 2 k + 2 m"""
    import ch03
    m, k = 24, 64
    assert ch03.gemv_fp8w_bytes(m, k, torch.bfloat16) == m * k + 4 * m + 2 * k + 2 * m
    r = ch03.benchmark_gemv_fp8w(m, k, dtype=torch.bfloat16, warmup=1, iterations=3, device="cpu")
    assert isinstance(r, ch03.gemv_benchmark.BenchmarkResult) and r.kernel_us is None and r.mean_us > 0
    assert r.memory_gbps * 1e9 * r.mean_us * 1e-6 == pytest.approx(ch03.gemv_fp8w_bytes(m, k), rel=1e-9)
