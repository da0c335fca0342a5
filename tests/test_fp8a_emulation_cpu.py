"""fp8 activations on the CPU: the quantiser's torch path and an fp32 emulation of pli_gemm_fp8's semantics.

* pli_hip.quantize_rows_fp8 on CPU tensors is bitwise pli_hip.quantize_weight_fp8 on finite rows, and follows the
  non-finite rule of include/pli.h element by element;
* the semantics emulated in float32 (fp32 sum of the exact code products, sum * (x_scale * w_scale), + bias, one
  rounding to T) over the case list of tests/fp8a_cases.py leave half of each GPU bound to the kernels: the value
  before the output rounding is within 0.5 of the accumulation bracket of bound (b), and the rounded value within
  0.5 of bound (a).  The output rounding itself is exactly half an ulp, so against the whole of bound (b), whose
  rounding term is 1.05 half-ulps, the rounded value is only asserted to be inside (ratio <= 1): that is the
  condition under which the oracle alone fits the bound;
* the exact patterns of the lane-map test are exact: their float32 emulation equals the float64 value.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import fp8a_cases as fc
from decode_step_cases import TDT
from oracle.numerics import seeded_normal


@pytest.fixture(scope="module")
def pli(built_lib):
    import pli_hip
    return pli_hip


@pytest.mark.parametrize("dt", fc.DTYPES)
def test_quantize_rows_is_quantize_weight_bitwise_on_finite_rows(pli, dt):
    for m, k in [(m, k) for m in fc.QUANT_MS for k in fc.QUANT_KS if k <= 2048] + [(2, fc.QUANT_REG_K + 8)]:
        x = torch.from_numpy(seeded_normal((m, k), 41000 + 3 * m + k, dt)).to(TDT[dt])
        x[0, 0] = 0.0
        got, want = pli.quantize_rows_fp8(x), pli.quantize_weight_fp8(x)
        assert got[0].dtype == torch.float8_e4m3fn and got[1].dtype == torch.float32
        assert torch.equal(got[0].view(torch.uint8), want[0].view(torch.uint8)) and torch.equal(got[1], want[1]), (m, k)
    z = torch.zeros(3, 16, dtype=TDT[dt])
    codes, scale = pli.quantize_rows_fp8(z)
    assert torch.equal(scale, torch.ones(3)) and bool((codes.view(torch.uint8) == 0).all())
    codes, scale = pli.quantize_rows_fp8(torch.zeros(3, 0, dtype=TDT[dt]))
    assert tuple(codes.shape) == (3, 0) and torch.equal(scale, torch.ones(3))


@pytest.mark.parametrize("dt", fc.DTYPES)
def test_quantize_rows_non_finite_rule(pli, dt):
    k = 24
    x = torch.from_numpy(seeded_normal((4, k), 42024, dt)).to(TDT[dt])
    clean = x.clone()
    x[1, 3], x[1, 7], x[1, 11] = float("nan"), float("inf"), float("-inf")
    x[2, 0] = -float("nan")
    x[3] = float("-inf")
    codes, scale = pli.quantize_rows_fp8(x)
    u8 = codes.view(torch.uint8)
    want_codes, want_scale = pli.quantize_weight_fp8(clean)
    # rows without a non-finite element are untouched by the rule
    assert torch.equal(u8[0], want_codes.view(torch.uint8)[0]) and scale[0] == want_scale[0]
    # row 1: the absmax skips the three elements; they get 0x7F, +448, -448; the others are quantised by that scale
    keep = [i for i in range(k) if i not in (3, 7, 11)]
    kc, ks = pli.quantize_weight_fp8(clean[1:2, keep])
    assert scale[1] == ks[0] and torch.equal(u8[1, keep], kc.view(torch.uint8)[0])
    assert (int(u8[1, 3]), int(u8[1, 7]), int(u8[1, 11])) == (0x7F, 0x7E, 0xFE)
    # a NaN of either sign is 0x7F and leaves the rest of its row alone
    kc, ks = pli.quantize_weight_fp8(clean[2:3, 1:])
    assert int(u8[2, 0]) == 0x7F and scale[2] == ks[0] and torch.equal(u8[2, 1:], kc.view(torch.uint8)[0])
    # no finite element: scale 1.0
    assert float(scale[3]) == 1.0 and bool((u8[3] == 0xFE).all())
    with pytest.raises(ValueError):
        pli.quantize_weight_fp8(x)  # the weight quantiser refuses what the row quantiser has a rule for


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("case", fc.GEMM_CASES, ids=fc.case_id)
def test_fp32_emulation_leaves_half_of_each_bound(case, dt):
    op, ref = fc.case_reference(case, dt)
    c32 = fc.emulate_f32(op)
    with np.errstate(divide="ignore", invalid="ignore"):
        chain = np.where(c32 == ref.c, 0.0, np.abs(c32.astype(np.float64) - ref.c) / ref.bracket)
    assert float(chain.max()) <= 0.5, ("accumulation bracket of (b)", float(chain.max()))
    ra, rb = fc.ratios(fc.emulate(op, dt), ref, dt)
    assert ra <= 0.5, ("bound (a)", ra)
    assert rb <= 1.0, ("bound (b)", rb)


def test_exact_patterns_are_exact_in_fp32():
    for k in (fc.KSTEP, 2 * fc.KSTEP):
        x8, w8 = fc.const_rows_codes(k)
        d32 = fc.DECODE.astype(np.float32)
        fin = ~np.isnan(fc.DECODE)
        # running sums of one product, count 1 .. k: each a float32 value
        prod = np.outer(fc.DECODE[fin], fc.DECODE[fin])
        for count in (1, 3, k - 1, k):
            assert np.array_equal((prod * count).astype(np.float32).astype(np.float64), prod * count)
        acc = torch.from_numpy(d32[x8][fin]) @ torch.from_numpy(d32[w8][fin]).t()
        assert np.array_equal(acc.double().numpy(), k * prod)
    m, n, k = fc.TM + 3, fc.TN + fc.STORE_N, 2 * fc.KSTEP
    x8, w8, xv, wv = fc.asymmetric_codes(m, n, k)
    assert np.array_equal(fc.DECODE[x8], xv) and np.array_equal(fc.DECODE[w8], wv)
    assert np.abs(xv).max() * np.abs(wv).max() * k < 2 ** 24, "integer partial sums stay exact in fp32"
    c = xv @ wv.T
    assert not np.array_equal(c[:n, :n], c[:n, :n].T), "the pattern is asymmetric"
    # a k permutation of one operand only, or swapped operands, changes it
    assert not np.array_equal(xv[:, ::-1] @ wv.T, c) and not np.array_equal(np.roll(xv, 32, axis=1) @ wv.T, c)
