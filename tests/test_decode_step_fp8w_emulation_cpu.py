"""The bound of tests/test_gpu_decode_step_fp8w.py against a CPU emulation of
pli_rms_gemm_nt_fp8w's documented semantics (tests/decode_step_fp8w_cases.py:
emulate_norm's y, the fp32 dot over the widened codes, the scale after the sum,
SwiGLU in fp32, one rounding): over the GPU test's own case list the emulation
must sit at no more than half the bound (lin_ratio <= 0.5), so a correct kernel
has the other half for its different fp32 summation order.  No GPU and no
library call: the case file quantises with torch ops only."""
from __future__ import annotations

import pytest

import decode_step_fp8w_cases as fc


def _worst(cases, dt):
    worst = {}
    for c in cases:
        op = fc.case_operands(c, dt)
        sw = c.kind == "swiglu"
        refs, emus = fc.reference(op, dt, fc.EPS, sw), fc.emulate(op, dt, fc.EPS, sw)
        r = max(fc.lin_ratio(e, ref, dt) for e, ref in zip(emus, refs))
        assert r <= 0.5, (fc.case_id(c), dt, r)
        worst[c.kind] = max(worst.get(c.kind, 0.0), r)
    return worst


@pytest.mark.parametrize("dt", fc.DTYPES)
def test_emulation_sits_at_half_the_gpu_bound(dt):
    worst = _worst(fc.FP8W_CASES + fc.FP8W_LDS_CASES, dt)
    print(f"{dt}: emulation / bound, worst element per kind: " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(worst.items())))
    assert set(worst) == {"linear", "swiglu", "qkv"}


@pytest.mark.parametrize("dt", fc.DTYPES)
def test_statistics_edges_sit_at_half_the_gpu_bound(dt):
    """the operands of the GPU test's statistics-edge runs: rows scaled by 2^-12 (eps dominates the mean) and
    by 2^12, and eps = 0 on unit rows"""
    for kind in ("linear", "swiglu"):
        for K in (2048, 4112):
            c = fc.Fp8Case(kind, K, 2, 2, 1, (10,), False, "res+h", None, K == 2048)
            for scale, eps in ((2.0 ** -12, 1e-6), (2.0 ** 12, 1e-6), (1.0, 0.0)):
                op = fc.case_operands(c, dt, scale)
                sw = kind == "swiglu"
                r = fc.lin_ratio(fc.emulate(op, dt, eps, sw)[0], fc.reference(op, dt, eps, sw)[0], dt)
                assert r <= 0.5, (kind, K, scale, eps, dt, r)


def test_case_list_reaches_every_instance():
    fc.self_test()
    assert len(fc.all_instances()) == 18
    # nothing was replaced: the one-chunk row keeps all three kinds
    assert {c.kind for c in fc.FP8W_CASES if c.K == 16} == {"linear", "swiglu", "qkv"}
