"""The bounds of tests/swiglu_cases.py held against a CPU emulation of the fused
SwiGLU semantics, over the GPU test's own case list: fp32 products and sums of
the rounded inputs (the split route: ks fp32 partials summed in order),
g / (1 + exp(-g)) * u in fp32, one rounding to the storage type.

The emulation is not the kernels' summation order; it shows that a correct
fp32 evaluation leaves room inside the bounds the kernels are held to:

* the fp32 chain before the output rounding <= 0.5 of the bracket of (b);
* the rounded value <= 1.0 of (b) and <= 0.5 of (a).

Measured over the list: the chain takes at most 0.03
(bf16 inputs), 0.05 (fp16) and 0.08 (fp32) of the bracket; the rounded value up
to 0.94 (bf16) and 0.87 (fp16) of (b) -- a correct rounding alone uses up to
1 / 1.05 of its first term -- and at most 0.39 (bf16), 0.12 (fp16) and 0.08
(fp32) of (a).
"""
from __future__ import annotations

import numpy as np
import pytest

import swiglu_cases as sc

PAIRS = [(c, dt) for c in sc.SWIGLU_CASES for dt in c.dts]


@pytest.mark.parametrize("c,dt", PAIRS, ids=lambda v: sc.case_id(v) if isinstance(v, tuple) else v)
def test_emulated_swiglu_sits_inside_both_bounds(c, dt):
    op, ref = sc.case_reference(c, dt)
    ks = sc.split_ks(c)
    chain = sc.chain_ratio(sc.emulate_f32(op, ks), ref)
    ra, rb = sc.ratios(sc.emulate(op, dt, ks), ref, dt)
    print(f"{sc.case_id(c)} {dt}: chain / bracket {chain:.3f}, rounded / (b) {rb:.3f}, rounded / (a) {ra:.3f}")
    assert chain <= 0.5, (sc.case_id(c), dt, chain)
    assert rb <= 1.0 and ra <= 0.5, (sc.case_id(c), dt, ra, rb, sc.worst(sc.emulate(op, dt, ks), ref, dt))


def test_bound_b_is_the_tighter_one_at_small_k_and_the_looser_at_large():
    """(b) / (a) per element: below 1 / 40 at K = 8, above 1 at K = 16384 (why both are asserted)"""
    small = next(c for c in sc.SWIGLU_CASES if (c.m, c.n, c.k) == (16, 8, 8))
    _, ref = sc.case_reference(small, "bf16")
    assert np.median(sc.bound_b(ref, "bf16") / sc.bound_a(ref, "bf16")) < 1 / 40
    big = sc._case(sc.SKINNY, "NB8", (8, 64, 16384))
    ref = sc.reference(sc.operands(big, "bf16"))
    assert np.median(sc.bound_b(ref, "bf16") / sc.bound_a(ref, "bf16")) > 1


def test_the_reference_is_the_oracle():
    """swiglu_cases.reference computes h itself (it needs g and u for the bound): the same numbers as
    oracle.linear.swiglu"""
    from oracle.linear import swiglu
    for c in sc.SWIGLU_CASES[:6]:
        op, ref = sc.case_reference(c, c.dts[0])
        np.testing.assert_array_equal(ref.h, swiglu(op.x, op.wg, op.wu))


def test_a_gate_rounded_to_the_storage_type_breaks_b_only():
    """what (b) buys: rounding g to bf16 before the silu stays inside (a) and leaves (b)"""
    import torch
    c = next(c for c in sc.SWIGLU_CASES if (c.m, c.n, c.k) == (64, 32, 512))
    op, ref = sc.case_reference(c, "bf16")
    x, wg, wu = (torch.from_numpy(np.ascontiguousarray(a)) for a in op)
    g = (x @ wg.t()).bfloat16().float()
    h = sc.f64((g / (1 + torch.exp(-g)) * (x @ wu.t())).bfloat16())
    ra, rb = sc.ratios(h, ref, "bf16")
    assert ra <= 1.0 < rb, (ra, rb)
