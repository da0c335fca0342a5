"""The MoE case lists (tests/moe_cases.py) against CPU emulations of the
kernels' documented semantics, without a GPU.

Grouped GEMM: torch fp32 matmul of the 16-bit operands, SwiGLU in fp32, one
rounding, over every GroupedCase in both types, must sit at lin_ratio <= 0.5,
so the bound the GPU test asserts is reachable by the arithmetic alone.
Measured over the list: 0.20 .. 0.33 of the bound in bf16, 0.05 .. 0.10 in
fp16.  A case that exceeds 0.5 is to be replaced, never given a wider bound.

Combine: the fp32 chain acc = fma(w_j, y_j, acc) is emulated and held to 0.5
of the chain term of combine_ratio, K * 2^-23 * sum_j |w_j y_j|, on its own
(measured 0.04 .. 0.49; K = 1 is one fp32 rounding of w y, which approaches
0.5 from below over a few thousand elements and cannot pass it).  The output
rounding that follows is a correct rounding to the storage type: it uses up to
1 / 1.05 of the first term of the bound by itself, for a value just above a
power of two, whatever computed it, so the rounded emulation is held to the
whole bound (<= 1, the figure the GPU test asserts; measured 0.50 .. 0.95),
not to half of it.

Also: the helpers build what they claim (routing, NaN placement, routes, the
instances the lists reach).
"""
from __future__ import annotations

import numpy as np
import pytest

import decode_step_cases as dc
import moe_cases as mc


@pytest.mark.parametrize("dt", dc.DTYPES)
def test_grouped_emulation_stays_inside_half_the_bound(dt):
    lo, hi = float("inf"), 0.0
    for c in mc.GROUPED_CASES + mc.AGREEMENT_CASES[::3] + [c for c, _ in mc.CHAIN_CASES]:
        op = mc.grouped_operands(c, dt)
        r = dc.lin_ratio(mc.emulate_grouped(op, dt), mc.grouped_reference(op), dt)
        lo, hi = min(lo, r), max(hi, r)
        assert r <= 0.5, (mc.grouped_id(c), dt, r)
    print(f"grouped emulation / bound, {dt}: {lo:.3f} .. {hi:.3f}")


@pytest.mark.parametrize("dt", dc.DTYPES)
def test_combine_chain_emulation_stays_inside_half_its_term(dt):
    lo, hi = float("inf"), 0.0
    for c in mc.COMBINE_CASES:
        op = mc.combine_operands(c.T, c.K, c.H, dt)
        ref, mag = mc.combine_reference(*op)
        chain = np.abs(mc.emulate_combine_f32(*op).astype(np.float64) - ref)
        r = float((chain / np.maximum(c.K * 2.0 ** -23 * mag, np.finfo(np.float64).tiny)).max())  # (0 / tiny: w = 0)
        lo, hi = min(lo, r), max(hi, r)
        assert r <= 0.5, (mc.combine_id(c), dt, r)
        # (the unrounded chain against the whole bound is smaller still)
        assert mc.combine_ratio(mc.emulate_combine_f32(*op), ref, mag, c.K, dt) <= 0.5
    print(f"combine fp32 chain / chain term, {dt}: {lo:.3f} .. {hi:.3f}")


@pytest.mark.parametrize("dt", dc.DTYPES)
def test_combine_rounded_emulation_stays_inside_the_bound(dt):
    lo, hi = float("inf"), 0.0
    for c in mc.COMBINE_CASES:
        op = mc.combine_operands(c.T, c.K, c.H, dt)
        ref, mag = mc.combine_reference(*op)
        r = mc.combine_ratio(mc.emulate_combine(*op, dt), ref, mag, c.K, dt)
        lo, hi = min(lo, r), max(hi, r)
        assert r <= 1.0, (mc.combine_id(c), dt, r)
    print(f"combine rounded emulation / bound, {dt}: {lo:.3f} .. {hi:.3f}")


def test_combine_ratio_sees_a_wrong_row_a_dropped_term_and_nan():
    c = mc.CombineCase(3, 2, 2056, False)
    op = mc.combine_operands(c.T, c.K, c.H, "bf16")
    ref, mag = mc.combine_reference(*op)
    good = mc.emulate_combine(*op, "bf16")
    assert mc.combine_ratio(good, ref, mag, c.K, "bf16") <= 1.0
    swapped = op.pos.copy()
    swapped[1] = swapped[1, ::-1]  # the right rows under the wrong weights
    assert mc.combine_ratio(mc.emulate_combine(op.y, swapped, op.w, "bf16"), ref, mag, c.K, "bf16") > 10
    assert mc.combine_ratio(mc.emulate_combine(op.y, op.pos[:, :1], op.w[:, :1], "bf16"), ref, mag, c.K, "bf16") > 10
    unnamed = [r for r in range(op.y.shape[0]) if r not in set(op.pos.ravel().tolist())]
    assert len(unnamed) == 3 and np.isnan(op.y[unnamed]).all() and np.isfinite(op.y[op.pos.ravel()]).all()
    wrong = op.pos.copy()
    wrong[2, 1] = unnamed[0]
    assert mc.combine_ratio(mc.emulate_combine(op.y, wrong, op.w, "bf16"), ref, mag, c.K, "bf16") == float("inf")
    one_ulp = good.copy()
    one_ulp[0, -1] *= 1 + 2.0 ** -7  # the last column of the second pass, one bf16 ulp off
    assert mc.combine_ratio(one_ulp, ref, mag, c.K, "bf16") > 1.0
    assert (op.w == 0).sum() == 1 and (op.w > 0).any() and (op.w < 0).any()
    assert len(set(op.pos.ravel().tolist())) == c.T * c.K


def test_synthetic_routing_is_what_the_grouped_tests_assume():
    for c in mc.GROUPED_CASES:
        op = mc.grouped_operands(c, "bf16")
        assert np.array_equal(op.offsets, np.concatenate([[0], np.cumsum(c.counts)]))
        assert op.gather.shape == (sum(c.counts),) and op.gather.dtype == np.int32 and op.offsets.dtype == np.int32
        assert 0 <= op.gather.min() and op.gather.max() < op.tokens
        per_expert = [op.gather[op.offsets[e]:op.offsets[e + 1]] for e in range(c.E)]
        assert all(len(set(g.tolist())) == len(g) for g in per_expert)       # at most once per expert
        seen = np.bincount(op.gather, minlength=op.tokens)
        assert (seen == 0).any()                                             # a token nobody reads: NaN
        if sum(1 for n in c.counts if n) > 1:
            assert seen.max() == sum(1 for n in c.counts if n)               # a token every live expert reads
        assert np.isnan(op.x[seen == 0]).all() and np.isfinite(op.x[seen > 0]).all()
        for e in range(c.E):                                                 # an expert without rows: NaN weights
            assert np.isnan(op.w[e]).all() if c.counts[e] == 0 else np.isfinite(op.w[e]).all()
        ref = mc.grouped_reference(op)
        assert ref.shape == (sum(c.counts), c.n) and np.isfinite(ref).all()
        assert not np.array_equal(op.gather, np.arange(len(op.gather)))      # reading row pr for gather[pr] shows


def test_case_lists_reach_every_instance():
    routes = {c.route for c in mc.GROUPED_CASES}
    want = ({f"gemm_grouped_nt<NBG{g},SW{s}>" for g in (1, 2, 4, 8) for s in (0, 1)} |
            {f"gemm_grouped_lds_nt<MC{m},SW{s}>" for m in (1, 2, 3, 4) for s in (0, 1)} |
            {f"gemm_256g<SW{s}>" for s in (0, 1)})
    assert routes == want
    nt = [c for c in mc.GROUPED_CASES if c.route.startswith("gemm_grouped_nt")]
    body = lambda c: c.k // 4 >= 32 * (4 if c.swiglu else 8)  # noqa: E731
    rem = lambda c: (c.k // 4) % (32 * (4 if c.swiglu else 8)) != 0  # noqa: E731
    assert any(not body(c) for c in nt) and any(body(c) and not rem(c) for c in nt) and any(body(c) and rem(c) for c in nt)
    assert any(max(c.counts) > 128 for c in nt)                               # a second chunk of the c0 loop
    lds = [c for c in mc.GROUPED_CASES if c.route.startswith("gemm_grouped_lds_nt")]
    assert any(sum(c.counts) == 1024 for c in lds) and any(c.k == 128 for c in lds)
    assert any(c.n in (384, 192) for c in lds)
    g = [c for c in mc.GROUPED_CASES if c.route.startswith("gemm_256g")]
    assert {c.counts for c in g} == {(255, 257), (256, 0, 1), (1100, 1100)}
    assert any(c.variant is None and sum(c.counts) == 2200 for c in g)
    for fam in (nt, lds, g):
        assert {c.padded for c in fam} == {True, False} and {c.use_gather for c in fam} == {True, False}
    # the routes of the agreement shapes differ between the variants
    for i in range(0, len(mc.AGREEMENT_CASES), 3):
        assert len({c.route for c in mc.AGREEMENT_CASES[i:i + 3]}) == 2
    assert mc.grouped_route(2, 2200, 128, False, None) == "gemm_256g<SW0>"
    assert mc.grouped_route(8, 16, 128, False, None) == "gemm_grouped_nt<NBG1,SW0>"   # rows_bound > 16 for the LDS route
    assert mc.grouped_route(8, 17, 128, False, None) == "gemm_grouped_lds_nt<MC1,SW0>"
    assert mc.grouped_route(8, 1025, 128, False, 2) == "gemm_grouped_nt<NBG8,SW0>"
    # router and combine lists
    assert {(c.T, c.E, c.k) for c in mc.ROUTE_CASES} == set(mc.ROUTE_TEK)
    for tek in mc.ROUTE_TEK:
        assert {c.logits_dtype for c in mc.ROUTE_CASES if (c.T, c.E, c.k) == tek and c.kind == "normal"
                and c.normalize} == set(mc.LOGITS_DTYPES)
    assert sum(1 for c in mc.ROUTE_CASES if not c.normalize) >= 3
    assert {c.kind for c in mc.ROUTE_CASES} == set(mc.ROUTE_KINDS)
    assert {c.ld_pad > 0 for c in mc.ROUTE_CASES} == {True, False}
    assert {c.H for c in mc.COMBINE_CASES} == {8, 2048, 2056, 4104}
    assert {c.K for c in mc.COMBINE_CASES} == {1, 2, 8} and {c.T for c in mc.COMBINE_CASES} == {1, 3}
    assert {c.padded for c in mc.COMBINE_CASES} == {True, False}


def test_router_guards_see_stray_writes():
    """the fp32 Guarded (weights) and the int32 guard buffers notice one changed element on either side"""
    import torch
    g = dc.Guarded((3, 2), "fp32", "cpu")
    g.view.fill_(0.25)
    dc.assert_untouched(g, lambda v: v)
    for at in (g.guard - 1, g.guard + 6):
        keep = g.buf.clone()
        g.buf[at] = 0.0
        with pytest.raises(AssertionError, match="outside the addressed region"):
            dc.assert_untouched(g, lambda v: v)
        g.buf.copy_(keep)
    b = mc.GuardedInts(7, "cpu")
    b.view[:5] = torch.arange(5, dtype=torch.int32)
    assert b.stray_writes().numel() == 0 and b.stray_writes(5).numel() == 0
    b.view[5] = 0
    assert b.stray_writes(5).tolist() == [5] and b.stray_writes().numel() == 0
    b.buf[b.guard - 1] = 3
    b.buf[b.guard + 7] = 0
    assert b.stray_writes().tolist() == [-1, 7]


def test_route_inputs_meet_the_separation_condition():
    """asserted when moe_cases is imported; restated with the figures: smallest non-zero gap per logits type"""
    from oracle.linear import moe_route
    worst = {}
    for c in mc.ROUTE_CASES:
        lg = mc.route_logits(c)
        assert np.array_equal(lg, dc.round_to_dtype(lg, c.logits_dtype))     # values of the type
        gap = mc.route_separation(lg, c.k)
        assert gap >= mc.SEPARATION, (mc.route_id(c), gap)
        worst[c.logits_dtype] = min(worst.get(c.logits_dtype, float("inf")), gap)
        w, idx = moe_route(lg, c.k, bool(c.normalize))
        if c.kind == "equal_row":
            assert idx[c.T // 2].tolist() == list(range(c.k))
        if c.kind == "dup":
            mx = lg.max(-1)
            assert ((lg == mx[:, None]).sum(-1) >= 2).all() and (idx[:, 0] == np.argmax(lg, -1)).all()
        if c.kind == "dead":
            assert not set(idx.ravel().tolist()) & set(mc.DEAD[c.E])
    print("smallest non-zero gap: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert mc.route_separation(np.array([[0.0, 1e-6, -3.0]]), 1) < mc.SEPARATION  # the condition can fail
