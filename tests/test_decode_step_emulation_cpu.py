"""The decode-step case list against a CPU emulation of the fused kernel's
documented semantics (h rounded to the storage type, fp32 statistics, y
rounded, fp32 dot, SwiGLU in fp32, one output rounding): the reference alone
must stay inside half of the bound the GPU test asserts, for every case that
tests/test_gpu_decode_step.py runs.  A case whose emulation exceeds 0.5 is to
be replaced, never given a wider bound.  Also: the list covers what it claims
to cover, and the sentinel helper notices a stray write."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import decode_step_cases as dc
from oracle import linear as olin


def _emulation_ratio(c, dt, scale=1.0, eps=dc.EPS):
    op = dc.case_operands(c, dt, scale=scale)
    sw = c.kind == "swiglu"
    ref, emu = dc.reference_fused(op, dt, eps, sw), dc.emulate_fused(op, dt, eps, sw)
    return max(dc.lin_ratio(e, r, dt) for e, r in zip(emu, ref))


@pytest.mark.parametrize("dt", dc.DTYPES)
def test_emulation_stays_inside_half_the_bound(dt):
    worst = {"linear": 0.0, "swiglu": 0.0, "qkv": 0.0}
    for c in dc.FUSED_CASES + dc.LDS_CASES:
        r = _emulation_ratio(c, dt)
        worst[c.kind] = max(worst[c.kind], r)
        assert r <= 0.5, (dc.case_id(c), dt, r)
    print(f"emulation / bound, {dt}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("dt", dc.DTYPES)
@pytest.mark.parametrize("kind", ["linear", "swiglu"])
def test_emulation_of_the_statistics_edges(kind, dt):
    """rows scaled by 2^-12 under eps = 1e-6 (eps dominates the mean) and eps = 0 on unit rows, K 2048 and 4104"""
    worst = 0.0
    for K in (2048, 4104):
        c = dc.FusedCase(kind, K, 2, 2, 1, (10,), False, "res+h", None)
        for scale, eps in ((2.0 ** -12, 1e-6), (1.0, 0.0)):
            r = _emulation_ratio(c, dt, scale=scale, eps=eps)
            worst = max(worst, r)
            assert r <= 0.5, (kind, K, scale, eps, r)
    print(f"statistics edges, emulation / bound, {kind} {dt}: {worst:.3f}")


@pytest.mark.parametrize("dt", dc.DTYPES)
def test_emulated_norm_rounds_within_half_an_ulp(dt):
    """y of the emulation against the oracle on the stored h: at most half an ulp (the GPU test allows 1.05x)"""
    worst = 0.0
    for K in (8, 2056, 4104, 8192):
        op = dc.operands(K, 3, (), dt, 77 + K)
        y = dc.f64(dc.emulate_norm(op, dt, dc.EPS))
        ref = olin.rms_norm(dc.f64(dc.stored_h(op, dt)), op.g, dc.EPS)
        worst = max(worst, dc.norm_ratio(y, ref, dt) * dc.NORM_SLACK)
    print(f"norm emulation / half an ulp, {dt}: {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dt", dc.DTYPES)
def test_unfused_multi_cases_stay_inside_half_the_bound(dt):
    """pli_gemm_multi_nt's semantics (fp32 dot of the stored x, one rounding) over its own case list"""
    for c in dc.SKINNY_MULTI_CASES + dc.SMALLM_MULTI_CASES:
        op = dc.operands(c.K, c.B * c.S, c.widths, dt, 5000 + c.K + c.B * c.S, residual=False)
        x = dc.t16(op.a, dt).float()
        for w in op.w:
            emu = dc.f64((x @ dc.t16(w, dt).float().t()).to(dc.TDT[dt]))
            r = dc.lin_ratio(emu, olin.linear(op.a, w), dt)
            assert r <= 0.5, (dc.multi_id(c), dt, r)


def test_case_list_covers_what_the_issue_lists():
    cases = dc.FUSED_CASES + dc.LDS_CASES
    assert 40 <= len(cases) <= 60
    assert {c.K for c in cases} == set(dc.KS)
    # every rms_gemm_skinny<T, NB, SW, RPT> instance is held to the oracle
    assert {dc.fused_instance(c) for c in cases} == {(sw, nb, rpt) for sw in (False, True) for nb in (1, 2, 4)
                                                     for rpt in (1, 2, 4)}
    assert {(c.K, c.M) for c in cases} == {(k, m) for k in dc.KS for m in dc.MS}
    assert all(c.M == c.B * c.S and (c.K, c.M) != (8192, 4) for c in dc.FUSED_CASES)
    assert all((c.K, c.M) == (8192, 4) for c in dc.LDS_CASES)
    for kind in ("linear", "swiglu", "qkv"):
        mine = [c for c in cases if c.kind == kind]
        assert {c.padded for c in mine} == {True, False}, kind
        assert {c.M for c in mine} == set(dc.MS), kind
        assert {c.res for c in mine} == {"res+h", "res", "none", "h"}, kind
    qkv = [c for c in cases if c.kind == "qkv"]
    assert {(c.B, c.S) for c in qkv} == set(dc.TOKEN_SPLITS)
    assert {c.pos for c in qkv} == set(dc.POS)
    assert any(c.pos == "last" and c.S == 2 for c in qkv)  # second token dropped
    assert all(c.widths == (5, 3, 2) for c in qkv)
    single = [c for c in cases if c.kind != "qkv"]
    assert {c.widths for c in single} == {(10,), (1,)}
    # h_out at one workgroup (ntot 1) and at several (ntot > 4)
    assert any(c.widths == (1,) and "h" in c.res for c in single) and any(c.widths == (10,) and "h" in c.res for c in single)
    assert len({dc.case_id(c) for c in cases}) == len(cases)
    assert {c.K for c in dc.SKINNY_MULTI_CASES} == {8, 1024, 1032, 2048, 2056, 4104}
    assert {c.B * c.S for c in dc.SKINNY_MULTI_CASES} == {1, 5, 8, 9, 16}
    assert {c.K for c in dc.SMALLM_MULTI_CASES} == {128, 1024, 1152, 2176}
    assert {c.B * c.S for c in dc.SMALLM_MULTI_CASES} == {17, 32, 33, 64, 65, 128}


@pytest.mark.parametrize("dt", dc.DTYPES)
def test_sentinel_helper_sees_stray_writes(dt):
    g = dc.Guarded((2, 3, 5), dt, "cpu", strides=(40, 9, 1))
    assert g.view.data_ptr() % 16 == 0 and g.guard >= 80
    g.view[:, 1:3, :4] = 1.0
    region = lambda v: v[:, 1:3, :4]  # noqa: E731
    dc.assert_untouched(g, region)
    for poke in (lambda: g.view[1, 1, 4].fill_(0.5), lambda: g.buf[g.guard - 1].fill_(0.0),
                 lambda: g.buf[-1].fill_(float("nan")), lambda: g.view[0, 0, 0].fill_(-1032.0)):
        keep = g.buf.clone()
        poke()
        with pytest.raises(AssertionError, match="outside the addressed region"):
            dc.assert_untouched(g, region)
        g.buf.copy_(keep)
    # padded input views: NaN around the values, values exact
    a = dc.seeded_normal((2, 16), 1, dt)
    v = dc.row_view(a, dt, "cpu", pad=8)
    assert v.stride(0) == 24 and torch.isnan(v._base[:, 16:]).all() and np.array_equal(dc.f64(v), a.astype(np.float64))
    w = dc.weight_view(a, dt, "cpu", padded=True)
    assert w.stride(0) == 32 and w.data_ptr() % 16 == 0 and np.array_equal(dc.f64(w), a.astype(np.float64))
    assert torch.isnan(w._base).sum().item() == 4 * 32 - 2 * 16
