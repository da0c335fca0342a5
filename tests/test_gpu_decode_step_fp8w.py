"""pli_rms_gemm_nt_fp8w (rms_linear_fp8w / rms_swiglu_fp8w /
rms_qkv_into_cache_fp8w) against the float64 oracle, against the unfused
launches bit for bit, and under ch02.Fp8WeightModel(fused_decode=True).

Inputs, guarded outputs and the bound are tests/decode_step_cases.py's; the
quantised weights, references and the case list are
tests/decode_step_fp8w_cases.py's.  Per element:
* h_out: bitwise the torch CPU add a + residual in the storage type.
* outputs: |err| <= LIN_TOL * (|ref| + 1), bf16 1e-2, fp16 4e-3, ref = float64
  over decode(code) * scale on the stored h.  The CPU emulation of the
  documented semantics (tests/test_decode_step_fp8w_emulation_cpu.py) reaches
  0.46 (bf16) / 0.14 (fp16) of it over this list; the kernels on an MI355X
  reach 0.40 / 0.13 (linear), 0.38 / 0.10 (SwiGLU), 0.38 / 0.11 (qkv), the
  statistics edges included (the worst "err / bound" these tests print, taken
  from two runs of this file with -s on an MI355X).
* everything outside the addressed elements keeps the sentinel's bits.

Kernel instances: rms_gemm_fp8w<T, NB, ROWS, CPL, SW, RPT>, T bf16 and fp16:
K 16 / 2048 -> RPT 1 and the short-row form (ROWS, CPL) = (4, 2) / SwiGLU
(2, 2); 2064 / 4096 -> RPT 2 and the long-row form (2, 4) / (1, 4); 4112 /
6160 / 8176 / 8192 -> RPT 4, long-row; M 1 / 2 / 3-4 -> NB 1 / 2 / 4.  All 18
(SW, NB, form) instances run per type (the case file's self-test).  K 16 /
2064 / 4112 / 6160 / 8176 leave the last weight trip partial (clamped loads);
the long-row loop takes a second trip from K 4112; widths (5, 3, 2) put two
group boundaries inside one wave's ROWS rows, (1,) leaves 3 waves inactive and
clamps ROWS - 1 rows of the fourth.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import decode_step_cases as dc
import decode_step_fp8w_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"
S_MAX = fc.S_MAX


@pytest.fixture(scope="module")
def pli():
    import pli_hip
    pli_hip.lib()
    return pli_hip


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int16)


def _route(kind):
    return "rms_gemm_fp8w<swiglu>" if kind == "swiglu" else "rms_gemm_fp8w"


def _run(pli, c, dt, eps=fc.EPS, scale=1.0, op=None, null_scales=False):
    """one fused call of case c -> (operands, h Guarded | None, output Guardeds [B, rows, n])"""
    op = op or fc.case_operands(c, dt, scale)
    pad = 8 if c.padded else 0
    a = fc.row_view(op.a, dt, DEV, pad)
    r = fc.row_view(op.residual, dt, DEV, pad) if op.residual is not None else None
    g = dc.t16(op.g, dt, DEV)
    w = [fc.codes_view(q, DEV, c.padded) for q in op.q]
    if null_scales:
        w = [(codes, None) for codes, _ in w]
    h = fc.Guarded((c.M, c.K), dt, DEV, strides=(c.K + pad, 1)) if "h" in c.res else None
    hv = h.view if h is not None else None
    if c.kind == "qkv":
        pos = torch.tensor([fc.POS[c.pos]], dtype=torch.int32, device=DEV)
        outs = dc.group_outputs(c.B, c.S, c.widths, S_MAX, dt, DEV, c.padded)
        pli.rms_qkv_into_cache_fp8w(a.unflatten(0, (c.B, c.S)), g, eps, w[0], w[1], w[2], outs[0].view,
                                    outs[1].view.unsqueeze(2), outs[2].view.unsqueeze(2), pos,
                                    residual=r.unflatten(0, (c.B, c.S)) if r is not None else None, h_out=hv)
    else:
        n = c.widths[0]
        st = n + (4 if c.padded else 0)
        out = fc.Guarded((c.M, 1, n), dt, DEV, strides=(st, st, 1))
        outs = [out]
        if c.kind == "linear":
            pli.rms_linear_fp8w(a, g, eps, *w[0], residual=r, h_out=hv, out=out.view[:, 0])
        else:
            wu = fc.codes_view(op.qu[0], DEV, c.padded)
            if null_scales:
                wu = (wu[0], None)
            pli.rms_swiglu_fp8w(a, g, eps, *w[0], *wu, residual=r, h_out=hv, out=out.view[:, 0])
    assert pli.last_route() == _route(c.kind)
    return op, h, outs


def _check(c, dt, op, h, outs, eps=fc.EPS):
    what = f"{fc.case_id(c)} {dt}"
    if h is not None:
        assert torch.equal(_bits(h.view), _bits(fc.stored_h(op, dt))), f"{what}: h_out is not the torch add"
        fc.assert_untouched(h, lambda v: v, what=f"{what} h_out")
    refs = fc.reference(op, dt, eps, c.kind == "swiglu")
    p0 = fc.POS[c.pos] if c.pos else 0
    for gi, (o, ref, n) in enumerate(zip(outs, refs, c.widths)):
        r0, nr = dc.written_rows(gi, c.S, p0, o.shape[1])
        got = dc.f64(o.view[:, r0:r0 + nr, :n])
        ratio = fc.lin_ratio(got, ref.reshape(c.B, c.S, n)[:, :nr], dt)
        print(f"{what} group {gi}: rows {r0}..{r0 + nr - 1}, err / bound {ratio:.3f}")
        assert ratio <= 1.0, (what, gi, ratio)
        fc.assert_untouched(o, lambda v: v[:, r0:r0 + nr, :n], what=f"{what} group {gi}")


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("case", fc.FP8W_CASES, ids=fc.case_id)
def test_fused_fp8w_vs_oracle(pli, case, dt):
    """h_out bitwise the torch add (written once whatever the grid, not at all when NULL), every output element
    within the linear bound of the float64 reference, rows past the capacity dropped, nothing else written"""
    op, h, outs = _run(pli, case, dt)
    _check(case, dt, op, h, outs)


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("case", fc.FP8W_LDS_CASES, ids=fc.case_id)
def test_fused_fp8w_m4_k8192(pli, case, dt):
    """the largest accepted shape: 65536 bytes of dynamic LDS next to the kernel's 16 static ones"""
    op, h, outs = _run(pli, case, dt)
    _check(case, dt, op, h, outs)


# ------------------------------------------------------- bitwise the unfused launches
@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("K", [2048, 4112, 8192])
def test_fused_is_bitwise_the_unfused_launches(pli, K, M, dt):
    """pli_rmsnorm -> pli_linear_fp8w / pli_linear_swiglu_fp8w on the vec route (widths that are no multiple of 16
    keep m > 1 off the MFMA kernel) == the fused launch, bit for bit: same y, same chunk map, pairing, accumulate
    order, reduction, scale and rounding"""
    widths = (10, 7, 7)
    op = fc.operands(K, M, widths, dt, 300 + K + M, swiglu=True, pow2=bool(M % 2))
    a, r, g = (dc.t16(x, dt, DEV) for x in (op.a, op.residual, op.g))
    w = [fc.codes_view(q, DEV, True) for q in op.q]
    wu = fc.codes_view(op.qu[0], DEV, True)
    h_ref, y = pli.rmsnorm(a, g, fc.EPS, residual=r)
    h = torch.empty_like(a)
    out = pli.rms_linear_fp8w(a, g, fc.EPS, *w[0], residual=r, h_out=h)
    assert torch.equal(_bits(h), _bits(h_ref))
    want = pli.linear_fp8w(y, *w[0])
    assert pli.last_route() == "linear_fp8w_vec"
    assert torch.equal(_bits(out), _bits(want))
    got = pli.rms_swiglu_fp8w(a, g, fc.EPS, *w[0], *wu, residual=r)
    want = pli.linear_swiglu_fp8w(y, *w[0], *wu)
    assert pli.last_route() == "linear_fp8w_vec<swiglu>"
    assert torch.equal(_bits(got), _bits(want))
    # q / k / v: three groups in one launch against three unfused linears; all M rows as one batch of M tokens
    pos = torch.tensor([2], dtype=torch.int32, device=DEV)
    q = torch.zeros(1, M, widths[0], dtype=fc.TDT[dt], device=DEV)
    kc, vc = (torch.zeros(1, S_MAX, 1, n, dtype=fc.TDT[dt], device=DEV) for n in widths[1:])
    pli.rms_qkv_into_cache_fp8w(a.view(1, M, K), g, fc.EPS, *w, q, kc, vc, pos, residual=r.view(1, M, K))
    for got, (codes, scale) in zip((q[0], kc[0, 2:2 + M, 0], vc[0, 2:2 + M, 0]), w):
        want = pli.linear_fp8w(y, codes, scale)
        assert pli.last_route() == "linear_fp8w_vec"
        assert torch.equal(_bits(got), _bits(want))
    assert kc[0, 2].abs().sum().item() > 0 and kc[0, :2].abs().sum().item() == 0


# ------------------------------------------------------------------ statistics edges
@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("K", [2048, 4112])
@pytest.mark.parametrize("kind", ["linear", "swiglu"])
def test_fused_fp8w_statistics_edges(pli, kind, K, dt):
    c = fc.Fp8Case(kind, K, 2, 2, 1, (10,), False, "res+h", None, K == 2048)
    # eps dominating the mean (rows scaled by 2^-12), large rows (2^12), and eps = 0 on unit rows
    for scale, eps in ((2.0 ** -12, 1e-6), (2.0 ** 12, 1e-6), (1.0, 0.0)):
        op, h, outs = _run(pli, c, dt, eps=eps, scale=scale)
        _check(c, dt, op, h, outs, eps=eps)
    # an all-zero row with eps > 0: exact zeros, the other row unaffected
    op = fc.case_operands(c, dt)
    op.a[0], op.residual[0] = 0, 0
    op, h, outs = _run(pli, c, dt, op=op)
    _check(c, dt, op, h, outs)
    assert (outs[0].view[0] == 0).all()
    # one NaN in row 1 of a (in the last, partial chunk trip at K 4112): exactly row 1's outputs are NaN
    op = fc.case_operands(c, dt)
    _, _, clean = _run(pli, c, dt, op=op)
    op.a[1, K - 3] = np.nan
    _, h, outs = _run(pli, c, dt, op=op)
    assert torch.isnan(outs[0].view[1]).all()
    assert torch.equal(_bits(outs[0].view[0]), _bits(clean[0].view[0]))
    assert torch.isnan(h.view[1, K - 3]) and torch.isnan(h.view).sum().item() == 1
    fc.assert_untouched(outs[0], lambda v: v, what="NaN run")
    fc.assert_untouched(h, lambda v: v, what="NaN run h_out")


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("kind,K,M", [("qkv", 2064, 3), ("swiglu", 4112, 4), ("linear", 16, 2)])
def test_nan_code_poisons_exactly_its_column_in_all_rows(pli, kind, K, M, dt):
    widths = (5, 3, 2) if kind == "qkv" else (10,)
    c = fc.Fp8Case(kind, K, M, 1 if kind == "qkv" else M, M if kind == "qkv" else 1, widths, True, "res", "zero" if
                   kind == "qkv" else None, False)
    op = fc.case_operands(c, dt)
    _, _, clean = _run(pli, c, dt, op=op)
    # the last code of a row in the last group (the last, partial chunk trip); SwiGLU: in the up weight
    gi, row = len(widths) - 1, widths[-1] - 1
    target = op.qu[gi][0] if kind == "swiglu" else op.q[gi][0]
    target.view(torch.uint8)[row, K - 1] = fc.NAN_CODE
    _, _, outs = _run(pli, c, dt, op=op)
    for i, (o, cl, n) in enumerate(zip(outs, clean, widths)):
        rows = slice(0, M) if kind == "qkv" else slice(None)
        got, ref = (x.view[0, rows, :n] if kind == "qkv" else x.view[:, 0, :n] for x in (o, cl))
        nan = torch.isnan(got)
        if i == gi:
            assert bool(nan[:, row].all()) and int(nan.sum()) == M
            keep = [j for j in range(n) if j != row]
            assert torch.equal(_bits(got[:, keep]), _bits(ref[:, keep]))
        else:
            assert not bool(nan.any()) and torch.equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("kind", ["linear", "swiglu", "qkv"])
def test_null_scales_are_all_ones(pli, kind, dt):
    c = fc.Fp8Case(kind, 2064, 3, 1 if kind == "qkv" else 3, 3 if kind == "qkv" else 1,
                   (5, 3, 2) if kind == "qkv" else (10,), False, "res", "mid" if kind == "qkv" else None, False)
    # codes 64 times smaller than usual: without their scales silu(g) * u still fits fp16
    op = fc.operands(c.K, c.M, c.widths, dt, fc.case_seed(c, dt), swiglu=kind == "swiglu", coarse=64.0)
    ones = op._replace(q=[(codes, torch.ones_like(s)) for codes, s in op.q],
                       qu=[(codes, torch.ones_like(s)) for codes, s in op.qu] if op.qu else None)
    _, _, want = _run(pli, c, dt, op=ones)
    _, _, got = _run(pli, c, dt, op=op, null_scales=True)
    for a, b in zip(got, want):
        assert torch.equal(_bits(a.buf), _bits(b.buf))
        assert torch.isfinite(a.view).all() and a.view.float().abs().max().item() > 1
    # one NULL entry among given ones (qkv: k's scale NULL == k's scale all ones)
    if kind == "qkv":
        mixed = op._replace(q=[op.q[0], (op.q[1][0], torch.ones_like(op.q[1][1])), op.q[2]])
        _, _, want = _run(pli, c, dt, op=mixed)
        a = fc.row_view(op.a, dt, DEV)
        r = fc.row_view(op.residual, dt, DEV)
        w = [fc.codes_view(q, DEV, False) for q in op.q]
        outs = dc.group_outputs(c.B, c.S, c.widths, S_MAX, dt, DEV, False)
        pli.rms_qkv_into_cache_fp8w(a.unflatten(0, (c.B, c.S)), dc.t16(op.g, dt, DEV), fc.EPS, w[0], (w[1][0], None),
                                    w[2], outs[0].view, outs[1].view.unsqueeze(2), outs[2].view.unsqueeze(2),
                                    torch.tensor([fc.POS["mid"]], dtype=torch.int32, device=DEV),
                                    residual=r.unflatten(0, (c.B, c.S)))
        for x, y in zip(outs, want):
            assert torch.equal(_bits(x.buf), _bits(y.buf))


# ----------------------------------------------------------------------------- graph
def test_graph_replays_after_in_place_changes(pli):
    """one captured call; codes, scales and *row_offset change in place; the replay equals a fresh eager call"""
    dt, K, B, S, widths = "bf16", 2064, 2, 2, (5, 3, 3)  # k and v caches of one shape, as the wrapper asks
    op = fc.operands(K, B * S, widths, dt, 9100, pow2=False)
    other = fc.operands(K, B * S, widths, dt, 9200, pow2=True)
    a, r, g = (dc.t16(x, dt, DEV) for x in (op.a, op.residual, op.g))
    w = [(codes.to(DEV), scale.to(DEV)) for codes, scale in op.q]
    pos = torch.tensor([1], dtype=torch.int32, device=DEV)

    def buffers():
        return (torch.zeros(B, S, widths[0], dtype=torch.bfloat16, device=DEV),
                torch.zeros(B, S_MAX, 1, widths[1], dtype=torch.bfloat16, device=DEV),
                torch.zeros(B, S_MAX, 1, widths[2], dtype=torch.bfloat16, device=DEV),
                torch.zeros(B * S, K, dtype=torch.bfloat16, device=DEV))

    def step(q, kc, vc, h):
        pli.rms_qkv_into_cache_fp8w(a.view(B, S, K), g, fc.EPS, *w, q, kc, vc, pos, residual=r.view(B, S, K), h_out=h)

    static = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(*static)
    for (codes, scale), (codes2, scale2) in zip(w, other.q):
        codes.view(torch.uint8).copy_(codes2.view(torch.uint8).to(DEV))
        scale.copy_(scale2.to(DEV))
    pos.fill_(5)
    for t in static:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    fresh = buffers()
    step(*fresh)
    for got, want in zip(static, fresh):
        assert torch.equal(_bits(got), _bits(want))
    assert static[1][:, 5:7].abs().sum().item() > 0 and static[1][:, :5].abs().sum().item() == 0
    ref = fc.reference(other._replace(a=op.a, residual=op.residual, g=op.g), dt, fc.EPS, False)
    assert fc.lin_ratio(dc.f64(static[0]).reshape(B * S, -1), ref[0], dt) <= 1.0


# ----------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def models(pli):
    """(fused fp8 model, unfused fp8 model, bf16 twin holding the identical dequantised weights): hidden 256,
    2 layers, 4 / 2 heads, 512, vocab 1000; power-of-two scales make every dequantised value a bf16 value"""
    from ch02 import CachedTransformerModel, Fp8WeightModel
    torch.manual_seed(21)
    model = CachedTransformerModel(1000, 256, 2, 4, 2, 512).to(DEV, torch.bfloat16).eval()
    fused = Fp8WeightModel.from_model(model, pow2_scales=True, fused_decode=True)
    plain = Fp8WeightModel.from_model(model, pow2_scales=True)
    with torch.no_grad():
        for b, fb in zip(model.layers, plain.layers):
            packed = fb.qkv.dequantized(torch.float32)
            nq, nk = b.attn.q_proj.weight.shape[0], b.attn.k_proj.weight.shape[0]
            for lin, wt in ((b.attn.q_proj, packed[:nq]), (b.attn.k_proj, packed[nq:nq + nk]),
                            (b.attn.v_proj, packed[nq + nk:]), (b.attn.o_proj, fb.o_proj.dequantized(torch.float32)),
                            (b.ffn.gate_proj, fb.gate.dequantized(torch.float32)),
                            (b.ffn.up_proj, fb.up.dequantized(torch.float32)),
                            (b.ffn.down_proj, fb.down.dequantized(torch.float32))):
                lin.weight.copy_(wt)
        model.lm_head.weight.copy_(plain.lm_head.dequantized(torch.float32))
    return fused, plain, model


def test_model_batch_1_is_bitwise_the_unfused_model(pli, models):
    """m = 1 is the vec route on both sides and the cache rows are equal, so a prefill and 6 steps give the same
    logits bit for bit; the fused steps run the fused kernels"""
    fused, plain, _ = models
    assert fused.fused_decode and not plain.fused_decode
    ids = torch.randint(0, 1000, (1, 20), generator=torch.Generator().manual_seed(6)).to(DEV)
    with torch.no_grad():
        ca = fused.create_caches(1, 32, torch.device(DEV), torch.bfloat16, device_pos=True)
        cb = plain.create_caches(1, 32, torch.device(DEV), torch.bfloat16, device_pos=True)
        a, b = fused(ids, ca, 0), plain(ids, cb, 0)
        assert torch.equal(a, b)
        for step in range(6):
            tok = b[:, -1].argmax(-1, keepdim=True)
            a = fused(tok, ca, 20 + step)
            assert pli.last_route() == "rms_gemm_fp8w", "the step ended in the fused lm_head launch"
            b = plain(tok, cb, 20 + step)
            assert a.shape == b.shape == (1, 1, 1000)
            assert torch.equal(a, b), step
        for x, y in zip(ca, cb):
            assert torch.equal(x.k, y.k) and torch.equal(x.v, y.v) and x.seq_len == y.seq_len == 26
        assert int(ca[0].pos.item()) == 26


def test_model_batch_2_against_the_bf16_twin(pli, models):
    fused, _, model = models
    B = 2
    ids = torch.randint(0, 1000, (B, 20), generator=torch.Generator().manual_seed(7)).to(DEV)
    rel = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())  # noqa: E731
    with torch.no_grad():
        ca = fused.create_caches(B, 32, torch.device(DEV), torch.bfloat16, device_pos=True)
        cb = model.create_caches(B, 32, torch.device(DEV), torch.bfloat16, device_pos=True)
        a, b = fused(ids, ca, 0), model(ids, cb, 0)
        assert rel(a, b) < 1e-2, ("prefill", rel(a, b))
        for step in range(6):
            tok = b[:, -1].argmax(-1, keepdim=True)  # the bf16 model's greedy token for both
            a = fused(tok, ca, 20 + step)
            assert pli.last_route() == "rms_gemm_fp8w"
            b = model(tok, cb, 20 + step)
            assert a.shape == b.shape == (B, 1, 1000)
            print(f"step {step}: relative L2 {rel(a, b):.2e}")
            assert rel(a, b) < 1e-2, (step, rel(a, b))


def test_decode_step_graph_replays_the_fused_models_eager_steps(pli, models):
    from ch08 import DecodeStepGraph
    fused, _, _ = models
    B = 2
    ids = torch.randint(0, 1000, (B, 20), generator=torch.Generator().manual_seed(9)).to(DEV)
    g = DecodeStepGraph(fused, batch_size=B, max_seq_len=32, dtype=torch.bfloat16, device=DEV)
    caches = fused.create_caches(B, 32, torch.device(DEV), torch.bfloat16, device_pos=True)
    with torch.no_grad():
        lg = g.prefill(ids)
        le = fused(ids, caches, 0)
        assert torch.equal(lg, le)
        for step in range(4):
            tok = le[:, -1].argmax(-1, keepdim=True)
            lg = g.step(tok).clone()
            le = fused(tok, caches, 20 + step)
            assert pli.last_route() == "rms_gemm_fp8w"
            assert torch.equal(lg, le), step
