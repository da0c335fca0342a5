"""Weight-only fp8 linear (pli_linear_fp8w / pli_gemv_fp8w / pli_linear_swiglu_fp8w) on the device.

Oracle: float64 over the dequantised weights decode(code) * scale, computed here with numpy.  Bound: the project's
linear bound |err| <= LIN_TOL[dt] * (|ref| + 1), bf16 1e-2, fp16 4e-3 (an fp32-accumulate emulation of these
semantics stays under 0.38 of it).  The cost of quantising is the format's, not the kernels', and is asserted
nowhere.  Shapes are the smallest at which each piece can go wrong; pli_last_route is asserted for each.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle.numerics import seeded_normal

pytestmark = pytest.mark.gpu

LIN_TOL = {"bf16": 1e-2, "fp16": 4e-3}
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
DEV = "cuda:0"
SENTINEL = -1024.0  # exact in bf16 and fp16
# every e4m3fn code's value (exact in fp32)
DECODE = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def pli(built_lib):
    import pli_hip
    return pli_hip


def pow2_scales(n, seed):
    """2^-8 .. 2^4, a different one on neighbouring rows, so that a scale applied to the wrong row shows"""
    e = np.random.RandomState(seed).permutation(np.arange(n) % 13) - 8
    return torch.from_numpy(np.exp2(e).astype(np.float32))


class Case:
    """x [m, k], codes [n, k] (+ scale), optional bias, all on the device, with padded leading dimensions on request;
    ref(): the float64 oracle over the dequantised weights"""

    def __init__(self, pli, m, n, k, dt, seed, scales="absmax", bias=False, pad=False, swiglu=False):
        self.m, self.n, self.k, self.dt, self.pad = m, n, k, dt, pad
        tdt = TORCH_DT[dt]
        self.x_np = seeded_normal((m, k), seed, dt).astype(np.float64)
        xt = torch.from_numpy(seeded_normal((m, k), seed, dt)).to(tdt)
        if pad:  # ldx = k + 8, NaN in the padding
            xw = torch.full((m, k + 8), float("nan"), dtype=tdt)
            xw[:, :k] = xt
            self.x = xw.to(DEV)[:, :k]
        else:
            self.x = xt.to(DEV)
        self.w = [self._weight(pli, n, k, seed + 1 + i, scales, pad) for i in range(2 if swiglu else 1)]
        self.bias_np = None
        self.bias = None
        if bias:
            b = seeded_normal((n,), seed + 7, dt)
            self.bias_np = b.astype(np.float64)
            self.bias = torch.from_numpy(b).to(tdt).to(DEV)

    @staticmethod
    def _weight(pli, n, k, seed, scales, pad):
        w = torch.from_numpy(seeded_normal((n, k), seed, "fp32"))
        if scales == "pow2":
            sc = pow2_scales(n, seed)
            codes, scale = pli.quantize_weight_fp8(w * 8.0 * sc[:, None], scale=sc)
        else:
            codes, scale = pli.quantize_weight_fp8(w)
        u8 = codes.view(torch.uint8)
        deq = DECODE[u8.numpy()] * (scale.numpy().astype(np.float64)[:, None] if scales is not None else 1.0)
        if pad:  # a column slice of a wider code matrix (ldw = k + 48), NaN codes around it
            wide = torch.full((n, k + 48), 0x7F, dtype=torch.uint8)
            wide[:, 16:16 + k] = u8
            dev_codes = wide.to(DEV)[:, 16:16 + k]
        else:
            dev_codes = u8.to(DEV)
        return dev_codes, (scale.to(DEV) if scales is not None else None), deq

    def out(self):
        tdt = TORCH_DT[self.dt]
        if not self.pad:
            return torch.full((self.m, self.n), SENTINEL, dtype=tdt, device=DEV), None
        whole = torch.full((self.m + 2, self.n + 8), SENTINEL, dtype=tdt, device=DEV)
        return whole[:self.m, :self.n], whole

    def ref(self):
        r = self.x_np @ self.w[0][2].T
        if len(self.w) == 2:
            u = self.x_np @ self.w[1][2].T
            r = r / (1.0 + np.exp(-r)) * u
        if self.bias_np is not None:
            r = r + self.bias_np
        return r


def assert_close(got: torch.Tensor, ref: np.ndarray, dt: str, what):
    g = got.float().cpu().numpy().astype(np.float64)
    err = np.abs(g - ref)
    bound = LIN_TOL[dt] * (np.abs(ref) + 1.0)
    assert np.all(err <= bound), (what, float((err / bound).max()))


def assert_padding_untouched(whole: torch.Tensor, m, n):
    w = whole.float().cpu()
    assert bool((w[m:] == SENTINEL).all()) and bool((w[:, n:] == SENTINEL).all()), "C outside [m, n] was written"


# ---- 1. vec --------------------------------------------------------------------------------------
# (m, n, k, scales, bias, pad): one chunk; a lane tail; both sides of each 64 * CPL chunk trip the plan uses (CPL 2
# up to K = 2048, CPL 4 past it), +-16; N = ROWS q + 1 .. ROWS - 1 (ROWS 4 short rows, 2 long rows); M in {1, 2, 3, 16}
VEC_CASES = [
    (1, 3, 16, "absmax", False, False),
    (1, 5, 16 * 65, "absmax", True, False),
    (2, 6, 2032, "absmax", False, True),
    (1, 7, 2048, None, False, False),
    (3, 5, 2064, "absmax", True, True),
    (1, 9, 4080, "absmax", False, False),
    (16, 5, 4096, "pow2", True, True),
    (1, 3, 4112, "absmax", True, True),
    (2, 3, 8192 + 16, None, False, False),
    (16, 7, 272, "pow2", False, True),
    (3, 17, 48, "absmax", True, False),
]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", VEC_CASES, ids=lambda c: "m{}n{}k{}{}{}".format(c[0], c[1], c[2], "b" if c[4] else "", "p" if c[5] else ""))
def test_vec_against_oracle(pli, case, dt):
    m, n, k, scales, bias, pad = case
    c = Case(pli, m, n, k, dt, 5000 + m + n + k, scales, bias, pad)
    out, whole = c.out()
    pli.linear_fp8w(c.x, c.w[0][0], c.w[0][1], bias=c.bias, out=out)
    assert pli.last_route() == "linear_fp8w_vec"
    assert_close(out, c.ref(), dt, case)
    if whole is not None:
        assert_padding_untouched(whole, m, n)


# ---- 2. smallm -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("k", [256, 512, 9 * 256])  # one body step, two, U steps + one
@pytest.mark.parametrize("m", [2, 15, 16, 17, 33, 128])
def test_smallm_against_oracle(pli, m, k, dt):
    n = 16 if (m + k // 256) % 2 else 48
    c = Case(pli, m, n, k, dt, 6000 + m + k, "pow2", bias=True, pad=(m in (15, 33)))
    out, whole = c.out()
    pli.linear_fp8w(c.x, c.w[0][0], c.w[0][1], bias=c.bias, out=out)
    assert pli.last_route() == "linear_fp8w_smallm"
    assert_close(out, c.ref(), dt, (m, n, k))
    if whole is not None:
        assert_padding_untouched(whole, m, n)


def test_smallm_both_widths_without_bias(pli):
    for n in (16, 48):
        c = Case(pli, 17, n, 512, "bf16", 6100 + n, "pow2")
        got = pli.linear_fp8w(c.x, c.w[0][0], c.w[0][1])
        assert pli.last_route() == "linear_fp8w_smallm"
        assert_close(got, c.ref(), "bf16", n)


# ---- 3. SwiGLU -----------------------------------------------------------------------------------
# m = 1 takes the VALU kernel whatever n is (the route rule puts no condition on n there); k = 40 is the generic one
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("m,n,k,route", [(1, 33, 256, "linear_fp8w_vec<swiglu>"), (1, 48, 256, "linear_fp8w_vec<swiglu>"),
                                         (16, 48, 512, "linear_fp8w_smallm<swiglu>"),
                                         (16, 48, 5 * 256, "linear_fp8w_smallm<swiglu>"),
                                         (3, 5, 4112, "linear_fp8w_vec<swiglu>"),
                                         (2, 33, 40, "linear_fp8w_generic<swiglu>")])
def test_swiglu_against_oracle(pli, m, n, k, route, dt):
    c = Case(pli, m, n, k, dt, 7000 + m + n + k, "absmax", pad=(k % 16 == 0 and n != 33), swiglu=True)
    out, whole = c.out()
    pli.linear_swiglu_fp8w(c.x, c.w[0][0], c.w[0][1], c.w[1][0], c.w[1][1], out=out)
    assert pli.last_route() == route
    assert_close(out, c.ref(), dt, (m, n, k))
    if whole is not None:
        assert_padding_untouched(whole, m, n)


# ---- 4. generic route and fallbacks --------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_generic_k40_and_unaligned_view(pli, dt):
    c = Case(pli, 3, 7, 40, dt, 8000, "pow2", bias=True)
    got = pli.linear_fp8w(c.x, c.w[0][0], c.w[0][1], bias=c.bias)
    assert pli.last_route() == "linear_fp8w_generic"
    assert_close(got, c.ref(), dt, "k40")
    # a W view starting 1 byte into its buffer
    c = Case(pli, 2, 16, 256, dt, 8001, "absmax")
    buf = torch.zeros(16 * 256 + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = c.w[0][0].reshape(-1)
    got = pli.linear_fp8w(c.x, buf[1:].view(16, 256), c.w[0][1])
    assert pli.last_route() == "linear_fp8w_generic"
    assert_close(got, c.ref(), dt, "unaligned")
    # float8 codes are the same bytes
    got8 = pli.linear_fp8w(c.x, c.w[0][0].view(torch.float8_e4m3fn), c.w[0][1])
    assert pli.last_route() == "linear_fp8w_smallm"
    assert_close(got8, c.ref(), dt, "float8 view")


def test_k0_returns_bias_or_zeros(pli):
    x = torch.zeros(3, 0, dtype=torch.bfloat16, device=DEV)
    codes = torch.zeros(5, 0, dtype=torch.uint8, device=DEV)
    bias = torch.arange(5, dtype=torch.bfloat16, device=DEV)
    out = torch.full((3, 5), SENTINEL, dtype=torch.bfloat16, device=DEV)
    pli.linear_fp8w(x, codes, None, out=out)
    assert bool((out == 0).all())
    pli.linear_fp8w(x, codes, None, bias=bias, out=out)
    assert torch.equal(out, bias.expand(3, 5))
    assert pli.last_route() == "linear_fp8w_generic"
    pli.linear_swiglu_fp8w(x, codes, None, codes, None, out=out)
    assert bool((out == 0).all())


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_m17_n24_generic_without_workspace_widen_gemm_with_one(pli, dt):
    m, n, k = 17, 24, 40
    c = Case(pli, m, n, k, dt, 8100, "absmax", bias=True)
    codes, scale = c.w[0][0], c.w[0][1]
    got = pli.linear_fp8w(c.x, codes, scale, bias=c.bias)
    assert pli.last_route() == "linear_fp8w_generic"
    assert_close(got, c.ref(), dt, "generic")
    nbytes = pli.linear_fp8w_workspace_bytes(m, n, k, TORCH_DT[dt])
    assert nbytes == n * k * 2
    ws = torch.zeros(nbytes + 64, dtype=torch.uint8, device=DEV)
    got = pli.linear_fp8w(c.x, codes, scale, bias=c.bias, workspace=ws)
    assert pli.last_route().startswith("fp8w_widen+") and "fp8w" not in pli.last_route()[len("fp8w_widen+"):]
    widened = (codes.view(torch.float8_e4m3fn).float() * scale[:, None]).to(TORCH_DT[dt])
    assert torch.equal(ws[:nbytes].view(TORCH_DT[dt]).view(n, k), widened)
    assert bool((ws[nbytes:] == 0).all()), "the workspace past the widened weight is not written"
    assert torch.equal(got, pli.gemm(c.x, widened, trans_b=True, bias=c.bias))
    ref = c.x_np @ widened.float().cpu().numpy().astype(np.float64).T + c.bias_np
    assert_close(got, ref, dt, "widen+gemm")
    # SwiGLU through the same route: gate, then up
    c = Case(pli, m, n, k, dt, 8200, "absmax", swiglu=True)
    nbytes = pli.linear_fp8w_workspace_bytes(m, n, k, TORCH_DT[dt], swiglu=True)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    got = pli.linear_swiglu_fp8w(c.x, c.w[0][0], c.w[0][1], c.w[1][0], c.w[1][1], workspace=ws)
    assert pli.last_route().startswith("fp8w_widen+fp8w_widen+")
    wd = [(cw.view(torch.float8_e4m3fn).float() * sc[:, None]).to(TORCH_DT[dt]) for cw, sc, _ in c.w]
    assert torch.equal(ws.view(TORCH_DT[dt]).view(2, n, k), torch.stack(wd))
    assert torch.equal(got, pli.gemm_swiglu(c.x, wd[0], wd[1]))
    g = c.x_np @ wd[0].float().cpu().numpy().astype(np.float64).T
    u = c.x_np @ wd[1].float().cpu().numpy().astype(np.float64).T
    assert_close(got, g / (1.0 + np.exp(-g)) * u, dt, "widen+swiglu")


# ---- 5. bitwise properties -----------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(7, 2064), (64, 4096), (5, 40)])
def test_gemv_is_linear_at_m1(pli, n, k):
    c = Case(pli, 1, n, k, "bf16", 9000 + n, "absmax")
    a = pli.linear_fp8w(c.x, c.w[0][0], c.w[0][1])
    route = pli.last_route()
    b = pli.gemv_fp8w(c.w[0][0], c.w[0][1], c.x[0])
    assert pli.last_route() == route
    assert torch.equal(a[0], b)
    assert_close(b[None], c.ref(), "bf16", (n, k))


@pytest.mark.parametrize("m,n,k,route", [(3, 7, 2064, "linear_fp8w_vec"), (17, 48, 512, "linear_fp8w_smallm")])
def test_rows_are_independent_repeatable_and_nan_stays_in_its_row(pli, m, n, k, route):
    c = Case(pli, m, n, k, "bf16", 9100 + m, "pow2", bias=True)
    codes, scale = c.w[0][0].clone(), c.w[0][1]
    a = pli.linear_fp8w(c.x, codes, scale, bias=c.bias)
    assert pli.last_route() == route
    assert torch.equal(a, pli.linear_fp8w(c.x, codes, scale, bias=c.bias)), "two runs differ"
    # other weight rows changed: row 2's outputs keep their bits
    other = codes.clone()
    other[:2] = 0x38
    other[3:] = 0xB1
    b = pli.linear_fp8w(c.x, other, scale, bias=c.bias)
    assert torch.equal(a[:, 2], b[:, 2])
    # other X rows changed: X row 1's outputs keep their bits
    x2 = c.x.clone()
    x2[0] = 3.0
    x2[2:] = -0.5
    b = pli.linear_fp8w(x2, codes, scale, bias=c.bias)
    assert torch.equal(a[1], b[1])
    # one NaN code: exactly that weight row's outputs are NaN
    for code in (0x7F, 0xFF):
        bad = codes.clone()
        bad[4, k // 2 + 3] = code
        b = pli.linear_fp8w(c.x, bad, scale, bias=c.bias)
        nan = torch.isnan(b)
        assert bool(nan[:, 4].all()) and int(nan.sum()) == m
        keep = [j for j in range(n) if j != 4]
        assert torch.equal(a[:, keep], b[:, keep])


# ---- 6. graph ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k", [(4, 48, 512), (4, 7, 2064)])  # smallm, vec
def test_graph_replays_after_in_place_changes(pli, m, n, k):
    c = Case(pli, m, n, k, "bf16", 9500 + n, "pow2", swiglu=True)
    x = c.x.clone()
    (gc, gs, _), (uc, us, _) = [(w[0].clone(), w[1].clone(), None) for w in c.w]
    out = torch.empty(m, n, dtype=torch.bfloat16, device=DEV)
    h = torch.empty(m, n, dtype=torch.bfloat16, device=DEV)

    def step():
        pli.linear_fp8w(x, gc, gs, out=out)
        pli.linear_swiglu_fp8w(x, gc, gs, uc, us, out=h)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    # change x, the codes and the scales in place, then replay
    x.copy_(torch.from_numpy(seeded_normal((m, k), 9600, "bf16")).to(torch.bfloat16))
    gc.copy_(uc)
    uc[1] = 0x3A
    gs.mul_(2.0)
    us.copy_(torch.flip(us, dims=[0]))
    g.replay()
    torch.cuda.synchronize()
    got_out, got_h = out.clone(), h.clone()
    want_out = pli.linear_fp8w(x, gc, gs)
    want_h = pli.linear_swiglu_fp8w(x, gc, gs, uc, us)
    assert torch.equal(got_out, want_out) and torch.equal(got_h, want_h)
    deq = DECODE[gc.cpu().numpy()] * gs.cpu().numpy().astype(np.float64)[:, None]
    assert_close(got_out, x.float().cpu().numpy().astype(np.float64) @ deq.T, "bf16", "graph")


# ---- 7. model ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_pair(pli):
    """(Fp8WeightModel, bf16 CachedTransformerModel holding the identical dequantised weights): power-of-two scales
    make every dequantised value a bf16 value"""
    import torch.nn as nn
    from ch02 import CachedTransformerModel, Fp8WeightModel
    torch.manual_seed(21)
    model = CachedTransformerModel(1000, 256, 2, 4, 2, 512).to(DEV, torch.bfloat16).eval()
    fq = Fp8WeightModel.from_model(model, pow2_scales=True)
    with torch.no_grad():
        blocks = [(b.attn.q_proj, b.attn.k_proj, b.attn.v_proj, b.attn.o_proj, b.ffn.gate_proj, b.ffn.up_proj,
                   b.ffn.down_proj) for b in model.layers]
        for (q, k, v, o, g, u, d), fb in zip(blocks, fq.layers):
            packed = fb.qkv.dequantized(torch.float32)
            assert torch.equal(packed.bfloat16().float(), packed), "dequantised values are bf16 values"
            nq, nk = q.weight.shape[0], k.weight.shape[0]
            for lin, w in ((q, packed[:nq]), (k, packed[nq:nq + nk]), (v, packed[nq + nk:]),
                           (o, fb.o_proj.dequantized(torch.float32)), (g, fb.gate.dequantized(torch.float32)),
                           (u, fb.up.dequantized(torch.float32)), (d, fb.down.dequantized(torch.float32))):
                lin.weight.copy_(w)
        model.lm_head.weight.copy_(fq.lm_head.dequantized(torch.float32))
    assert not any(isinstance(m, nn.Linear) for m in fq.modules())
    return fq, model


@pytest.mark.parametrize("B", [1, 2])
def test_model_against_bf16_model_teacher_forced(pli, model_pair, B):
    fq, model = model_pair
    ids = torch.randint(0, 1000, (B, 20), generator=torch.Generator().manual_seed(5 + B)).to(DEV)
    rel = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())  # noqa: E731
    with torch.no_grad():
        ca = fq.create_caches(B, 32, torch.device(DEV), torch.bfloat16)
        cb = model.create_caches(B, 32, torch.device(DEV), torch.bfloat16)
        a, b = fq(ids, ca, 0), model(ids, cb, 0)
        assert rel(a, b) < 1e-2, ("prefill", rel(a, b))
        for step in range(6):
            tok = b[:, -1].argmax(-1, keepdim=True)  # the bf16 model's greedy token for both
            a, b = fq(tok, ca, 20 + step), model(tok, cb, 20 + step)
            assert a.shape == b.shape == (B, 1, 1000)
            assert rel(a, b) < 1e-2, (step, rel(a, b))


def test_decode_step_graph_replays_its_own_eager_steps(pli, model_pair):
    from ch08 import DecodeStepGraph
    fq, _ = model_pair
    B = 2
    ids = torch.randint(0, 1000, (B, 20), generator=torch.Generator().manual_seed(9)).to(DEV)
    g = DecodeStepGraph(fq, batch_size=B, max_seq_len=32, dtype=torch.bfloat16, device=DEV)
    caches = fq.create_caches(B, 32, torch.device(DEV), torch.bfloat16, device_pos=True)
    with torch.no_grad():
        lg = g.prefill(ids)
        le = fq(ids, caches, 0)
        assert torch.equal(lg, le)
        for step in range(4):
            tok = le[:, -1].argmax(-1, keepdim=True)
            lg = g.step(tok).clone()
            le = fq(tok, caches, 20 + step)
            assert torch.equal(lg, le), step


def test_ch03_benchmark_gemv_fp8w_runs_the_kernel(pli):
    import ch03
    r = ch03.benchmark_gemv_fp8w(256, 512, dtype=torch.bfloat16, warmup=2, iterations=5)
    assert pli.last_route() == "linear_fp8w_vec"
    assert r.kernel_us is not None and r.kernel_us > 0 and r.kernel_gbps > 0
