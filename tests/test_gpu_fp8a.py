"""fp8 activations (pli_quantize_rows_fp8 / pli_gemm_fp8, Fp8WeightModel(fp8_activations=True)) on the device.

Case list, oracle and the two bounds: tests/fp8a_cases.py.  Outputs sit inside sentinel-filled buffers, padded
leading dimensions hold NaN (codes 0x7F) in the padding, pli_last_route is asserted in each case.

1. the lane map of the scaled MFMA, its scale byte and its subnormals, bit for bit on data whose every partial sum
   is exact; the same data through gemm_fp8_generic, bit for bit
2. the quantiser: bitwise pli_hip.quantize_weight_fp8 on finite rows, the non-finite rule, row independence
3. the GEMM against the float64 oracle over the dequantised operands, per element, bounds (a) and (b)
4. repeatability, graph capture;  5. linear_fp8a is the two calls;  6. the model option

Model bound (test 6): the teacher-forced prefill logits of the device model against the model's own CPU mirror, as
rel. L2, must stay within four times the mirror's own floor: the mirror against itself with float64 intermediates
(no rounding to bf16 between the operations; rows quantised from the float64 values, so code flips at rounding
boundaries are in it).  Both figures are printed by the test and recorded in DESIGN.md 3.3c.  One wrong tile of one
linear moves the logits by order 1.
"""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

import fp8a_cases as fc
from decode_step_cases import SENTINEL, TDT, Guarded, assert_untouched
from oracle.numerics import seeded_normal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD_CODE = 0x7F   # NaN: a padding byte that is read poisons the output
GUARD_CODE = 0x55


@pytest.fixture(scope="module")
def pli(built_lib):
    import pli_hip
    return pli_hip


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16).cpu()


def dev_codes(a: np.ndarray, ld: int | None = None, col0: int = 0, off1: bool = False) -> torch.Tensor:
    """codes [rows, k] on the device: contiguous, a column slice of a [rows, ld] matrix of NaN codes, or a view that
    starts one byte into its buffer"""
    rows, k = a.shape
    t = torch.from_numpy(np.array(a))
    if off1:
        buf = torch.full((rows * k + 1,), PAD_CODE, dtype=torch.uint8, device=DEV)
        buf[1:] = t.reshape(-1).to(DEV)
        return buf[1:].view(rows, k)
    if ld is None:
        return t.to(DEV)
    wide = torch.full((rows, ld), PAD_CODE, dtype=torch.uint8)
    wide[:, col0:col0 + k] = t
    return wide.to(DEV)[:, col0:col0 + k]


def dev_f32(a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)


# ---- 1. lane map and exactness -------------------------------------------------------------------
def _both_routes(pli, x8, xs, w8, ws, dt):
    """the call on gemm_fp8_mx and, through a w8 view one byte into its buffer, on gemm_fp8_generic"""
    m, n = x8.shape[0], w8.shape[0]
    out = []
    for off1, kernel in ((False, fc.MX), (True, fc.GENERIC)):
        g = Guarded((m, n), dt, DEV)
        pli.gemm_fp8(dev_codes(x8), dev_f32(xs), dev_codes(w8, off1=off1), dev_f32(ws), out_dtype=TDT[dt], out=g.view)
        assert pli.last_route() == kernel
        torch.cuda.synchronize()
        assert_untouched(g, lambda v: v)
        out.append(g.view.clone())
    return out


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("k", [fc.KSTEP, 2 * fc.KSTEP])
def test_lane_map_all_code_pairs_bitwise(pli, k, dt):
    """x8 row r = code r, w8 row j = code j in every column: C[r, j] = k * decode(r) * decode(j) * scales, every
    partial sum a multiple of one exact product with a count <= 256, so exact in fp32 in any order.  Power-of-two
    scales that differ between neighbouring rows keep the largest result (k * 448^2 * 2^-12) finite in fp16."""
    x8, w8 = fc.const_rows_codes(k)
    xs = np.exp2(-6.0 - (np.arange(256) % 3)).astype(np.float32)
    ws = np.exp2(-6.0 - (np.arange(256) % 2)).astype(np.float32)
    # + 0.0: the sum starts from +0, so a sum of -0 products (a zero code times a negative one) is +0, not -0
    want64 = k * np.outer(fc.DECODE * xs, fc.DECODE * ws) + 0.0
    want = torch.from_numpy(want64).to(TDT[dt])
    nan = np.isnan(fc.DECODE)
    finite64 = want64[~nan][:, ~nan]
    assert np.array_equal(finite64.astype(np.float32).astype(np.float64), finite64), "exact in fp32: one rounding to T"
    want_nan = torch.from_numpy(nan[:, None] | nan[None, :])
    assert int(nan.sum()) == 2
    got_mx, got_gen = _both_routes(pli, x8, xs, w8, ws, dt)
    for got, what in ((got_mx, "mx"), (got_gen, "generic")):
        g = got.cpu()
        assert torch.equal(torch.isnan(g), want_nan), f"{what}: a NaN code must poison exactly its row / column"
        diff = (bits(g) != bits(want)) & ~want_nan
        assert int(diff.sum()) == 0, (what, int(diff.sum()), diff.nonzero()[:8].tolist())


@pytest.mark.parametrize("dt", fc.DTYPES)
def test_lane_map_asymmetric_pattern_bitwise(pli, dt):
    """distinct small-integer patterns in (row, k) and (col, k), ragged in m and n: catches a row <-> column swap or a
    k permutation of one operand, which constant rows cannot"""
    m, n, k = fc.TM + 3, fc.TN + fc.STORE_N, 2 * fc.KSTEP
    x8, w8, xv, wv = fc.asymmetric_codes(m, n, k)
    xs = np.full(m, 0.25, np.float32)
    want = torch.from_numpy(0.25 * (xv @ wv.T)).to(TDT[dt])
    assert not torch.equal(want[:n, :n], want[:n, :n].t())
    got_mx, got_gen = _both_routes(pli, x8, xs, w8, None, dt)
    assert torch.equal(bits(got_mx), bits(want)), int((bits(got_mx) != bits(want)).sum())
    assert torch.equal(bits(got_gen), bits(want))
    assert torch.equal(bits(got_mx), bits(got_gen))


# ---- 2. quantiser --------------------------------------------------------------------------------
def _quantize_padded(pli, x: torch.Tensor, pad: bool):
    """quantize_rows_fp8 of x (CPU, T) on the device; pad: ldx = k + 8 with NaN in the padding, codes inside a
    [m + 1, k + 16] buffer of guard bytes, the scale inside a guarded buffer.  Returns (codes u8, scale) on the CPU"""
    m, k = x.shape
    if not pad:
        codes, scale = pli.quantize_rows_fp8(x.to(DEV))
        assert pli.last_route() == fc.QUANT
        return codes.view(torch.uint8).cpu(), scale.cpu()
    xw = torch.full((m, k + 8), float("nan"), dtype=x.dtype)
    xw[:, :k] = x
    whole = torch.full((m + 1, k + 16), GUARD_CODE, dtype=torch.uint8, device=DEV)
    sc = torch.full((m + 16,), SENTINEL, dtype=torch.float32, device=DEV)
    pli.quantize_rows_fp8(xw.to(DEV)[:, :k], out=(whole[:m, :k], sc[8:8 + m]))
    assert pli.last_route() == fc.QUANT
    w, s = whole.cpu(), sc.cpu()
    assert bool((w[m:] == GUARD_CODE).all()) and bool((w[:, k:] == GUARD_CODE).all()), "codes outside [m, k] written"
    assert bool((s[:8] == SENTINEL).all()) and bool((s[8 + m:] == SENTINEL).all()), "scales outside [m] written"
    return w[:m, :k].clone(), s[8:8 + m].clone()


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("k", fc.QUANT_KS)
@pytest.mark.parametrize("m", fc.QUANT_MS)
def test_quantiser_is_quantize_weight_fp8_bitwise(pli, m, k, dt):
    x = torch.from_numpy(seeded_normal((m, k), 41000 + 3 * m + k, dt)).to(TDT[dt])
    want_codes, want_scale = pli.quantize_weight_fp8(x)
    for pad in (False, True):
        codes, scale = _quantize_padded(pli, x, pad)
        assert torch.equal(scale.view(torch.int32), want_scale.view(torch.int32)), (pad, "scales")
        assert torch.equal(codes, want_codes.view(torch.uint8)), (pad, int((codes != want_codes.view(torch.uint8)).sum()))


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("k", [24, 130])  # the vector class and the scalar one
def test_quantiser_zero_rows_non_finite_elements_and_row_independence(pli, k, dt):
    tdt = TDT[dt]
    x = torch.from_numpy(seeded_normal((5, k), 42000 + k, dt)).to(tdt)
    x[1] = 0.0
    x[2, 3], x[2, 7], x[2, 11] = float("nan"), float("inf"), float("-inf")
    x[3, 0] = -float("nan")
    x[4] = float("inf")          # no finite element: scale 1.0
    x[4, 5] = float("nan")
    codes, scale = _quantize_padded(pli, x, pad=False)
    want_codes, want_scale = pli.quantize_rows_fp8(x)   # the CPU path: the same rule in torch ops
    assert torch.equal(codes, want_codes.view(torch.uint8)) and torch.equal(scale, want_scale)
    # the rule, element by element
    assert float(scale[1]) == 1.0 and bool((codes[1] == 0).all())
    finite = x[2].float()[torch.isfinite(x[2].float())]
    assert float(scale[2]) == float(finite.abs().max() / 448.0)
    assert int(codes[2, 3]) == 0x7F and int(codes[2, 7]) == 0x7E and int(codes[2, 11]) == 0xFE
    keep = [i for i in range(k) if i not in (3, 7, 11)]
    xr = x[2:3, keep]
    assert torch.equal(codes[2, keep], pli.quantize_weight_fp8(xr)[0].view(torch.uint8)[0])
    assert int(codes[3, 0]) == 0x7F, "a NaN of either sign gets 0x7F"
    assert float(scale[4]) == 1.0 and int(codes[4, 5]) == 0x7F and bool((codes[4, :5] == 0x7E).all())
    # rows are independent: another row 0 changes only row 0's codes and scale
    y = x.clone()
    y[0] = y[0] * 3 + 1
    codes2, scale2 = _quantize_padded(pli, y, pad=False)
    assert torch.equal(codes2[1:], codes[1:]) and torch.equal(scale2[1:], scale[1:])
    assert not torch.equal(codes2[0], codes[0]) and float(scale2[0]) != float(scale[0])


def test_quantiser_empty_shapes(pli):
    codes, scale = pli.quantize_rows_fp8(torch.zeros(3, 0, dtype=torch.bfloat16, device=DEV))
    assert tuple(codes.shape) == (3, 0) and torch.equal(scale.cpu(), torch.ones(3))
    codes, scale = pli.quantize_rows_fp8(torch.zeros(0, 64, dtype=torch.float16, device=DEV))
    assert tuple(codes.shape) == (0, 64) and tuple(scale.shape) == (0,)


# ---- 3. the GEMM against the float64 oracle ------------------------------------------------------
def _launch(pli, c: fc.Case, op: fc.Operands, dt: str):
    ldx8, ldw, ldc = fc.leading_dims(c)
    pad = c.mode == "pad"
    x8 = dev_codes(op.x8, ldx8 if pad else None)
    w8 = dev_codes(op.w8, ldw if pad else None, col0=16 if pad else 0, off1=c.mode == "off1")
    assert (x8.stride(0), w8.stride(0)) == (ldx8, ldw)
    bias = None
    if op.bias is not None:
        bias = torch.from_numpy(np.array(op.bias)).to(TDT[dt]).to(DEV)
    g = Guarded((c.m, c.n), dt, DEV, strides=(ldc, 1))
    pli.gemm_fp8(x8, dev_f32(op.xs), w8, dev_f32(op.ws), bias=bias, out_dtype=TDT[dt], out=g.view)
    route = pli.last_route()
    torch.cuda.synchronize()
    return g, route


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("case", fc.GEMM_CASES, ids=fc.case_id)
def test_gemm_against_f64_oracle(pli, case, dt):
    op, ref = fc.case_reference(case, dt)
    g, route = _launch(pli, case, op, dt)
    assert route == case.kernel
    assert_untouched(g, lambda v: v, what=fc.case_id(case))
    ra, rb = fc.ratios(g.view.double().cpu().numpy(), ref, dt)
    print(f"{fc.case_id(case)} {dt} {route}: err / (a) {ra:.3f}, err / (b) {rb:.3f}")
    assert ra <= 1.0 and rb <= 1.0, (fc.case_id(case), dt, ra, rb)


def test_gemm_k0_and_empty(pli):
    x8 = torch.zeros(19, 0, dtype=torch.uint8, device=DEV)
    w8 = torch.zeros(8, 0, dtype=torch.uint8, device=DEV)
    bias = torch.arange(8, dtype=torch.bfloat16, device=DEV)
    out = torch.full((19, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    pli.gemm_fp8(x8, None, w8, None, out=out)
    assert pli.last_route() == fc.GENERIC and bool((out == 0).all())
    pli.gemm_fp8(x8, None, w8, None, bias=bias, out=out)
    assert torch.equal(out, bias.expand(19, 8))
    assert tuple(pli.gemm_fp8(x8[:0], None, w8, None).shape) == (0, 8) and pli.last_route() == ""


# ---- 4. repeatability and capture ----------------------------------------------------------------
def test_repeatable_and_graph_replays_after_in_place_changes(pli):
    m, n, k = fc.TM + 1, fc.TN + fc.STORE_N, fc.KSTEP * (fc.STAGES + 1)
    tdt = torch.bfloat16
    x = torch.from_numpy(seeded_normal((m, k), 43000, "bf16")).to(tdt).to(DEV)
    w8, ws = pli.quantize_weight_fp8(torch.from_numpy(seeded_normal((n, k), 43001, "fp32")).to(DEV))
    w8, ws = w8.clone(), ws.clone()
    x8 = torch.empty(m, k, dtype=torch.float8_e4m3fn, device=DEV)
    xs = torch.empty(m, dtype=torch.float32, device=DEV)
    out = torch.empty(m, n, dtype=tdt, device=DEV)

    def step():
        pli.quantize_rows_fp8(x, out=(x8, xs))
        pli.gemm_fp8(x8, xs, w8, ws, out_dtype=tdt, out=out)

    step()
    assert pli.last_route() == fc.MX
    first = out.clone()
    step()
    assert torch.equal(bits(first), bits(out)), "two runs differ"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    # x, the weight codes and w_scale change in place, then the replay
    x.copy_(torch.from_numpy(seeded_normal((m, k), 43002, "bf16")).to(tdt))
    w8.view(torch.uint8).copy_(torch.flip(w8.view(torch.uint8), dims=[0]))
    ws.mul_(0.5)
    g.replay()
    torch.cuda.synchronize()
    got = out.clone()
    assert not torch.equal(bits(got), bits(first))
    want = pli.gemm_fp8(*pli.quantize_rows_fp8(x), w8, ws, out_dtype=tdt)
    assert torch.equal(bits(got), bits(want))
    c8, cs = pli.quantize_rows_fp8(x.cpu())
    op = fc.Operands(c8.view(torch.uint8).numpy(), cs.numpy(), w8.view(torch.uint8).cpu().numpy(), ws.cpu().numpy(), None)
    ra, rb = fc.ratios(got.double().cpu().numpy(), fc.reference(op), "bf16")
    assert ra <= 1.0 and rb <= 1.0, (ra, rb)


# ---- 5. linear_fp8a is the two calls -------------------------------------------------------------
@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("m,n,k,kernel", [(fc.TM + 1, fc.TN, 2 * fc.KSTEP, fc.MX), (fc.MIN_M, 24, 40, fc.GENERIC)])
def test_linear_fp8a_is_quantise_then_gemm(pli, m, n, k, kernel, dt):
    tdt = TDT[dt]
    x = torch.from_numpy(seeded_normal((m, k), 44000 + k, dt)).to(tdt).to(DEV)
    w8, ws = pli.quantize_weight_fp8(torch.from_numpy(seeded_normal((n, k), 44001 + k, "fp32")).to(DEV))
    bias = torch.from_numpy(seeded_normal((n,), 44002, dt)).to(tdt).to(DEV)
    got = pli.linear_fp8a(x, w8, ws, bias=bias)
    assert pli.last_route() == kernel and got.dtype == tdt
    x8, xs = pli.quantize_rows_fp8(x)
    assert torch.equal(bits(got), bits(pli.gemm_fp8(x8, xs, w8, ws, bias=bias, out_dtype=tdt)))


# ---- 6. model ------------------------------------------------------------------------------------
def rel(a, b) -> float:
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


@pytest.fixture(scope="module")
def models(pli):
    """the small model of test_gpu_fp8w.py: (device W8A8 model, device W8A16 model, CPU W8A8 mirror), all three with
    the codes and scales quantised once on the CPU"""
    from ch02 import CachedTransformerModel, Fp8WeightModel
    torch.manual_seed(21)
    base = CachedTransformerModel(1000, 256, 2, 4, 2, 512).to(torch.bfloat16).eval()
    mirror = Fp8WeightModel.from_model(base).with_fp8_activations()
    on_dev = copy.deepcopy(base).to(DEV)
    fa = Fp8WeightModel.from_model(on_dev).with_fp8_activations()
    fw = Fp8WeightModel.from_model(on_dev)
    for dev_model in (fa, fw):
        for lin, src in zip(dev_model.linears(), mirror.linears()):
            lin.codes, lin.scale = src.codes.to(DEV), src.scale.to(DEV)
    return fa, fw, mirror


class RouteLog:
    """the route of every linear call the model makes"""

    NAMES = ("gemm_fp8", "linear_fp8w", "linear_swiglu_fp8w")

    def __init__(self, pli, monkeypatch):
        self.routes = []
        for name in self.NAMES:
            monkeypatch.setattr(pli, name, self._wrap(pli, getattr(pli, name)))

    def _wrap(self, pli, fn):
        def call(*a, **kw):
            r = fn(*a, **kw)
            self.routes.append(pli.last_route())
            return r
        return call


def mirror_f64(fq, ids: torch.Tensor) -> torch.Tensor:
    """the CPU mirror's prefill with float64 intermediates: nothing is rounded to bf16 between the operations, the
    rows of every linear are quantised from the float64 values by the same rule"""
    import pli_hip
    from ch02.kv_cache import attend_cached

    def lin(x, layer):
        x2 = x.reshape(-1, x.shape[-1])
        x8, xs = pli_hip._quantize_rows_fp8_torch(x2)
        acc = x8.double() @ layer.codes.double().t()
        return (acc * (xs.double()[:, None] * layer.scale.double()[None, :])).view(*x.shape[:-1], -1)

    def rms(x, norm):
        return x / torch.sqrt(torch.mean(x ** 2, dim=-1, keepdim=True) + norm.eps) * norm.weight.double()

    x = fq.embed(ids).double()
    B, S, _ = x.shape
    for b in fq.layers:
        nq, nk = b.num_heads * b.head_dim, b.num_kv_heads * b.head_dim
        qkv = lin(rms(x, b.input_norm), b.qkv)
        q = qkv[..., :nq].reshape(B, S, b.num_heads, b.head_dim)
        k = qkv[..., nq:nq + nk].reshape(B, S, b.num_kv_heads, b.head_dim)
        v = qkv[..., nq + nk:].reshape(B, S, b.num_kv_heads, b.head_dim)
        h = x + lin(attend_cached(q, k, v, S).reshape(B, S, -1), b.o_proj)
        n2 = rms(h, b.post_attn_norm)
        x = h + lin(torch.nn.functional.silu(lin(n2, b.gate)) * lin(n2, b.up), b.down)
    return lin(rms(x, fq.norm), fq.lm_head)


def test_model_prefill_routes_and_logits(pli, models, monkeypatch):
    fa, fw, mirror = models
    B, S = 2, 20
    ids = torch.randint(0, 1000, (B, S), generator=torch.Generator().manual_seed(7))
    log = RouteLog(pli, monkeypatch)
    with torch.no_grad():
        got = fa(ids.to(DEV), fa.create_caches(B, 32, torch.device(DEV), torch.bfloat16), 0)
        on_routes, log.routes = log.routes, []
        fw(ids.to(DEV), fw.create_caches(B, 32, torch.device(DEV), torch.bfloat16), 0)
        off_routes = log.routes
        want = mirror(ids)
        want64 = mirror_f64(mirror, ids)
    # every linear of the 40-row prefill: qkv, o, gate, up, down per layer, then lm_head
    assert on_routes == [fc.MX] * (5 * len(fa.layers) + 1), on_routes
    assert len(off_routes) == 4 * len(fw.layers) + 1 and not any("gemm_fp8" in r for r in off_routes), off_routes
    floor, err = rel(want, want64), rel(got, want)
    print(f"prefill logits rel. L2: mirror against its float64 form {floor:.3e}, device against the mirror {err:.3e}")
    assert floor > 0 and err <= 4 * floor, (err, floor)


def test_model_decode_steps_stay_on_w8a16_bitwise(pli, models, monkeypatch):
    fa, fw, _ = models
    B, S = 2, 20
    ids = torch.randint(0, 1000, (B, S), generator=torch.Generator().manual_seed(8)).to(DEV)
    with torch.no_grad():
        ca = fa.create_caches(B, 32, torch.device(DEV), torch.bfloat16)
        cb = fw.create_caches(B, 32, torch.device(DEV), torch.bfloat16)
        la = fa(ids, ca, 0)
        for a, b in zip(ca, cb):  # the same cache contents for the W8A16 model
            b.k.copy_(a.k)
            b.v.copy_(a.v)
            b.seq_len = a.seq_len
        log = RouteLog(pli, monkeypatch)
        for step in range(3):
            tok = la[:, -1].argmax(-1, keepdim=True)
            la, lb = fa(tok, ca, S + step), fw(tok, cb, S + step)
            assert torch.equal(bits(la), bits(lb)), step
        assert log.routes and not any("gemm_fp8" in r for r in log.routes), log.routes
