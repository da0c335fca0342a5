"""pli_gemm_grouped_mxfp4_a4 and ch09.Mxfp4MoELayer(activations="mxfp4") on the device; the cases, NaN conventions and
bounds are DESIGN.md §3.7d's (Checks), the routing sets and the SwiGLU bracket test_gpu_grouped_mxfp4.py's."""
import functools

import numpy as np
import pytest
import torch

import fp8a_cases as fc
from decode_step_cases import HALF_ULP, MIN_NORMAL, NORM_SLACK, TDT, Guarded, assert_untouched
from oracle.numerics import round_to_dtype, seeded_normal
from test_gpu_grouped_mxfp4 import ROWSETS, routing, device_operands as a8_operands, oracle_case as a8_oracle_case
from test_gpu_mxfp4a4 import DEV, bits, dev_u8, pack, pli, value64  # noqa: F401  (pli: the module fixture)

pytestmark = pytest.mark.gpu
MX, GENERIC = "gemm_grouped_mxfp4_a4", "gemm_grouped_mxfp4_a4_generic"
E2M1_INT = np.array([7 | 8, 5 | 8, 4 | 8, 2 | 8, 0, 2, 4, 5, 7], np.uint8)  # the codes of -6, -3, -2, -1, 0, 1, 2, 3, 6


def run(pli, xnib, xexp, xs, gather, offsets, w, wu, dt, rows_bound, route=MX, pad=False):
    """the W4A8 test's operands with x4 in x8's place (pad: NaN-filled strides), and x_exp: 0xFF in unread token rows"""
    n, k, rows = w[0][0].shape[0], xnib.shape[1], int(offsets[-1])
    xexp = xexp.copy()
    xexp[np.setdiff1d(np.arange(xexp.shape[0]), np.arange(rows) if gather is None else gather)] = 0xFF
    x4, xsd, gd, tab, od, up = a8_operands(pli, pack(xnib), xs, gather, offsets, w, wu, pad)
    g = Guarded((rows_bound, n), dt, DEV, strides=(n + (8 if pad else 0), 1))
    pli.gemm_grouped_mxfp4_a4(x4, dev_u8(xexp, 0xFF, 12 * pad, 8 * pad), xsd, gd, tab, od, rows_bound, n, k, up_tables=up, out=g.view, out_dtype=TDT[dt])
    assert pli.last_route() == route
    torch.cuda.synchronize()
    assert_untouched(g, lambda v: v[:rows])
    return g.view[:rows].clone().cpu()


@functools.lru_cache(maxsize=None)
def exact_case(counts, n, k):
    """small-integer x codes, x_exp per (row, block) over [-4, 4], no row scale (NULL), all 16 weight codes"""
    offsets, gather, tokens = routing(counts, 7 * k + n)
    r, j, i, b = np.arange(tokens)[:, None], np.arange(len(counts) * n)[:, None], np.arange(k)[None, :], np.arange(k // 32)[None, :]
    xnib = E2M1_INT[1:8][(3 * r + 5 * i + (r * i) // 7) % 7]
    xexp = (127 + (r + 2 * b + (r * b) // 3) % 9 - 4).astype(np.uint8)
    wnib = ((7 * j + 2 * i + (j * i) // 5 + 1) % 16).astype(np.uint8)
    wexp = (127 + ((j + 3 * b) % 5 - 2)).astype(np.uint8)
    xd, wd = value64(xnib, xexp), value64(wnib, wexp)
    # every term a multiple of 2^-7 and every partial sum below 2^17: 24 bits; the results inside fp16's range
    assert np.array_equal(np.rint(xd * 16), xd * 16) and np.array_equal(np.rint(wd * 8), wd * 8)
    full = xd @ wd.T + 0.0
    assert float((np.abs(xd) @ np.abs(wd).T).max()) < 2 ** 17 and len(np.unique(xexp)) == 9 and float(np.abs(full).max()) < 65504
    w = [(wnib[e * n:(e + 1) * n], wexp[e * n:(e + 1) * n]) for e in range(len(counts))]
    want = np.stack([full[t, e * n:(e + 1) * n] for t, e in zip(gather, np.repeat(np.arange(len(counts)), counts))])
    return xnib, xexp, gather, offsets, w, want


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("use_gather", [True, False], ids=["gather", "sorted"])
@pytest.mark.parametrize("n,k,route", [(144, 256, MX), (144, 768, MX), (24, 96, GENERIC)])
@pytest.mark.parametrize("counts", list(ROWSETS))
def test_plain_form_is_the_f64_result_bitwise(pli, counts, n, k, route, use_gather, dt):
    xnib, xexp, gather, offsets, w, want = exact_case(counts, n, k)
    if not use_gather:  # the rows already sorted, gather NULL
        xnib, xexp, gather = xnib[gather], xexp[gather], None
    got = run(pli, xnib, xexp, None, gather, offsets, w, None, dt, ROWSETS[counts], route=route)
    assert torch.equal(bits(got), bits(torch.from_numpy(want).to(TDT[dt])))


@functools.lru_cache(maxsize=None)
def oracle_case(counts, sw, dt, k=2048):
    """the W4A8 test's routing and weights (n 256, row magnitudes over 2^+-4; cached there), rows by quantize_rows_mxfp4"""
    import pli_hip
    x8, _, gather, offsets, w, wu, _ = a8_oracle_case(counts, sw, dt)
    seed = 66000 + 13 * sum(counts) + 500 * (dt == "fp16") + 1000 * sw
    x = torch.from_numpy(round_to_dtype(seeded_normal((x8.shape[0], k), seed) * np.float32(0.5), dt)).to(TDT[dt])
    codes, xexp, xs = (t.numpy() for t in pli_hip.quantize_rows_mxfp4(x))
    xnib = np.stack((codes & 15, codes >> 4), axis=2).reshape(codes.shape[0], -1)
    xd = (value64(xnib, xexp) * xs.astype(np.float64)[:, None])[gather]

    def sums(m, f):  # f(x) f(W_e)^T over each expert's rows
        return np.concatenate([f(xd[offsets[e]:offsets[e + 1]]) @ f(value64(*m[e])).T for e in range(len(counts))])
    ref, bound = sums(w, np.asarray), (k + 2) * 2.0 ** -23 * sums(w, np.abs)
    if sw:
        u, silu = sums(wu, np.asarray), ref / (1 + np.exp(-ref))
        ref, bound = silu * u, 1.1 * np.abs(u) * bound + np.abs(silu) * (k + 2) * 2.0 ** -23 * sums(wu, np.abs)
    return xnib, xexp, xs, gather, offsets, w, wu, fc.Reference(ref, bound, k)


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("sw", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("counts", list(ROWSETS))
def test_against_f64_oracle(pli, counts, sw, dt):
    xnib, xexp, xs, gather, offsets, w, wu, ref = oracle_case(counts, sw, dt)
    got = run(pli, xnib, xexp, xs, gather, offsets, w, wu, dt, ROWSETS[counts], pad=True)
    ra, rb = fc.ratios(got.double().numpy(), ref, dt)  # (b) over ref.bracket: the plain bracket or the SwiGLU one
    print(f"{counts} {'swiglu' if sw else 'plain'} {dt}: err / (a) {ra:.3f}, err / (b) {rb:.3f}")
    assert rb <= 1.0 and (sw or ra <= 1.0), (counts, sw, dt, ra, rb)


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("sw", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("n,k,route", [(144, 768, MX), (24, 96, GENERIC)])
def test_nan_poisons_exactly_its_rows_or_its_column(pli, n, k, route, sw, dt):
    counts, (xnib, xexp, gather, offsets, w, _) = (0, 1, 33, 130), exact_case((0, 1, 33, 130), n, k)
    wu = [(nib[::-1].copy(), ex) for nib, ex in w] if sw else None
    go = lambda xe, ws: run(pli, xnib, xe, None, gather, offsets, ws, wu, dt, ROWSETS[counts], route=route)  # noqa: E731
    clean = go(xexp, w)
    token, col = int(gather[40]), n - 14
    xn = xexp.copy()
    xn[token, k // 32 - 2] = 0xFF
    wn = [(nib, ex.copy()) for nib, ex in w]
    wn[3][1][col, 1] = 0xFF
    cases = [(go(xn, w), (torch.from_numpy(gather == token), slice(None))), (go(xexp, wn), (slice(*offsets[3:5]), col))]
    if sw:  # a 0xFF byte of the up matrix alone
        wu = [(nib, ex.copy()) for nib, ex in wu]
        wu[2][1][7, 2] = 0xFF
        cases.append((go(xexp, w), (slice(*offsets[2:4]), 7)))
    for got, where in cases:
        want_nan = torch.zeros(clean.shape, dtype=torch.bool)
        want_nan[where] = True
        assert int(want_nan.sum()) > 1 and torch.equal(torch.isnan(got), want_nan)
        assert torch.equal(bits(got)[~want_nan], bits(clean)[~want_nan])


def test_graph_replays_after_in_place_changes(pli):
    counts, n, k = (17, 0, 96, 128), 144, 768
    xnib, xexp, gather, offsets, w, _ = exact_case(counts, n, k)
    x4, xsd, gd, tab, od, _ = a8_operands(pli, pack(xnib), np.linspace(0.5, 1.5, len(xnib), dtype=np.float32), gather, offsets, w, None)
    xe = dev_u8(xexp, 0xFF)
    out = torch.empty(ROWSETS[counts], n, dtype=torch.bfloat16, device=DEV)
    call = lambda o=None: pli.gemm_grouped_mxfp4_a4(x4, xe, xsd, gd, tab, od, ROWSETS[counts], n, k, up_tables=tab, out=o)  # noqa: E731
    call(out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(out)
    seen, rows = [], int(offsets[-1])
    for change in (False, True, True):  # several replays, each against the eager call on the same operands
        if change:
            od[1:3] += 5  # expert 0 grows, expert 2 shrinks
            gd[9:20].copy_(torch.roll(gd[9:20], 1))
            xe[int(gather[30]), 1] += 1
            tab.weights[2][0][11].copy_(torch.roll(tab.weights[2][0][11], 1))
        g.replay()
        torch.cuda.synchronize()
        seen.append(out[:rows].clone())
        assert torch.equal(bits(seen[-1]), bits(call()[:rows]))
    assert pli.last_route() == MX and not torch.equal(bits(seen[0]), bits(seen[1])) and not torch.equal(bits(seen[1]), bits(seen[2]))


def test_layer_on_the_device_meets_its_cpu_mirror(pli, monkeypatch):
    """the W4A8 layer test with its e4m3 flip replaced by one e2m1 code step of h per element: half the code spacing at
    the block's scale (0.5 / 1 / 2 units below 2 / below 4 / from 4 on), times |w2|"""
    from ch09 import MoEConfig, MoELayer, Mxfp4MoELayer
    torch.manual_seed(9)
    H, I, u = 256, 512, HALF_ULP["bf16"]
    layer = MoELayer(MoEConfig(hidden_dim=H, expert_dim=I, num_experts=8, num_experts_per_tok=2)).bfloat16()
    routes, real = [], pli.gemm_grouped_mxfp4_a4
    monkeypatch.setattr(pli, "gemm_grouped_mxfp4_a4", lambda *a, **kw: (real(*a, **kw), routes.append(pli.last_route()))[0])
    with torch.no_grad():
        layer.router.gate.weight.copy_(torch.randint(-1, 2, layer.router.gate.weight.shape) / 16)  # exact logits:
        x = (torch.round(torch.randn(1, 40, H) * 64).clamp(-255, 255) / 64).bfloat16()  # both sides route alike
        q, trace = Mxfp4MoELayer.from_layer(layer, activations="mxfp4"), []
        ref = q._forward_torch(x.view(-1, H), trace).double()
        got = q.to(DEV)(x.to(DEV)).double().cpu().view(-1, H)
        fp8 = [Mxfp4MoELayer.from_layer(layer, **kw).to(DEV)(x.to(DEV)) for kw in ({}, {"activations": "fp8"})]
    assert routes == [MX, MX] and torch.equal(bits(fp8[0]), bits(fp8[1]))
    tol = NORM_SLACK * 2 * u * ref.abs() + MIN_NORMAL["bf16"]
    for rows, wk, hq, w2, y in trace:
        _, he, hs = pli._quantize_rows_mxfp4_torch(hq.bfloat16())  # hq is exact in bf16: h's row and block scales again
        unit = torch.ldexp(hs.double()[:, None], he.int() - 127).repeat_interleave(32, dim=1)
        hq, w2 = hq.double().abs(), w2.double().abs()
        step = 0.5 * unit * torch.where(hq < 2 * unit, 0.5, torch.where(hq < 4 * unit, 1.0, 2.0))
        per_slot = 2 * (I + 2) * 2.0 ** -23 * (hq @ w2.t()) + 2 * u * y.double().abs() + step @ w2.t()
        tol[rows] += wk.double()[:, None] * per_slot
    err = (got - ref).abs()
    print(f"layer (mxfp4 activations): max err / bound {float((err / tol).max()):.2e}")
    assert bool((err <= tol).all())
