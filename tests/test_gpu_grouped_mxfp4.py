"""pli_gemm_grouped_mxfp4 and ch09.Mxfp4MoELayer on the device; the cases, NaN conventions and bounds are DESIGN.md
§3.7b's (Checks).  SwiGLU bound, g and u the float64 sums, b_g and b_u their brackets of (b) of tests/fp8a_cases.py:
NORM_SLACK u |ref| + 1.1 |u| b_g + |silu(g)| b_u + MIN_NORMAL."""
import functools

import numpy as np
import pytest
import torch

import fp8a_cases as fc
from decode_step_cases import HALF_ULP, MIN_NORMAL, NORM_SLACK, TDT, Guarded, assert_untouched
from oracle.numerics import round_to_dtype, seeded_normal
from test_gpu_mx_splitk import exact_data
from test_gpu_mxfp4a import DEV, bits, dev_u8, pack, pli, weight64  # noqa: F401  (pli: the module fixture)

pytestmark = pytest.mark.gpu
MX, GENERIC = "gemm_grouped_mxfp4", "gemm_grouped_mxfp4_generic"
# rows per expert -> rows_bound (the last above the real count): empty expert, each MC, slab crossing, exact slab
ROWSETS = {(0, 1, 33, 130): 164, (17, 0, 96, 128): 241, (300, 0, 5, 0): 320}


def routing(counts, seed):  # offsets, gather (every used token twice, permuted: top-2; the last token unread), tokens
    rows, tokens = sum(counts), sum(counts) // 2 + 3
    pool = np.arange(tokens - 1)
    gather = np.random.RandomState(seed).permutation(np.concatenate([pool, pool]))[:rows].astype(np.int32)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), gather, tokens


def device_operands(pli, x8, xs, gather, offsets, w, wu, pad=False):
    """on the device; unread token rows become NaN codes, experts without rows 0xFF scale bytes; pad: NaN-filled strides"""
    p = (lambda v: v) if pad else (lambda v: 0)
    x8 = x8.copy()
    x8[np.setdiff1d(np.arange(x8.shape[0]), np.arange(offsets[-1]) if gather is None else gather)] = 0x7F
    table = lambda ws: ws and pli.mxfp4_weight_tables(  # noqa: E731
        [(dev_u8(pack(nib), 0xFF, p(48), p(16)), dev_u8(ex if c else np.full_like(ex, 0xFF), 0xFF, p(8), p(4)))
         for (nib, ex), c in zip(ws, np.diff(offsets))])
    put = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return dev_u8(x8, 0x7F, p(16)), put(xs), put(gather), table(w), put(offsets), table(wu)


def run(pli, x8, xs, gather, offsets, w, wu, dt, rows_bound, route=MX, pad=False):
    n, k, rows = w[0][0].shape[0], x8.shape[1], int(offsets[-1])
    x8d, xsd, gd, tab, od, up = device_operands(pli, x8, xs, gather, offsets, w, wu, pad)
    g = Guarded((rows_bound, n), dt, DEV, strides=(n + (8 if pad else 0), 1))
    pli.gemm_grouped_mxfp4(x8d, xsd, gd, tab, od, rows_bound, n, k, up_tables=up, out=g.view, out_dtype=TDT[dt])
    assert pli.last_route() == route
    torch.cuda.synchronize()
    assert_untouched(g, lambda v: v[:rows])
    return g.view[:rows].clone().cpu()


def exact_case(counts, n, k):
    offsets, gather, tokens = routing(counts, 7 * k + n)
    x8, (nib, ex), want = exact_data("mxfp4", tokens, len(counts) * n, k)
    w = [(nib[e * n:(e + 1) * n], ex[e * n:(e + 1) * n]) for e in range(len(counts))]
    expert = np.repeat(np.arange(len(counts)), counts)
    want = np.stack([want[t, e * n:(e + 1) * n] for t, e in zip(gather, expert)])
    return x8, gather, offsets, w, want


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("k", [256, 640])
@pytest.mark.parametrize("counts,use_gather", [(c, True) for c in ROWSETS] + [((0, 1, 33, 130), False)])
def test_plain_form_is_the_f64_result_bitwise(pli, counts, use_gather, k, dt):
    x8, gather, offsets, w, want = exact_case(counts, 144, k)
    if not use_gather:  # the rows already sorted, gather NULL
        x8, gather = x8[gather], None
    got = run(pli, x8, None, gather, offsets, w, None, dt, ROWSETS[counts])
    assert torch.equal(bits(got), bits(torch.from_numpy(want).to(TDT[dt])))


@functools.lru_cache(maxsize=None)
def oracle_case(counts, sw, dt, n=256, k=2048):
    import pli_hip
    offsets, gather, tokens = routing(counts, 11 + sw)
    seed = 61000 + 13 * sum(counts) + 500 * (dt == "fp16") + 1000 * sw
    x = round_to_dtype(seeded_normal((tokens, k), seed) * np.float32(0.5), dt)
    c8, s = pli_hip.quantize_rows_fp8(torch.from_numpy(x).to(TDT[dt]))
    x8, xs = c8.view(torch.uint8).numpy(), s.numpy()

    def weight(sd):
        wf = seeded_normal((n, k), sd) * np.float32(k ** -0.5) * np.exp2(np.arange(n) % 9 - 4.0)[:, None].astype(np.float32)
        codes, ex = (t.numpy() for t in pli_hip.quantize_weight_mxfp4(torch.from_numpy(wf)))
        return np.stack((codes & 15, codes >> 4), axis=2).reshape(n, k), ex

    w, wu = ([weight(seed + 10 + 100 * m + e) for e in range(len(counts))] for m in (0, 1))
    xd = (fc.DECODE[x8] * xs.astype(np.float64)[:, None])[gather]

    def sums(m, f):  # f(x) f(W_e)^T over each expert's rows
        return np.concatenate([f(xd[offsets[e]:offsets[e + 1]]) @ f(weight64(*m[e])).T for e in range(len(counts))])
    ref, bound = sums(w, np.asarray), (k + 2) * 2.0 ** -23 * sums(w, np.abs)
    if sw:
        u, silu = sums(wu, np.asarray), ref / (1 + np.exp(-ref))
        ref, bound = silu * u, 1.1 * np.abs(u) * bound + np.abs(silu) * (k + 2) * 2.0 ** -23 * sums(wu, np.abs)
    return x8, xs, gather, offsets, w, (wu if sw else None), fc.Reference(ref, bound, k)


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("sw", [False, True], ids=["plain", "swiglu"])
@pytest.mark.parametrize("counts,n,k,route", [(c, 256, 2048, MX) for c in ROWSETS] + [((0, 1, 33, 130), 24, 96, GENERIC)])
def test_against_f64_oracle(pli, counts, n, k, route, sw, dt):  # k 96, n 24: outside the route rule, same bounds
    x8, xs, gather, offsets, w, wu, ref = oracle_case(counts, sw, dt, n, k)
    got = run(pli, x8, xs, gather, offsets, w, wu, dt, ROWSETS[counts], route=route, pad=True)
    ra, rb = fc.ratios(got.double().numpy(), ref, dt)  # (b) over ref.bracket: the plain bracket or the SwiGLU one
    print(f"{route} {counts} {'swiglu' if sw else 'plain'} {dt}: err / (a) {ra:.3f}, err / (b) {rb:.3f}")
    assert rb <= 1.0 and (sw or ra <= 1.0), (counts, sw, dt, ra, rb)


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("sw", [False, True], ids=["plain", "swiglu"])
def test_nan_poisons_exactly_its_rows_or_its_column(pli, sw, dt):
    counts, n, k = (0, 1, 33, 130), 144, 640
    x8, gather, offsets, w, _ = exact_case(counts, n, k)
    wu = [(nib[::-1].copy(), ex) for nib, ex in w] if sw else None
    go = lambda x, ws: run(pli, x, None, gather, offsets, ws, wu, dt, ROWSETS[counts])  # noqa: E731
    clean = go(x8, w)
    token = int(gather[40])
    xn = x8.copy()
    xn[token, 3 * 128 + 77] = 0x7F
    wn = [(nib, ex.copy()) for nib, ex in w]
    wn[3][1][130, (2 * 128 + 64) // 32] = 0xFF
    cases = [(go(xn, w), (torch.from_numpy(gather == token), slice(None))), (go(x8, wn), (slice(*offsets[3:5]), 130))]
    if sw:  # a 0xFF byte of the up matrix alone
        wu = [(nib, ex.copy()) for nib, ex in wu]
        wu[2][1][7, 3] = 0xFF
        cases.append((go(x8, w), (slice(*offsets[2:4]), 7)))
    for got, where in cases:
        want_nan = torch.zeros(clean.shape, dtype=torch.bool)
        want_nan[where] = True
        assert int(want_nan.sum()) > 1 and torch.equal(torch.isnan(got), want_nan)
        assert torch.equal(bits(got)[~want_nan], bits(clean)[~want_nan])


def test_graph_replays_after_in_place_changes(pli):
    counts, n, k = (17, 0, 96, 128), 144, 256
    x8, gather, offsets, w, _ = exact_case(counts, n, k)
    x8d, xs, gd, tab, od, _ = device_operands(pli, x8, np.linspace(0.5, 1.5, x8.shape[0], dtype=np.float32), gather, offsets, w, None)
    out = torch.empty(ROWSETS[counts], n, dtype=torch.bfloat16, device=DEV)
    call = lambda o=None: pli.gemm_grouped_mxfp4(x8d, xs, gd, tab, od, ROWSETS[counts], n, k, up_tables=tab, out=o)  # noqa: E731
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
            tab.weights[2][0][11].copy_(torch.roll(tab.weights[2][0][11], 1))
        g.replay()
        torch.cuda.synchronize()
        seen.append(out[:rows].clone())
        assert torch.equal(bits(seen[-1]), bits(call()[:rows]))
    assert pli.last_route() == MX and not torch.equal(bits(seen[0]), bits(seen[1])) and not torch.equal(bits(seen[1]), bits(seen[2]))


def test_layer_on_the_device_meets_its_cpu_mirror():
    """against the torch mirror on the CPU: test 2's bound through W2 and the combine plus one e4m3 flip per sorted row
    (DESIGN.md §3.7b).  x on a 1/64 grid, gate weights in {-1, 0, 1} / 16: exact logits, both sides route alike."""
    from ch09 import MoEConfig, MoELayer, Mxfp4MoELayer
    torch.manual_seed(9)
    H, I, u = 256, 384, HALF_ULP["bf16"]
    layer = MoELayer(MoEConfig(hidden_dim=H, expert_dim=I, num_experts=8, num_experts_per_tok=2)).bfloat16()
    with torch.no_grad():
        layer.router.gate.weight.copy_(torch.randint(-1, 2, layer.router.gate.weight.shape) / 16)
        x = (torch.round(torch.randn(1, 40, H) * 64).clamp(-255, 255) / 64).bfloat16()
        q, trace = Mxfp4MoELayer.from_layer(layer), []
        ref = q._forward_torch(x.view(-1, H), trace).double()
        got = q.to(DEV)(x.to(DEV)).double().cpu().view(-1, H)
    tol = NORM_SLACK * 2 * u * ref.abs() + MIN_NORMAL["bf16"]
    for rows, wk, hq, w2, y in trace:
        hq, w2 = hq.double().abs(), w2.double().abs()
        per_slot = 2 * (I + 2) * 2.0 ** -23 * (hq @ w2.t()) + 2 * u * y.double().abs() + 2.0 ** -3 * (hq[:, None, :] * w2[None]).amax(2)
        tol[rows] += wk.double()[:, None] * per_slot
    err = (got - ref).abs()
    print(f"layer: max err / bound {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())
