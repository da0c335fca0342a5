"""pli_gemm_grouped_mxfp4_ws (split-K decode route of the grouped W4A8 GEMM, at most 32 sorted rows) and the split_decode
Mxfp4MoELayer on the device; operands, oracle, NaN conventions and bounds are tests/test_gpu_grouped_mxfp4.py's."""
import numpy as np
import pytest
import torch

import fp8a_cases as fc
from decode_step_cases import HALF_ULP, MIN_NORMAL, NORM_SLACK, TDT, Guarded, assert_untouched
from test_gpu_grouped_mxfp4 import MX, device_operands, exact_case, oracle_case
from test_gpu_mxfp4a import DEV, bits, pli  # noqa: F401  (pli: the module fixture)

pytestmark = pytest.mark.gpu  # run(): one call with a sentinel-guarded output and workspace (exact / None / short / misaligned)
SPLIT = "gemm_grouped_mxfp4_splitk+gemm_grouped_mxfp4_splitk_reduce"
# rows per expert -> rows_bound: empty expert and a bound above the count, one full m block, one row each, two experts
ROWSETS = {(0, 1, 2, 5): 11, (32, 0, 0, 0): 32, (1, 1, 1, 1): 4, (3, 0, 29, 0): 32}
FORMS = pytest.mark.parametrize("sw", [False, True], ids=["plain", "swiglu"])
up_of = lambda w: [(nib[::-1].copy(), ex) for nib, ex in w]  # noqa: E731  a second matrix for SwiGLU: the rows in reverse


def run(pli, x8, xs, gather, offsets, w, wu, dt, rows_bound, splits=0, work="exact", route=SPLIT, pad=False):
    n, k, rows = w[0][0].shape[0], x8.shape[1], int(offsets[-1])
    x8d, xsd, gd, tab, od, up = device_operands(pli, x8, xs, gather, offsets, w, wu, pad)
    need = pli.gemm_grouped_mxfp4_workspace_bytes(len(w), rows_bound, n, k, wu is not None, splits)
    assert need > 0 or route == MX
    g = Guarded((rows_bound, n), dt, DEV, strides=(n + (8 if pad else 0), 1))
    wg = Guarded(((need or 1 << 20) // 4 + 4,), "fp32", DEV)
    ws = {"exact": wg.view[:need // 4 or None], None: None, "short": wg.view.view(torch.uint8)[:need - 1], "misaligned": wg.view[1:need // 4 + 1]}[work]
    pli.gemm_grouped_mxfp4(x8d, xsd, gd, tab, od, rows_bound, n, k, up_tables=up, out=g.view, out_dtype=TDT[dt], workspace=ws, splits=splits)
    assert pli.last_route() == route
    torch.cuda.synchronize()
    assert_untouched(g, lambda v: v[:rows])
    assert_untouched(wg, *([lambda v: v[:need // 4]] if route == SPLIT else []), what="workspace")
    return g.view[:rows].clone().cpu()


@pytest.mark.parametrize("dt", fc.DTYPES)
@FORMS
@pytest.mark.parametrize("k,splits", [(256, 2), (640, 2), (640, 5), (2304, 2)])  # even chunks, 3 + 2 steps, one step per chunk, 9 steps: passes of 8 + 1
@pytest.mark.parametrize("counts,use_gather", [(c, True) for c in ROWSETS] + [((0, 1, 2, 5), False)])
def test_split_is_the_f64_result_and_the_plain_call_bitwise(pli, counts, use_gather, k, splits, sw, dt):
    x8, gather, offsets, w, want = exact_case(counts, 144, k)
    x8, gather = (x8, gather) if use_gather else (x8[gather], None)  # or the rows already sorted, gather NULL
    args = (pli, x8, None, gather, offsets, w, up_of(w) if sw else None, dt, ROWSETS[counts])
    got = run(*args, splits=splits)  # every partial sum is exact: the plain call's sums and its epilogue
    assert torch.equal(bits(got), bits(run(*args, work=None, route=MX)))
    assert sw or torch.equal(bits(got), bits(torch.from_numpy(want).to(TDT[dt])))


@pytest.mark.parametrize("dt", fc.DTYPES)
@FORMS
@pytest.mark.parametrize("splits", [0, 3])  # the rule (S = 4, 4 steps each) and 6 + 6 + 4 steps
@pytest.mark.parametrize("counts", ROWSETS)
def test_against_f64_oracle(pli, counts, splits, sw, dt):
    x8, xs, gather, offsets, w, wu, ref = oracle_case(counts, sw, dt)
    got = run(pli, x8, xs, gather, offsets, w, wu, dt, ROWSETS[counts], splits=splits, pad=True)
    ra, rb = fc.ratios(got.double().numpy(), ref, dt)  # (b) over ref.bracket: the plain bracket or the SwiGLU one
    print(f"{SPLIT} {counts} S={splits} {'swiglu' if sw else 'plain'} {dt}: err / (a) {ra:.3f}, err / (b) {rb:.3f}")
    assert rb <= 1.0 and (sw or ra <= 1.0), (counts, splits, sw, dt, ra, rb)


@pytest.mark.parametrize("dt", fc.DTYPES)
@FORMS
def test_nan_poisons_exactly_its_rows_or_its_column(pli, sw, dt):
    counts, n, k = (3, 0, 29, 0), 144, 640
    x8, gather, offsets, w, _ = exact_case(counts, n, k)
    wu = up_of(w) if sw else None
    go = lambda x, ws: run(pli, x, None, gather, offsets, ws, wu, dt, ROWSETS[counts], splits=2)  # noqa: E731
    clean, token, xn, wn = go(x8, w), int(gather[9]), x8.copy(), [(nib, ex.copy()) for nib, ex in w]
    xn[token, 3 * 128 + 77] = 0x7F  # in the second chunk
    wn[2][1][130, (2 * 128 + 64) // 32] = 0xFF
    cases = [(go(xn, w), (torch.from_numpy(gather == token), slice(None))), (go(x8, wn), (slice(*offsets[2:4]), 130))]
    if sw:  # a 0xFF byte of the up matrix alone
        wu = [(nib, ex.copy()) for nib, ex in wu]
        wu[0][1][7, 3] = 0xFF
        cases.append((go(x8, w), (slice(*offsets[0:2]), 7)))
    for got, where in cases:
        want_nan = torch.zeros(clean.shape, dtype=torch.bool)
        want_nan[where] = True
        assert int(want_nan.sum()) > 1 and torch.equal(torch.isnan(got), want_nan)
        assert torch.equal(bits(got)[~want_nan], bits(clean)[~want_nan])


@FORMS
@pytest.mark.parametrize("work,rows_bound,splits", [(None, 11, 2), ("short", 11, 2), ("misaligned", 11, 2), ("exact", 33, 2), ("exact", 11, 1)])
def test_fallbacks_are_the_plain_call(pli, work, rows_bound, splits, sw):
    x8, gather, offsets, w, _ = exact_case((0, 1, 2, 5), 144, 640)
    args = (pli, x8, None, gather, offsets, w, up_of(w) if sw else None, "bf16", rows_bound)
    assert torch.equal(bits(run(*args, splits=splits, work=work, route=MX)), bits(run(*args, work=None, route=MX)))


@FORMS
def test_graph_replays_after_in_place_changes(pli, sw):
    counts, n, k, bound = (0, 1, 2, 5), 144, 640, 11
    x8, gather, offsets, w, _ = exact_case(counts, n, k)
    x8d, xs, gd, tab, od, _ = device_operands(pli, x8, np.linspace(0.5, 1.5, x8.shape[0], dtype=np.float32), gather, offsets, w, None)
    ws = torch.empty(pli.gemm_grouped_mxfp4_workspace_bytes(4, bound, n, k, sw, 2), dtype=torch.uint8, device=DEV)
    out = torch.empty(bound, n, dtype=torch.bfloat16, device=DEV)
    call = lambda o=None: pli.gemm_grouped_mxfp4(x8d, xs, gd, tab, od, bound, n, k, up_tables=tab if sw else None, out=o, workspace=ws, splits=2)  # noqa: E731
    call(out)
    torch.cuda.synchronize()
    g, seen, rows = torch.cuda.CUDAGraph(), [], int(offsets[-1])
    with torch.cuda.graph(g):
        call(out)
    for step in (0, -1, 1):  # expert 1 loses its row to expert 2, then gets it back; each replay against the eager call
        if step:
            od[2] += step
            gd[2:8].copy_(torch.roll(gd[2:8], 1))
            tab.weights[3][0][11].copy_(torch.roll(tab.weights[3][0][11], 1))
        g.replay()
        torch.cuda.synchronize()
        seen.append(out[:rows].clone())
        assert torch.equal(bits(seen[-1]), bits(call()[:rows]))
    assert pli.last_route() == SPLIT and not torch.equal(bits(seen[0]), bits(seen[1])) and not torch.equal(bits(seen[1]), bits(seen[2]))


# test_layer_on_the_device_meets_its_cpu_mirror's bound and exact-logit inputs at 1 and 16 tokens; 40 tokens are above 32 sorted rows
@pytest.mark.parametrize("H,I", [(256, 384), (1024, 1280)])  # below the rule's four steps per chunk: plain calls; S = 2 on both GEMMs
def test_split_decode_layer_meets_its_cpu_mirror(monkeypatch, H, I):
    import pli_hip
    from ch09 import MoEConfig, MoELayer, Mxfp4MoELayer
    torch.manual_seed(9)
    u, routes, real = HALF_ULP["bf16"], [], pli_hip.gemm_grouped_mxfp4
    monkeypatch.setattr(pli_hip, "gemm_grouped_mxfp4", lambda *a, **kw: (real(*a, **kw), routes.append(pli_hip.last_route()))[0])
    layer = MoELayer(MoEConfig(hidden_dim=H, expert_dim=I, num_experts=8, num_experts_per_tok=2)).bfloat16()
    with torch.no_grad():
        layer.router.gate.weight.copy_(torch.randint(-1, 2, layer.router.gate.weight.shape) / 16)
        q, plain = Mxfp4MoELayer.from_layer(layer, split_decode=True), Mxfp4MoELayer.from_layer(layer)
        xs, traces = [(torch.round(torch.randn(1, T, H) * 64).clamp(-255, 255) / 64).bfloat16() for T in (1, 16, 40)], [[], []]
        refs = [q._forward_torch(x.view(-1, H), t).double() for x, t in zip(xs, traces)]
        q, plain = q.to(DEV), plain.to(DEV)
        gots = [q(x.to(DEV)).double().cpu().view(-1, H) for x in xs[:2]]
        assert routes == [SPLIT if H == 1024 else MX] * 4  # W1/W3 and W2 of both decode batches
        assert torch.equal(bits(q(xs[2].to(DEV))), bits(plain(xs[2].to(DEV)))) and routes[4:] == [MX] * 4
    for got, ref, trace in zip(gots, refs, traces):
        tol = NORM_SLACK * 2 * u * ref.abs() + MIN_NORMAL["bf16"]
        for rows, wk, hq, w2, y in trace:
            hq, w2 = hq.double().abs(), w2.double().abs()
            per_slot = 2 * (I + 2) * 2.0 ** -23 * (hq @ w2.t()) + 2 * u * y.double().abs() + 2.0 ** -3 * (hq[:, None, :] * w2[None]).amax(2)
            tol[rows] += wk.double()[:, None] * per_slot
        err = (got - ref).abs()
        print(f"split_decode layer H {H}, {ref.shape[0]} tokens: max err / bound {float((err / tol).max()):.3f}")
        assert bool((err <= tol).all())
