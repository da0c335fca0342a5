"""Which kernel each call runs (pli_last_route): the dispatch tables that
DESIGN.md §0 / §3 and include/pli.h state, checked on the device.  Flash:
csrc/flash_plan.h plan_flash -- pp64 (attn_pp64_ok, where its blocks fill the
chip) -> v13 (attn_v13_ok) -> v12 (attn_v12_ok) -> v7 / v10 -> v2, the generic
kernel for what no MFMA kernel reads; the same cases are asked of the planner
on the CPU in tests/test_flash_plan.py.  Each routed call is also checked
against fp32 torch attention, so a route is only "taken" when its result is
right."""
from __future__ import annotations

import pytest
import torch

from flash_route_cases import BF, FLASH, FORCED, forced_id

pytestmark = pytest.mark.gpu
DEV = "cuda"


def flash_case(B, H, Hkv, Nq, Nk, D, dt, causal, want, variant=None, scale=None):
    """one call through the public ABI: its route, and its result against fp32 torch attention"""
    import pli_hip
    g = torch.Generator(device=DEV).manual_seed(Nq + Nk + D)
    # an explicit scale > 0: Q shrunk so the scaled scores spread as at the default D^-1/2 -- a softmax
    # near one-hot would return single V values up to ~4.5, whose 16-bit rounding alone (2^-6) passes 1e-2
    amp = D ** -0.5 / scale if scale is not None and scale > 0 else 1.0
    q = (torch.randn(B, H, Nq, D, device=DEV, generator=g) * amp).to(dt)
    k = torch.randn(B, Hkv, Nk, D, device=DEV, generator=g).to(dt)
    v = torch.randn(B, Hkv, Nk, D, device=DEV, generator=g).to(dt)
    out = pli_hip.flash_attn_fwd(q, k, v, scale=scale, causal=causal, variant=variant)
    assert pli_hip.last_route() == want
    G = H // Hkv
    s = (q.float() @ k.float().repeat_interleave(G, 1).transpose(-1, -2)) * (D ** -0.5 if scale is None else scale)
    if causal:
        s = s.masked_fill(torch.ones(Nq, Nk, dtype=torch.bool, device=DEV).triu(Nk - Nq + 1), float("-inf"))
    ref = torch.softmax(s, -1) @ v.float().repeat_interleave(G, 1) if Nk else torch.zeros_like(q, dtype=torch.float32)
    ref = torch.nan_to_num(ref)  # (causal Nq > Nk: rows with no key are 0 here and NaN in torch)
    assert (out.float() - ref).abs().max().item() <= 1e-2


@pytest.mark.parametrize("case", FLASH, ids=lambda c: "b{}h{}kv{}q{}k{}d{}-{}-causal{}".format(
    *c[:6], str(c[6]).split(".")[-1], int(c[7])))
def test_flash_route(case):
    flash_case(*case)


@pytest.mark.parametrize("case", FORCED, ids=forced_id)
def test_flash_forced_variant(case):
    """every variant number where it applies and where it falls through, c > 1 and scale <= 0"""
    variant, *shape, scale, want = case
    flash_case(*shape, want, variant=variant, scale=scale)


@pytest.mark.parametrize("short", (0, 1), ids=("fills", "one-short"))
def test_flash_fill_rule(short):
    """the default at D 64 non-causal: pp64 where B H ceil(Nq / 512) blocks fill the CUs, else v13"""
    H = torch.cuda.get_device_properties(0).multi_processor_count - short
    flash_case(1, H, H, 64, 128, 64, BF, False, "attn_fwd_v13_d64" if short else "attn_fwd_pp64")


def test_gemm_and_decode_routes():
    import pli_hip
    g = torch.Generator(device=DEV).manual_seed(3)
    a = torch.randn(4096, 4096, device=DEV, generator=g).to(BF)
    b = torch.randn(4096, 4096, device=DEV, generator=g).to(BF)
    pli_hip.gemm(a, b)
    assert pli_hip.last_route() == "gemm_w5"                      # 4096^3 NN: the 256^2 one-wave-per-SIMD tile
    pli_hip.gemm(a[:1], b, trans_b=True)
    assert pli_hip.last_route() == "gemv_vec"                     # M = 1, no bias: the GEMV
    x = torch.randn(8, 4096, device=DEV, generator=g).to(BF)
    pli_hip.gemm(x, b, trans_b=True, bias=b[0])
    assert pli_hip.last_route() in ("gemm_smallm_nt", "gemm_skinny_nt")
    f = torch.randn(2048, 2048, device=DEV, generator=g)
    pli_hip.gemm(f, f)
    assert pli_hip.last_route() == "gemm_f32_mfma"
    pli_hip.gemm(a[:, :0], b[:0])
    assert pli_hip.last_route() == "gemm_generic"                 # K = 0: C = 0
    pli_hip.gemm(a[:0], b)
    assert pli_hip.last_route() == ""                             # empty output: nothing launched
    pli_hip.gemv(a, a[0])
    assert pli_hip.last_route() == "gemv_vec"
    q = torch.randn(8, 1, 32, 128, device=DEV, generator=g).to(BF)
    kc = torch.randn(8, 32768, 8, 128, device=DEV, generator=g).to(BF)
    pli_hip.attn_decode(q, kc, kc, 32768)
    assert pli_hip.last_route() == "attn_decode_chunk+attn_decode_combine"
    pli_hip.attn_decode(q, kc, kc, 0)
    assert pli_hip.last_route() == "attn_fwd_generic"             # empty cache: O = 0


# (M, N, K, trans_b, bias, expected route or prefix): csrc/gemm.hip gemm_dispatch
# through the Python wrapper (which passes a split-K workspace when one is needed)
GEMM = [
    (1, 4096, 4096, True, True, "gemm_skinny_nt"),                          # M = 1 with a bias
    (16, 2048, 2048, True, False, "gemm_smallm_nt"),                        # short K, M <= 32
    (64, 8192, 1024, True, False, "gemm_midm_nt"),                          # the TP-8 row shard at M 64
    (128, 8192, 8192, True, False, "gemm_splitk_lds_nt+gemm_splitk_reduce"),  # decode batch, deep K
    (1024, 4096, 4096, True, False, "gemm_splitk_lds_nt"),                  # few tiles: 128-row slabs
    (384, 384, 256, False, False, "gemm_mfma"),                             # below the 2 x 2 grid of 256^2
    (8192, 8192, 1024, True, False, "gemm_w5"),                             # 1024 tiles
    (4096, 4096, 4096, False, True, "gemm_w5"),                             # NN with a bias
]


@pytest.mark.parametrize("case", GEMM, ids=lambda c: "m{}n{}k{}-nt{}-bias{}".format(*c[:5]))
def test_gemm_route(case):
    import pli_hip
    M, N, K, nt, bias, want = case
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    a = torch.randn(M, K, device=DEV, generator=g).to(BF)
    b = torch.randn(N, K, device=DEV, generator=g).to(BF) if nt else torch.randn(K, N, device=DEV, generator=g).to(BF)
    bi = torch.randn(N, device=DEV, generator=g).to(BF) if bias else None
    c = pli_hip.gemm(a, b, trans_b=nt, bias=bi)
    route = pli_hip.last_route()
    assert route == want or (want.endswith("_nt") and route.startswith(want + "+")), route
    ref = a.float() @ (b.float().t() if nt else b.float()) + (bi.float() if bias else 0)
    scale = ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-3)
    assert ((c.float() - ref).abs() / scale).max().item() <= 2.0 ** -7
