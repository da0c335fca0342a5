"""GPU parity of the fused SwiGLU projection (pli_gemm_swiglu) against the f64
oracle, and of the FFN / TP-MLP modules that use it.

The first tests run production-sized shapes under the project's bound
|err| <= tol * (|ref| + 1) per element (bf16 1e-2, fp16 4e-3, fp32 1e-4 as for
pli_gemm).  The per-element tests below them run the case list of
tests/swiglu_cases.py: every route behind pli_gemm_swiglu -- gemm_skinny_nt
(NB 1 / 2 / 4 / 8 / 16), gemm_smallm_nt (NBG 1 / 2 / 4 / 8), the split-K pair
gemm_splitk_lds_nt (MC 1 / 2 / 3 / 4, ks 1 / 2 / 4 / 8) + reduce, gemm_mfma,
gemm_w5 (forced and default), the phased gemm_256p (variant 4 only: the default
reaches it just where gemm_w5's leading-dimension limits fail) and
gemm_generic (fp32, and 16-bit through n % 8, k % 8, ldx % 8 and a misaligned
pointer) -- at the smallest shapes that reach each instance and its K seams, in
bf16 and fp16, with

* the kernel name asserted against the CPU replay of the dispatch;
* x, the gate and the up weight as views with three different row strides, NaN
  in the padding and in three spare rows after each;
* the output inside a sentinel-filled buffer with guard rows, ldh = n + 8 and
  three spare rows (decode_step_cases.Guarded / assert_untouched);
* two bounds per element, both asserted: (a) the project's, and (b) one output
  rounding + the fp32 evaluation (swiglu_cases' docstring; about 50 times
  tighter than (a) at small K).  The CPU emulation of the semantics
  (tests/test_swiglu_emulation_cpu.py) sits at most at 0.94 of (b), and so do
  the kernels on the MI355X.

Relations: variant 3 (gemm_w5) and 4 (phased tile) bitwise on the phased cases;
the padded and the contiguous operand family bitwise per route; a workspace one
byte short takes the unsplit route and is left alone; an exactly sized one is
not written past its end."""
from __future__ import annotations


import ctypes

import numpy as np
import pytest
import torch

import decode_step_cases as dc
import swiglu_cases as sc
from conftest import load_golden
from oracle.linear import swiglu
from oracle.numerics import seeded_normal

pytestmark = pytest.mark.gpu
TDT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
TOL = {"fp32": 1e-4, "fp16": 4e-3, "bf16": 1e-2}

CASES = [  # m, n, k, dtype -> route
    (1, 4096, 4096, "bf16"),     # skinny, decode batch 1
    (5, 1376, 4096, "bf16"),     # skinny, n % 16 != 0
    (16, 4096, 1024, "fp16"),    # small-M MFMA
    (48, 2048, 512, "bf16"),     # small-M MFMA, NBG = 4
    (128, 1024, 4096, "bf16"),   # small-M MFMA, NBG = 8
    (200, 1000, 768, "bf16"),    # 128x128 tile, ragged m and n
    (1024, 2048, 1024, "fp16"),  # 128x128 tile (64 tiles of 256x128: too few for gemm_w5)
    (2304, 1376, 256, "bf16"),   # gemm_w5<swiglu> (>= 96 tiles of 256x128), ragged n (10.75 column tiles)
    (2100, 1536, 640, "fp16"),   # gemm_w5<swiglu>, ragged m, 10 K-tiles
    (2048, 5632, 2048, "bf16"),  # gemm_w5<swiglu>, Llama-shaped MLP
    (3072, 1024, 64, "bf16"),    # gemm_w5<swiglu>, one K-tile
    (33, 100, 72, "bf16"),       # generic: n % 8 != 0
    (64, 96, 40, "fp32"),        # generic fp32
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "m{}n{}k{}_{}".format(*c))
def test_gemm_swiglu_vs_oracle(case):
    import pli_hip
    m, n, k, dt = case
    x = seeded_normal((m, k), 1, dt) * 0.5
    wg = seeded_normal((n, k), 2, dt) * k ** -0.5
    wu = seeded_normal((n, k), 3, dt) * k ** -0.5
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda().to(TDT[dt])
    h = pli_hip.gemm_swiglu(d(x), d(wg), d(wu))
    ref = swiglu(x, wg, wu)
    got = h.float().cpu().numpy().astype(np.float64)
    bad = np.abs(got - ref) > TOL[dt] * (np.abs(ref) + 1)
    assert not bad.any(), f"{bad.sum()} beyond tol, max err {np.abs(got - ref).max():.3e}"


@pytest.mark.parametrize("split_k", [True, False])
@pytest.mark.parametrize("case", [(32, 1024, 4096, "bf16"), (100, 416, 8192, "bf16"),
                                  (200, 384, 4096, "fp16"), (256, 512, 2048, "bf16"),
                                  (64, 4096, 1024, "bf16")],
                         ids=lambda c: "m{}n{}k{}_{}".format(*c))
def test_gemm_swiglu_decode_batch_split_k(case, split_k):
    """Decode batches 16 < m <= 256: gate and up split-K planes through the
    wrapper's workspace + the silu(g) * u reduce, and the no-workspace routes."""
    import pli_hip
    m, n, k, dt = case
    x = seeded_normal((m, k), 4, dt) * 0.5
    wg = seeded_normal((n, k), 5, dt) * k ** -0.5
    wu = seeded_normal((n, k), 6, dt) * k ** -0.5
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda().to(TDT[dt])
    h = pli_hip.gemm_swiglu(d(x), d(wg), d(wu), split_k=split_k)
    ref = swiglu(x, wg, wu)
    got = h.float().cpu().numpy().astype(np.float64)
    bad = np.abs(got - ref) > TOL[dt] * (np.abs(ref) + 1)
    assert not bad.any(), f"{bad.sum()} beyond tol, max err {np.abs(got - ref).max():.3e}"


@pytest.mark.parametrize("m", [64, 3072])
def test_gemm_swiglu_strided_halves_of_fused_weight(m):
    """FusedSwiGLUFFN passes the two row halves of one [2n, k] weight (m = 3072:
    gemm_w5<swiglu>, 96 tiles), per element."""
    import pli_hip
    n, k = 1024, 256
    x = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(2 * n, k, device="cuda", dtype=torch.bfloat16) * k ** -0.5
    h = pli_hip.gemm_swiglu(x, w[:n], w[n:])
    ref = swiglu(x.float().cpu().numpy(), w[:n].float().cpu().numpy(), w[n:].float().cpu().numpy())
    got = h.float().cpu().numpy().astype(np.float64)
    bad = np.abs(got - ref) > TOL["bf16"] * (np.abs(ref) + 1)
    assert not bad.any(), f"{bad.sum()} beyond tol, max err {np.abs(got - ref).max():.3e}"


@pytest.mark.parametrize("name,seed", [("NaiveFFN", 5), ("SwiGLUFFN", 6), ("FusedSwiGLUFFN", 7)])
def test_ffn_modules_on_gpu_match_reference(name, seed):
    import ch01
    g = load_golden("ffn.npz")
    torch.manual_seed(seed)
    m = getattr(ch01, name)(256, 512).cuda()
    x = torch.from_numpy(seeded_normal((2, 16, 256), 51)).cuda()
    with torch.no_grad():
        np.testing.assert_allclose(m(x).cpu().numpy(), g[name], rtol=1e-3, atol=1e-3)


def test_tp_mlp_on_gpu_matches_reference_and_bf16_tracks():
    from ch09 import TensorParallelConfig, TensorParallelMLP
    g = load_golden("ffn.npz")
    torch.manual_seed(8)
    m = TensorParallelMLP(TensorParallelConfig(world_size=1, rank=0, hidden_dim=256,
                                               intermediate_dim=512))
    x = torch.from_numpy(seeded_normal((2, 16, 256), 51))
    with torch.no_grad():
        np.testing.assert_allclose(m.cuda()(x.cuda()).cpu().numpy(), g["TensorParallelMLP"],
                                   rtol=1e-3, atol=1e-3)
        yb = m.bfloat16()(x.cuda().bfloat16()).float().cpu().numpy()
    rel = np.linalg.norm(yb - g["TensorParallelMLP"]) / np.linalg.norm(g["TensorParallelMLP"])
    assert rel < 2e-2, rel


@pytest.mark.parametrize("m,n,k", [(2048, 5632, 2048), (4096, 1792, 4096), (2100, 1376, 640)])
def test_gemm_swiglu_w5_route_matches_phased(m, n, k):
    """gemm_w5's SwiGLU form (variant 3, the prefill default since round 4)
    against the phased 256 x 128 tile (variant 4): the same MFMA
    chains in k order and the same silu(g) * u in fp32, so bitwise equal;
    and sampled rows against the f64 oracle."""
    import pli_hip
    g = torch.Generator(device="cuda").manual_seed(m + n + k)
    x = torch.randn(m, k, device="cuda", dtype=torch.bfloat16, generator=g)
    wg = torch.randn(n, k, device="cuda", dtype=torch.bfloat16, generator=g) * k ** -0.5
    wu = torch.randn(n, k, device="cuda", dtype=torch.bfloat16, generator=g) * k ** -0.5
    h3 = pli_hip.gemm_swiglu(x, wg, wu, variant=3)
    h4 = pli_hip.gemm_swiglu(x, wg, wu, variant=4)
    assert torch.equal(h3, h4), f"max diff {(h3.float() - h4.float()).abs().max().item():.3e}"
    rows = torch.randperm(m, generator=torch.Generator().manual_seed(5))[:24]
    ref = swiglu(x[rows].float().cpu().numpy(), wg.float().cpu().numpy(), wu.float().cpu().numpy())
    err = np.abs(h3[rows].float().cpu().numpy() - ref) / (np.abs(ref) + 1)
    assert err.max() <= TOL["bf16"], f"max rel err {err.max():.3e}"


# ------------------------------------------------ every route, per element
DEV = "cuda"
PAIRS = [(c, dt) for c in sc.SWIGLU_CASES for dt in c.dts]
CONTIG_PAIRS = [(c, dt) for c in sc.CONTIG_CASES for dt in c.dts]
_pair_id = lambda v: sc.case_id(v) if isinstance(v, tuple) else v  # noqa: E731


def _launch(c, op, dt, padded=True, variant="case"):
    """one pli_hip.gemm_swiglu call on the case's device operands into a Guarded output; returns it with the route
    string pli_last_route reports"""
    import pli_hip
    x, wg, wu, out = sc.device_operands(c, op, dt, DEV, padded)
    ldx, ldwg, ldwu, ldh = sc.leading_dims(c, padded)
    assert (x.stride(0), wg.stride(0), wu.stride(0), out.view.stride(0)) == (ldx, ldwg, ldwu, ldh)
    assert (x.data_ptr() % 16 != 0) == (padded and c.xmode == "off1")
    pli_hip.gemm_swiglu(x, wg, wu, out=out.view[:c.m], split_k=c.split_k,
                        variant=c.variant if variant == "case" else variant)
    route = pli_hip.last_route()
    torch.cuda.synchronize()
    return out, route


def _check(out, c, ref, dt, what):
    """[:m, :n] finite and inside (a) and (b); the spare rows, the row padding and the guards untouched"""
    got = dc.f64(out.view[:c.m])
    nonfinite = int((~np.isfinite(got)).sum())
    assert nonfinite == 0, f"{what}: {nonfinite} non-finite outputs (padding or a spare row was read)"
    ra, rb = sc.ratios(got, ref, dt)
    print(f"{what}: err / (a) {ra:.3f}, err / (b) {rb:.3f}")
    assert ra <= 1.0 and rb <= 1.0, (what, ra, rb, sc.worst(got, ref, dt))
    dc.assert_untouched(out, lambda v: v[:c.m], what=what)


@pytest.mark.parametrize("c,dt", PAIRS, ids=_pair_id)
def test_swiglu_route_per_element(c, dt):
    op, ref = sc.case_reference(c, dt)
    out, route = _launch(c, op, dt)
    assert route == c.route == sc.case_route(c, dt).kernel, (sc.case_id(c), route)
    _check(out, c, ref, dt, f"{sc.case_id(c)} {dt}")


@pytest.mark.parametrize("c,dt", CONTIG_PAIRS, ids=_pair_id)
def test_swiglu_contiguous_operands_match_padded_bitwise(c, dt):
    """ld == k and ldh == n: the same route, the same bounds, and bit for bit the padded family's values"""
    op, ref = sc.case_reference(c, dt)
    out, route = _launch(c, op, dt, padded=False)
    assert route == c.route == sc.case_route(c, dt, padded=False).kernel, (sc.case_id(c), route)
    _check(out, c, ref, dt, f"{sc.case_id(c)} {dt} contiguous")
    padded, _ = _launch(c, op, dt)
    assert torch.equal(out.view[:c.m].view(sc.BITS[dt]), padded.view[:c.m].view(sc.BITS[dt])), sc.case_id(c)


@pytest.mark.parametrize("c,dt", [(c, dt) for c in sc.PHASED_CASES for dt in c.dts], ids=_pair_id)
def test_swiglu_w5_equals_phased_bitwise(c, dt):
    """variant 3 (gemm_w5) and variant 4 (the phased tile): the same MFMA chains in k order and the same fp32
    silu(g) * u, so the same bits -- in fp16 too, whose phased instance no other test launches"""
    op, _ = sc.case_reference(c, dt)
    h4, r4 = _launch(c, op, dt, variant=4)
    h3, r3 = _launch(c, op, dt, variant=3)
    assert (r3, r4) == (sc.W5, sc.P256)
    assert r3 == sc.swiglu_route(c.m, c.n, c.k, dt, 3, 0, lds=sc.leading_dims(c)[:3]).kernel
    assert torch.equal(h3.view[:c.m].view(sc.BITS[dt]), h4.view[:c.m].view(sc.BITS[dt]))


# ---------------------------------------- the workspace, through the C ABI
WS_BYTE = 0xA5
WS_CASES = [c for c in sc.SWIGLU_CASES if (c.m, c.n, c.k, c.kind) in ((65, 32, 1024, "default"),
                                                                       (130, 160, 1024, "default"))]


def _call_ws(c, op, dt, ws_ptr, ws_bytes):
    """pli_gemm_swiglu_ws on the padded operands; returns the Guarded output and the route"""
    import pli_hip
    x, wg, wu, out = sc.device_operands(c, op, dt, DEV)
    rc = pli_hip.lib().pli_gemm_swiglu_ws(x.data_ptr(), wg.data_ptr(), wu.data_ptr(), out.view.data_ptr(), c.m, c.n,
                                          c.k, x.stride(0), wg.stride(0), wu.stride(0), out.view.stride(0),
                                          sc.DTYPE_CODE[dt], ctypes.c_void_p(ws_ptr), ws_bytes,
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0, pli_hip.lib().pli_last_error()
    route = pli_hip.last_route()
    torch.cuda.synchronize()
    return out, route


@pytest.mark.parametrize("c,dt", [(c, dt) for c in WS_CASES for dt in c.dts], ids=_pair_id)
def test_swiglu_workspace_one_byte_short_takes_the_unsplit_route(c, dt):
    import pli_hip
    op, ref = sc.case_reference(c, dt)
    need = pli_hip.lib().pli_gemm_swiglu_workspace_size(c.m, c.n, c.k, sc.DTYPE_CODE[dt])
    assert need == sc.workspace_size(c.m, c.n, c.k, dt) > 0
    ws = torch.full((need,), WS_BYTE, dtype=torch.uint8, device=DEV)
    out, route = _call_ws(c, op, dt, ws.data_ptr(), need - 1)
    unsplit = sc.case_route(c, dt, workspace=need - 1).kernel
    assert route == unsplit and unsplit != sc.SPLIT, (route, unsplit)
    _check(out, c, ref, dt, f"{sc.case_id(c)} {dt} short workspace")
    assert bool((ws == WS_BYTE).all()), "the refused workspace was written"


@pytest.mark.parametrize("c,dt", [(c, dt) for c in WS_CASES for dt in c.dts], ids=_pair_id)
def test_swiglu_workspace_exactly_sized_is_not_overrun(c, dt):
    op, ref = sc.case_reference(c, dt)
    need, guard = sc.workspace_size(c.m, c.n, c.k, dt), 4096
    buf = torch.full((need + 2 * guard,), WS_BYTE, dtype=torch.uint8, device=DEV)
    out, route = _call_ws(c, op, dt, buf.data_ptr() + guard, need)
    assert route == sc.SPLIT == sc.case_route(c, dt, workspace=need).kernel
    _check(out, c, ref, dt, f"{sc.case_id(c)} {dt} exact workspace")
    assert bool((buf[:guard] == WS_BYTE).all()) and bool((buf[guard + need:] == WS_BYTE).all()), \
        "bytes outside the workspace were written"
    planes = buf[guard:guard + need].view(torch.int32)   # 2 ks planes of m x n fp32, every element written
    unwritten = int((planes == int.from_bytes(bytes([WS_BYTE] * 4), "little", signed=True)).sum())
    assert unwritten == 0 and bool(torch.isfinite(planes.view(torch.float32)).all()), unwritten
