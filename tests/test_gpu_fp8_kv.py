"""GPU tests of the 1-byte (fp8 e4m3fn) paged KV cache: the quantising appends
(pli_kv_append_paged_fp8 / pli_kv_append_varlen_paged_fp8), decode and packed
attention over fp8 pools (pli_attn_decode_paged_fp8 / pli_attn_varlen_paged_fp8)
and ch07.PagedKVCache(kv_dtype=torch.float8_e4m3fn).

Oracle of the attention calls: the codes are made on the host (torch's cast
behind a clamp, tests/fp8_cases.py), dequantised exactly (code value times the
fp32 scale, in float64) and oracle.attention.naive_attention runs in float64 per
sequence.  The kernels widen each code exactly to q's type, so their result is
attention over that dequantised pool with the arithmetic of the 16-bit kernels,
and the tolerance is the project's own (tests/test_gpu_paged.py): 1e-2 for bf16 /
fp16 outputs, 1e-3 for fp32.

Layout as in tests/test_gpu_paged.py: two-layer 5-D pools attended over layer 1,
a randomly permuted table over a pool with spare pages.  Every byte no sequence
owns (spare pages, last-page tails, the other layer, and through a spare page
every unused table entry) is code 0x7E = 448, the largest value the format has.
The scales are per head, distinct and not powers of two; the values are
seeded_normal / scale before quantisation.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np
import pytest
import torch

import paged_cases
import varlen_cases
from fp8_cases import FP8, build_checker, codec_codes, decode_table, dequantise, edge_values, quantise, spacing_of, torch_codes
from oracle import attention as oatt
from oracle.numerics import seeded_normal

pytestmark = pytest.mark.gpu
TDT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
TOL = {"fp32": 1e-3, "fp16": 1e-2, "bf16": 1e-2}
POISON = 0x7E
LAYERS, LAYER = 2, 1
EXTRA, SENTINEL = 3, 77.0
DECODE_ROUTE = {paged_cases.FAST: "attn_decode_paged_fp8",
                paged_cases.COMBINE: "attn_decode_paged_fp8+attn_decode_paged_combine",
                paged_cases.GENERIC: "attn_decode_paged_generic_fp8"}
VARLEN_ROUTE = {varlen_cases.FAST: "attn_varlen_paged_fp8", varlen_cases.GENERIC: "attn_varlen_paged_generic_fp8"}


def scales_of(Hkv: int):
    """per-head scales, distinct, none a power of two"""
    return (torch.linspace(0.37, 1.9, Hkv + 1)[:Hkv].contiguous(), torch.linspace(1.7, 0.53, Hkv + 1)[:Hkv].contiguous())


def lay_out(bs, Hkv, D, kv_lens, max_blocks, seed, spare=5):
    """uint8 5-D pools of host-quantised codes, the permuted table, the scales and the dequantised float64 K / V
    [B, longest, Hkv, D] of every sequence"""
    rng = np.random.default_rng(seed)
    B = len(kv_lens)
    owned = [-(-n // bs) for n in kv_lens]
    nb = sum(owned) + spare
    order = rng.permutation(nb)
    table = np.full((B, max_blocks), order[sum(owned)], dtype=np.int32)  # unused entries: a page nobody owns
    kpool = np.full((nb, LAYERS, bs, Hkv, D), POISON, dtype=np.uint8)
    vpool = np.full((nb, LAYERS, bs, Hkv, D), POISON, dtype=np.uint8)
    longest = max(max(kv_lens), 1)
    ksc, vsc = scales_of(Hkv)
    kc = quantise(torch.from_numpy(seeded_normal((B, longest, Hkv, D), seed + 1)), ksc)
    vc = quantise(torch.from_numpy(seeded_normal((B, longest, Hkv, D), seed + 2)), vsc)
    at = 0
    for b, n in enumerate(kv_lens):
        pages = order[at:at + owned[b]]
        at += owned[b]
        table[b, :owned[b]] = pages
        for i, p in enumerate(pages):
            rows = slice(i * bs, min((i + 1) * bs, n))
            kpool[p, LAYER, :rows.stop - rows.start] = kc[b, rows].numpy()
            vpool[p, LAYER, :rows.stop - rows.start] = vc[b, rows].numpy()
    return dict(kpool=kpool, vpool=vpool, table=table, ksc=ksc, vsc=vsc, kd=dequantise(kc, ksc), vd=dequantise(vc, vsc))


def freeze(h):
    for a in h.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return h


def on_gpu(h, view=FP8):
    """the layer views of the pools (as float8_e4m3fn or uint8 tensors), the table and the scales on the device"""
    pool = lambda a: torch.from_numpy(np.array(a)).cuda().view(view)  # noqa: E731 (a copy: the shared arrays are read-only)
    return (pool(h["kpool"])[:, LAYER], pool(h["vpool"])[:, LAYER], torch.from_numpy(np.array(h["table"])).cuda(),
            h["ksc"].cuda(), h["vsc"].cuda())


# ------------------------------------------------------------------ decode --
@functools.lru_cache(maxsize=None)
def prepared_decode(name: str):
    """a decode case's fp8 layout and reference, computed once and shared (treated as read-only)"""
    c = paged_cases.CASES[name]
    seed = zlib.crc32(("fp8" + name).encode()) % 1000
    h = lay_out(c.bs, c.Hkv, c.D, c.lens, c.max_blocks, seed)
    h["q"] = seeded_normal((c.B, c.Sq, c.H, c.D), seed, c.dt)
    ref = np.zeros((c.B, c.Sq, c.H, c.D))
    for b, n in enumerate(c.lens):
        if n > 0:
            ref[b] = oatt.naive_attention(h["q"][b:b + 1].transpose(0, 2, 1, 3), h["kd"][b:b + 1, :n].transpose(0, 2, 1, 3),
                                          h["vd"][b:b + 1, :n].transpose(0, 2, 1, 3), causal=True)[0].transpose(1, 0, 2)
    h["ref"] = ref
    return freeze(h)


def run_decode(c, h, q_dtype=None, scales=True, view=FP8):
    import pli_hip
    kp, vp, table, ksc, vsc = on_gpu(h, view)
    q = torch.from_numpy(np.array(h["q"])).cuda().to(q_dtype or TDT[c.dt])
    lens = torch.tensor(c.lens, dtype=torch.int32, device="cuda")
    out = pli_hip.attn_decode_paged_fp8(q, kp, vp, table, lens, ksc if scales else None, vsc if scales else None,
                                        max_kv=paged_cases.max_kv_of(c))
    return out, pli_hip.last_route()


@pytest.mark.parametrize("name", paged_cases.CASES)
def test_decode_vs_oracle(name):
    c, h = paged_cases.CASES[name], prepared_decode(name)
    out, route = run_decode(c, h)
    assert route == DECODE_ROUTE[c.route], route
    assert out.shape == (c.B, c.Sq, c.H, c.D) and out.dtype == TDT[c.dt]
    got = out.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - h["ref"]).max()
    print(f"case {name}: route {route}, max |err| {err:.3e} (tolerance {TOL[c.dt]:g})")
    assert err <= TOL[c.dt], f"max |err| {err:.3e}"
    for b, n in enumerate(c.lens):
        if n == 0:
            assert not got[b].any(), "an empty sequence's rows are 0"


# ------------------------------------------------------------------ varlen --
@functools.lru_cache(maxsize=None)
def prepared_varlen(name: str):
    c = varlen_cases.CASES[name]
    seed = zlib.crc32(("fp8varlen" + name).encode()) % 1000
    h = lay_out(c.bs, c.Hkv, c.D, c.kv_lens, c.max_blocks, seed)
    cu = np.concatenate([[0], np.cumsum(c.q_lens)]).astype(np.int32)
    h["cu"] = cu
    h["q"] = seeded_normal((int(cu[-1]) + EXTRA, c.H, c.D), seed, c.dt)
    ref = np.zeros((int(cu[-1]), c.H, c.D))
    for b, n in enumerate(c.kv_lens):
        q = h["q"][cu[b]:cu[b + 1]]
        first = max(0, q.shape[0] - n) if c.causal else 0  # bottom-right: rows before `first` see nothing
        if n > 0 and q.shape[0] > first:
            ref[cu[b] + first:cu[b + 1]] = oatt.naive_attention(
                q[None, first:].transpose(0, 2, 1, 3), h["kd"][b:b + 1, :n].transpose(0, 2, 1, 3),
                h["vd"][b:b + 1, :n].transpose(0, 2, 1, 3), causal=c.causal)[0].transpose(1, 0, 2)
    h["ref"] = ref
    return freeze(h)


def run_varlen(c, h, q_dtype=None):
    import pli_hip
    kp, vp, table, ksc, vsc = on_gpu(h)
    q = torch.from_numpy(np.array(h["q"])).cuda().to(q_dtype or TDT[c.dt])
    out = torch.full_like(q, SENTINEL)
    lens = torch.tensor(c.kv_lens, dtype=torch.int32, device="cuda")
    got = pli_hip.attn_varlen_paged_fp8(q, kp, vp, table, lens, torch.from_numpy(np.array(h["cu"])).cuda(), ksc, vsc,
                                        max_kv=varlen_cases.max_kv_of(c), causal=c.causal, out=out)
    assert got is out
    return out, pli_hip.last_route()


@pytest.mark.parametrize("name", varlen_cases.CASES)
def test_varlen_vs_oracle(name):
    c, h = varlen_cases.CASES[name], prepared_varlen(name)
    out, route = run_varlen(c, h)
    assert route == VARLEN_ROUTE[c.route], route
    total = int(h["cu"][-1])
    assert out.shape == (total + EXTRA, c.H, c.D) and out.dtype == TDT[c.dt]
    got = out.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    assert (got[total:] == SENTINEL).all(), "rows past cu[batch] are not written"
    err = np.abs(got[:total] - h["ref"]).max()
    print(f"case {name}: route {route}, max |err| {err:.3e} (tolerance {TOL[c.dt]:g})")
    assert err <= TOL[c.dt], f"max |err| {err:.3e}"
    if c.causal:
        for b, (ql, n) in enumerate(zip(c.q_lens, c.kv_lens)):
            blind = max(0, min(ql, ql - n))
            assert not got[h["cu"][b]:h["cu"][b] + blind].any(), "rows that see no key are exactly 0"


# ------------------------------------------------------- fast against generic --
def test_fast_against_generic():
    """split-K decode case 4 and varlen case 1 on the same pools through the MFMA kernels (bf16 q) and through the
    generic ones (the same q values as fp32, which the fast rule excludes)"""
    c, h = paged_cases.CASES["4"], prepared_decode("4")
    fast, rf = run_decode(c, h)
    gen, rg = run_decode(c, h, q_dtype=torch.float32)
    assert rf == DECODE_ROUTE[paged_cases.COMBINE] and rg == DECODE_ROUTE[paged_cases.GENERIC] and gen.dtype == torch.float32
    err = (fast.float() - gen).abs().max().item()
    print(f"decode case 4: max |fast - generic| {err:.3e}")
    assert err <= TOL["bf16"]
    c, h = varlen_cases.CASES["1"], prepared_varlen("1")
    total = int(h["cu"][-1])
    fast, rf = run_varlen(c, h)
    gen, rg = run_varlen(c, h, q_dtype=torch.float32)
    assert rf == VARLEN_ROUTE[varlen_cases.FAST] and rg == VARLEN_ROUTE[varlen_cases.GENERIC]
    err = (fast[:total].float() - gen[:total]).abs().max().item()
    print(f"varlen case 1: max |fast - generic| {err:.3e}")
    assert err <= TOL["bf16"]


def test_null_scales_equal_ones():
    """NULL scale pointers and tensors of ones: bitwise equal attention outputs (pools passed as uint8 views too)
    and bitwise equal appended codes"""
    import pli_hip
    c, h = paged_cases.CASES["1"], dict(prepared_decode("1"))
    h["ksc"], h["vsc"] = torch.ones(c.Hkv), torch.ones(c.Hkv)
    ones, _ = run_decode(c, h)
    null, route = run_decode(c, h, scales=False, view=torch.uint8)
    assert route == DECODE_ROUTE[paged_cases.FAST] and torch.equal(ones, null)
    scaled, _ = run_decode(c, prepared_decode("1"))
    assert not torch.equal(ones, scaled)
    torch.manual_seed(5)
    kn, vn = (torch.randn(2, 3, 2, 64, device="cuda") * 3 for _ in range(2))
    table = torch.tensor([[1, 0], [2, 3]], dtype=torch.int32, device="cuda")
    lens = torch.tensor([14, 0], dtype=torch.int32, device="cuda")
    pools = [torch.full((4, LAYERS, 16, 2, 64), POISON, dtype=torch.uint8, device="cuda") for _ in range(4)]
    one = torch.ones(2, device="cuda")
    pli_hip.kv_append_paged_fp8(kn, vn, pools[0][:, LAYER], pools[1][:, LAYER], table, lens, one, one)
    pli_hip.kv_append_paged_fp8(kn, vn, pools[2][:, LAYER], pools[3][:, LAYER], table, lens)
    assert torch.equal(pools[0], pools[2]) and torch.equal(pools[1], pools[3]) and not torch.equal(pools[0], pools[1])


# ------------------------------------------------------------------ append --
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """csrc/fp8_codec.h on the host (tests/host/fp8_codec_check.cpp, a plain build)"""
    return build_checker(tmp_path_factory.mktemp("fp8_codec_gpu"), sanitize=False)


POW2 = ([1.0, 0.5, 8.0], [8.0, 1.0, 0.5])  # k / v scales of the bitwise test: the product x * (1 / scale) is exact


def edge_source(shape, dt, scale, flip):
    """a source tensor [..., 3, D] of dtype dt whose values times 1 / scale[head] are the edge values of
    tests/fp8_cases.py (every e4m3 value, every tie and its neighbours, +-0, saturation, +-inf, NaN) and then normal
    data; rounding to bf16 / fp16 moves some off their edge, the expectation is computed from what was stored"""
    edge = edge_values()
    n = int(np.prod(shape))
    assert n >= edge.size
    flat = np.concatenate([edge, 3 * seeded_normal((n - edge.size,), 17 + flip)]).astype(np.float32)
    x = torch.from_numpy(flat[::-1].copy() if flip else flat).reshape(shape)
    return (x * torch.tensor(scale)[:, None]).to(TDT[dt])


def expected_codes(checker, src, scale):
    """codes of a source tensor by the header codec, checked against torch's clamp + cast where the value is no NaN"""
    y = src.float() * (1.0 / torch.tensor(scale, dtype=torch.float32))[:, None]  # exact: powers of two
    codes = torch.from_numpy(codec_codes(checker, y.numpy()))
    ok = ~torch.isnan(y)
    assert torch.equal(codes[ok], torch_codes(y)[ok])
    assert ((codes[~ok] & 0x7F) == 0x7F).all() and int((~ok).sum()) >= 4
    return codes


def random_pools(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, shape, dtype=torch.uint8, generator=g) for _ in range(2)]


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_append_is_bitwise(checker, dt):
    import pli_hip
    Hkv, D, bs, mb, nb, B, T = 3, 64, 16, 2, 9, 3, 5
    table_h = torch.from_numpy(np.random.default_rng(1).permutation(nb)[:B * mb].reshape(B, mb).astype(np.int32))
    kn, vn = edge_source((B, T, Hkv, D), dt, POW2[0], 0), edge_source((B, T, Hkv, D), dt, POW2[1], 1)
    kc, vc = expected_codes(checker, kn, POW2[0]), expected_codes(checker, vn, POW2[1])
    assert set(range(256)) <= set(kc.reshape(-1).tolist()) | {0x7F, 0xFF}  # every code is produced
    ksc, vsc = (torch.tensor(s, device="cuda") for s in POW2)
    # [15, 16, 0]: across a page boundary, the start of a fresh page, an empty sequence;
    # [30, 31, 32]: tokens past max_blocks * block_size = 32 are dropped
    for lens_h in ([15, 16, 0], [30, 31, 32]):
        kpool, vpool = random_pools((nb, LAYERS, bs, Hkv, D), 3)
        want_k, want_v = kpool.clone(), vpool.clone()
        for b in range(B):
            for t in range(T):
                pos = lens_h[b] + t
                if pos < mb * bs:
                    want_k[table_h[b, pos // bs], LAYER, pos % bs] = kc[b, t]
                    want_v[table_h[b, pos // bs], LAYER, pos % bs] = vc[b, t]
        kpool, vpool = kpool.cuda().view(FP8), vpool.cuda().view(FP8)
        lens = torch.tensor(lens_h, dtype=torch.int32, device="cuda")
        pli_hip.kv_append_paged_fp8(kn.cuda(), vn.cuda(), kpool[:, LAYER], vpool[:, LAYER], table_h.cuda(), lens, ksc, vsc)
        assert pli_hip.last_route() == "kv_append_paged_fp8"
        # every byte of both pools: the scattered rows exactly, everything else (layer 0 too) unchanged
        assert torch.equal(kpool.view(torch.uint8).cpu(), want_k) and torch.equal(vpool.view(torch.uint8).cpu(), want_v)
        assert lens.tolist() == lens_h


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_varlen_append_is_bitwise(checker, dt):
    import pli_hip
    Hkv, D, bs, mb, nb = 3, 64, 16, 2, 12
    table_h = torch.from_numpy(np.random.default_rng(2).permutation(nb)[:4 * mb].reshape(4, mb).astype(np.int32))
    ksc, vsc = (torch.tensor(s, device="cuda") for s in POW2)
    # (q_lens, seq_lens after the step): across a page boundary, a fresh page, a sequence sitting out (q_len 0), one
    # token; then tokens past max_blocks * block_size = 32 and positions below 0 (seq_len < q_len) are dropped
    for q_lens, lens_h in (([5, 16, 0, 1], [18, 32, 7, 1]), ([6, 3, 2, 4], [35, 33, 32, 2])):
        cu_h = [0] + list(np.cumsum(q_lens))
        total = int(cu_h[-1])
        shape = (total + EXTRA, Hkv, D)
        kn, vn = edge_source(shape, dt, POW2[0], 0), edge_source(shape, dt, POW2[1], 1)
        kc, vc = expected_codes(checker, kn, POW2[0]), expected_codes(checker, vn, POW2[1])
        kpool, vpool = random_pools((nb, LAYERS, bs, Hkv, D), 4)
        want_k, want_v = kpool.clone(), vpool.clone()
        written = 0
        for b, ql in enumerate(q_lens):
            for i in range(ql):
                pos = lens_h[b] - ql + i
                if 0 <= pos < mb * bs:
                    want_k[table_h[b, pos // bs], LAYER, pos % bs] = kc[cu_h[b] + i]
                    want_v[table_h[b, pos // bs], LAYER, pos % bs] = vc[cu_h[b] + i]
                    written += 1
        assert written == (total if lens_h[0] == 18 else 3 + 2 + 2 + 2)
        kpool, vpool = kpool.cuda().view(FP8), vpool.cuda().view(FP8)
        lens = torch.tensor(lens_h, dtype=torch.int32, device="cuda")
        cu = torch.tensor(cu_h, dtype=torch.int32, device="cuda")
        pli_hip.kv_append_varlen_paged_fp8(kn.cuda(), vn.cuda(), kpool[:, LAYER], vpool[:, LAYER], table_h.cuda(), lens, cu,
                                           ksc, vsc)
        assert pli_hip.last_route() == "kv_append_varlen_paged_fp8"
        assert torch.equal(kpool.view(torch.uint8).cpu(), want_k) and torch.equal(vpool.view(torch.uint8).cpu(), want_v)
        assert lens.tolist() == lens_h and cu.tolist() == cu_h


def test_append_error_bound_with_general_scales():
    """scales that are no powers of two: |code * s - x| <= 1/2 spacing(code) * s * (1 + 2^-10) for every element that
    does not saturate -- round-to-nearest of x * fl(1 / s) with the reciprocal and the product rounded to fp32
    (relative 2^-23 together, on a value of at most 16 spacings: 2^-19 spacings, far inside the 2^-11 allowed)"""
    import pli_hip
    Hkv, D, bs, B, T = 4, 64, 16, 2, 8
    ksc, vsc = scales_of(Hkv)
    x = [torch.from_numpy(seeded_normal((B, T, Hkv, D), s)) * 2 for s in (41, 42)]
    x[0][0, 0, :, :4] = torch.tensor([1e3, -1e3, 5.0, -0.0])  # two that saturate under every scale here
    table = torch.tensor([[2, 0], [1, 3]], dtype=torch.int32, device="cuda")
    lens = torch.tensor([10, 0], dtype=torch.int32, device="cuda")
    pools = [torch.zeros(4, LAYERS, bs, Hkv, D, dtype=torch.uint8, device="cuda") for _ in range(2)]
    pli_hip.kv_append_paged_fp8(x[0].cuda(), x[1].cuda(), pools[0][:, LAYER], pools[1][:, LAYER], table, lens, ksc.cuda(),
                                vsc.cuda())
    worst = 0.0
    for pool, src, sc in zip(pools, x, (ksc, vsc)):
        got = torch.empty(B, T, Hkv, D, dtype=torch.uint8)
        for b, (start, row) in enumerate(zip((10, 0), ((2, 0), (1, 3)))):
            for t in range(T):
                got[b, t] = pool[row[(start + t) // bs], LAYER, (start + t) % bs].cpu()
        s64, x64 = sc.double()[:, None], src.double()
        free = (x64 / s64).abs() < 448
        assert ((got[~free] & 0x7F) == POISON).all() and int((~free).sum()) == (2 * Hkv if src is x[0] else 0)
        err = (decode_table().double()[got.long()] * s64 - x64).abs()
        bound = 0.5 * spacing_of(got).double() * s64 * (1 + 2.0 ** -10)
        assert bool((err <= bound)[free].all()), float((err / bound)[free].max())
        worst = max(worst, float((err / bound)[free].max()))
    print(f"max |code * s - x| / bound: {worst:.6f}")
    assert worst > 0.9  # the bound is not slack: some element sits next to a tie


# ------------------------------------------------------------ graph replay --
def test_graph_replay_reads_scales_table_and_lengths_on_the_device():
    """append + decode (n_kv_add=1) + seq_lens.add_(1) captured once; before every replay k_scale / v_scale, the
    table and the lengths are rewritten in place: each replay equals the eager calls on the same contents bitwise"""
    import pli_hip
    B, H, Hkv, D, bs, mb, nb = 2, 8, 2, 128, 16, 16, 40
    torch.manual_seed(9)
    dt = torch.bfloat16
    configs = [  # table, start lengths, k_scale, v_scale
        (torch.randperm(nb)[:B * mb].reshape(B, mb).to(torch.int32), [14, 31], [0.37, 1.9], [1.3, 0.53]),
        (torch.randperm(nb)[:B * mb].reshape(B, mb).to(torch.int32), [200, 47], [1.1, 0.71], [0.9, 2.3]),
    ]
    init = [((torch.randint(0, 0x48, (nb, LAYERS, bs, Hkv, D)) | (torch.randint(0, 2, (nb, LAYERS, bs, Hkv, D)) << 7))
             .to(torch.uint8).cuda()) for _ in range(2)]  # |values| < 4, no NaN
    g_k, g_v = (p.clone().view(FP8) for p in init)
    e_k, e_v = (p.clone().view(FP8) for p in init)
    table_s = torch.zeros(B, mb, dtype=torch.int32, device="cuda")
    ks_s, vs_s = torch.ones(Hkv, device="cuda"), torch.ones(Hkv, device="cuda")
    g_lens = torch.zeros(B, dtype=torch.int32, device="cuda")
    q_s, kn_s, vn_s = (torch.zeros(B, 1, h, D, device="cuda", dtype=dt) for h in (H, Hkv, Hkv))
    out_s = torch.empty(B, 1, H, D, device="cuda", dtype=dt)
    ws_bytes = pli_hip.attn_decode_paged_workspace_bytes(B, H, Hkv, 1, mb * bs, D)
    assert ws_bytes > 0  # split-K: the combine kernel is in the graph
    ws = torch.empty(ws_bytes // 4, device="cuda", dtype=torch.float32)

    def step(q, kn, vn, k, v, lens, out):
        pli_hip.kv_append_paged_fp8(kn, vn, k[:, LAYER], v[:, LAYER], table_s, lens, ks_s, vs_s)
        pli_hip.attn_decode_paged_fp8(q, k[:, LAYER], v[:, LAYER], table_s, lens, ks_s, vs_s, n_kv_add=1, out=out,
                                      workspace=ws)
        lens.add_(1)

    def load(i):
        table, start, ks, vs = configs[i]
        table_s.copy_(table), ks_s.copy_(torch.tensor(ks)), vs_s.copy_(torch.tensor(vs))
        g_lens.copy_(torch.tensor(start, dtype=torch.int32))
        return g_lens.clone()

    # warm-up on throwaway state (code objects loaded before the capture)
    load(0)
    step(q_s, kn_s, vn_s, init[0].clone().view(FP8), init[1].clone().view(FP8), g_lens.clone(), torch.empty_like(out_s))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(q_s, kn_s, vn_s, g_k, g_v, g_lens, out_s)
    assert torch.equal(g_k.view(torch.uint8), init[0])  # a capture runs nothing
    for i in (0, 1, 0, 1):
        e_lens = load(i)
        q, kn, vn = (torch.randn(B, 1, h, D, device="cuda").to(dt) for h in (H, Hkv, Hkv))
        out_e = torch.empty_like(out_s)
        step(q, kn, vn, e_k, e_v, e_lens, out_e)
        assert pli_hip.last_route() == DECODE_ROUTE[paged_cases.COMBINE]
        q_s.copy_(q), kn_s.copy_(kn), vn_s.copy_(vn)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_s, out_e), f"replay with config {i}"
        assert g_lens.tolist() == e_lens.tolist() == [n + 1 for n in configs[i][1]]
        assert torch.equal(g_k.view(torch.uint8), e_k.view(torch.uint8)) and torch.equal(g_v.view(torch.uint8), e_v.view(torch.uint8))
    assert not torch.equal(g_k.view(torch.uint8), init[0])


# ---------------------------------------------------------- PagedKVCache --
def test_fp8_cache_round_trip():
    """PagedKVCache(kv_dtype=float8_e4m3fn): two prompts through append_packed, then three decode steps of
    extend_blocks / tables / append / attend on both layers, against the oracle over the host-quantised history"""
    from ch07 import PagedKVCache
    H, Hkv, D, bs = 8, 2, 64, 16
    cache = PagedKVCache(num_blocks=6, block_size=bs, num_layers=LAYERS, num_heads=Hkv, head_dim=D,
                         dtype=torch.bfloat16, device="cuda", kv_dtype=FP8)
    assert cache.k_cache.shape == (6, LAYERS, bs, Hkv, D) and cache.k_cache.dtype == FP8
    assert cache.k_scale.shape == (LAYERS, Hkv) and cache.k_scale.is_cuda and bool((cache.v_scale == 1).all())
    assert cache.get_memory_usage()["bytes_per_block"] == 2 * LAYERS * bs * Hkv * D
    sc = {}
    for layer in range(LAYERS):
        sc[layer] = tuple(s * (1 + 0.25 * layer) for s in scales_of(Hkv))
        cache.set_scales(layer, *sc[layer])
    bf = lambda a: torch.from_numpy(a).cuda().bfloat16()  # noqa: E731
    deq = lambda a, s: dequantise(quantise(torch.from_numpy(a), s), s)  # noqa: E731
    seeds = iter(range(50_000, 51_000))
    rids, prompts = [1, 2], [20, 7]
    for rid, n in zip(rids, prompts):
        cache.allocate_blocks(rid, n)
    table, lens, cu = cache.tables_packed(rids, prompts)
    cu_h, hist = cu.tolist(), {}
    for layer in range(LAYERS):
        k, v = (seeded_normal((27, Hkv, D), next(seeds), "bf16") for _ in range(2))
        cache.append_packed(layer, bf(k), bf(v), table, lens, cu)
        kd, vd = deq(k, sc[layer][0]), deq(v, sc[layer][1])
        for i, rid in enumerate(rids):
            hist[rid, layer] = ([kd[cu_h[i]:cu_h[i + 1]]], [vd[cu_h[i]:cu_h[i + 1]]])
    worst = 0.0
    for _ in range(3):
        for rid in rids:
            cache.extend_blocks(rid, 1)
        table, lens = cache.tables(rids, max_blocks=2)
        for layer in range(LAYERS):
            q, k, v = (seeded_normal((2, 1, s, D), next(seeds), "bf16") for s in (H, Hkv, Hkv))
            cache.append(layer, bf(k), bf(v), table, lens)
            out = cache.attend(layer, bf(q), table, lens).float().cpu().numpy()
            kd, vd = deq(k, sc[layer][0]), deq(v, sc[layer][1])
            for i, rid in enumerate(rids):
                hist[rid, layer][0].append(kd[i])
                hist[rid, layer][1].append(vd[i])
                ks, vs = (np.concatenate(x)[None].transpose(0, 2, 1, 3) for x in hist[rid, layer])
                assert ks.shape[2] == cache.block_tables[rid].num_tokens
                ref = oatt.naive_attention(q[i:i + 1].transpose(0, 2, 1, 3), ks, vs, causal=True)
                worst = max(worst, np.abs(out[i:i + 1].transpose(0, 2, 1, 3) - ref).max())
    print(f"max |err| over 3 decode steps {worst:.3e}")
    assert worst <= TOL["bf16"], f"max |err| {worst:.3e}"
    assert [cache.block_tables[r].num_tokens for r in rids] == [23, 10]
