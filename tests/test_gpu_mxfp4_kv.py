"""GPU tests of the MXFP4 paged KV cache: the quantising appends
(pli_kv_append_paged_mxfp4 / pli_kv_append_varlen_paged_mxfp4), decode attention
over code + scale pools (pli_attn_decode_paged_mxfp4) and
ch07.PagedKVCache(kv_dtype=torch.float4_e2m1fn_x2).

pli_hip.quantize_weight_mxfp4(rows, torch.float16) is the append's bit pattern;
the attention reference is oracle.attention.naive_attention in float64 over
dequantize_weight_mxfp4 of the pool, within TOL of tests/test_gpu_fp8_kv.py, and
the MFMA route is also held bitwise to attn_decode_paged over a pool of the
dequantised values.  Every byte no sequence owns is code 0x77 under scale byte
0xFF, so a read past n_kv - 1 shows as NaN.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from oracle import attention as oatt
from oracle.numerics import seeded_normal
from test_gpu_fp8_kv import TDT, TOL

pytestmark = pytest.mark.gpu
MX = torch.float4_e2m1fn_x2
H, HKV = 8, 2
LENS = (0, 1, 33, 100)


def quant(x: torch.Tensor):
    """(codes [..., D/2], exps [..., D/32], dequantised fp32 [..., D]) of x [..., D] by the Python mirror"""
    import pli_hip
    D = x.shape[-1]
    c, e = pli_hip.quantize_weight_mxfp4(x.reshape(-1, D).float(), torch.float16)
    d = pli_hip.dequantize_weight_mxfp4(c, e)
    return c.reshape(*x.shape[:-1], D // 2), e.reshape(*x.shape[:-1], D // 32), d.reshape(x.shape)


@functools.lru_cache(maxsize=None)
def lay_out(bs, Hkv, D, lens, max_blocks, seed, spare=3):
    """host pools (codes, exps for K and V; poison everywhere else), the permuted table and the dequantised K / V
    [B, longest, Hkv, D]; computed once per shape and treated as read-only"""
    rng = np.random.default_rng(seed)
    B, owned = len(lens), [-(-n // bs) for n in lens]
    nb = sum(owned) + spare
    order = torch.from_numpy(rng.permutation(nb))
    table = torch.full((B, max_blocks), int(order[sum(owned)]), dtype=torch.int32)
    longest = max(max(lens), 1)
    h = {"table": table}
    for name, s in (("k", 1), ("v", 2)):
        c, e, d = quant(torch.from_numpy(seeded_normal((B, longest, Hkv, D), seed + s)))
        pool, exp = torch.full((nb, bs, Hkv, D // 2), 0x77, dtype=torch.uint8), torch.full((nb, bs, Hkv, D // 32), 0xFF, dtype=torch.uint8)
        at = 0
        for b, n in enumerate(lens):
            for i in range(owned[b]):
                p, rows = int(order[at + i]), slice(i * bs, min((i + 1) * bs, n))
                table[b, i] = p
                pool[p, :rows.stop - rows.start], exp[p, :rows.stop - rows.start] = c[b, rows], e[b, rows]
            at += owned[b]
        h[name], h[name + "e"], h[name + "d"] = pool, exp, d
    return h


def reference(q, h, lens, causal):
    """float64 attention of q [B, Sq, H, D] (numpy) over each sequence's dequantised rows; rows that see no key are 0"""
    ref = np.zeros(q.shape)
    Sq = q.shape[1]
    for b, n in enumerate(lens):
        first = max(0, Sq - n) if causal else 0
        if n > 0 and Sq > first:
            kd, vd = (h[x][b:b + 1, :n].double().numpy().transpose(0, 2, 1, 3) for x in ("kd", "vd"))
            ref[b, first:] = oatt.naive_attention(q[b:b + 1, first:].transpose(0, 2, 1, 3), kd, vd,
                                                  causal=causal)[0].transpose(1, 0, 2)
    return ref


def run(h, q, lens, causal, max_kv, **kw):
    import pli_hip
    out = pli_hip.attn_decode_paged_mxfp4(q, h["k"].cuda(), h["v"].cuda(), h["ke"].cuda(), h["ve"].cuda(), h["table"].cuda(),
                                          torch.tensor(lens, dtype=torch.int32, device="cuda"), causal=causal,
                                          max_kv=max_kv, **kw)
    return out, pli_hip.last_route()


def dense_pools(h, dt):
    """16-bit pools holding the dequantised values (exact in bf16 and fp16); a poisoned block becomes 0"""
    import pli_hip
    out = []
    for name in ("k", "v"):
        c, e = h[name], h[name + "e"].clone()
        e[e == 0xFF] = 127
        d = pli_hip.dequantize_weight_mxfp4(c.reshape(-1, c.shape[-1]), e.reshape(-1, e.shape[-1]))
        out.append(d.reshape(*c.shape[:-1], -1).to(dt).cuda())
    return out


# (B, heads, kv heads, lengths, max_kv): the issue's shape (one step per wave), and 128 (batch, kv head) pairs, which
# the plan gives one chunk each, so a wave walks 4 steps and the two-step-deep load pipeline turns over
SHAPES = {"b4": (H, HKV, LENS, 128), "deep": (8, 8, tuple([0, 512, 97, 450] + [300 + 13 * i for i in range(12)]), 512)}
CASES = [(dt, D, nq, bs, "b4") for dt in ("bf16", "fp16") for D in (64, 128) for nq in (1, 2) for bs in (16, 64)] + \
        [(dt, 64, nq, 16, "deep") for dt in ("bf16", "fp16") for nq in (1, 2)]


@pytest.mark.parametrize("dt,D,nq,bs,shape", CASES)
def test_decode_vs_oracle_and_bitwise_vs_16bit(dt, D, nq, bs, shape):
    """n_q 1 runs non-causal, n_q 2 causal"""
    import pli_hip
    causal = nq == 2
    heads, hkv, lens, max_kv = SHAPES[shape]
    h = lay_out(bs, hkv, D, lens, max_kv // bs, 7)
    qh = seeded_normal((len(lens), nq, heads, D), 11, dt)
    q = torch.from_numpy(qh).cuda().to(TDT[dt])
    out, route = run(h, q, lens, causal, max_kv)
    assert route == "attn_decode_paged_mxfp4" and out.dtype == TDT[dt]
    got = out.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), "a poisoned byte (a token at or past n_kv, a page no row names) was read"
    err = np.abs(got - reference(qh, h, lens, causal)).max()
    print(f"{shape} {dt} D{D} nq{nq} bs{bs}: max |err| {err:.3e} (tolerance {TOL[dt]:g})")
    assert err <= TOL[dt]
    assert not got[0].any(), "an empty sequence's rows are 0"
    kd, vd = dense_pools(h, TDT[dt])
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    dense = pli_hip.attn_decode_paged(q, kd, vd, h["table"].cuda(), lens_d, causal=causal, max_kv=max_kv)
    assert pli_hip.last_route() == "attn_decode_paged" and torch.equal(out, dense)


def test_split_k():
    """2 chunks of 128 keys: the workspace from the size function, guarded behind its last byte, and an output with
    guarded gaps between its rows; bitwise the 16-bit split-K call too"""
    import pli_hip
    D, n, max_kv, bs = 128, 200, 256, 16
    need = pli_hip.attn_decode_paged_workspace_bytes(1, H, HKV, 1, max_kv, D)
    assert need > 0 and pli_hip.attn_decode_paged_workspace_bytes(1, H, HKV, 1, 128, D) == 0
    h = lay_out(bs, HKV, D, (n,), max_kv // bs, 21)
    qh = seeded_normal((1, 1, H, D), 22, "bf16")
    q = torch.from_numpy(qh).cuda().bfloat16()
    ws = torch.full((need // 4 + 64,), 777.0, device="cuda")
    wide = torch.full((1, 1, H, D + 8), 777.0, device="cuda", dtype=torch.bfloat16)
    out, route = run(h, q, (n,), True, max_kv, out=wide[..., :D], workspace=ws[:need // 4])
    assert route == "attn_decode_paged_mxfp4+attn_decode_paged_combine"
    assert bool((ws[need // 4:] == 777.0).all()) and bool((wide[..., D:] == 777.0).all())
    err = np.abs(out.float().cpu().numpy() - reference(qh, h, (n,), True)).max()
    print(f"split-K: max |err| {err:.3e}")
    assert err <= TOL["bf16"]
    kd, vd = dense_pools(h, torch.bfloat16)
    dense = pli_hip.attn_decode_paged(q, kd, vd, h["table"].cuda(), torch.tensor([n], dtype=torch.int32, device="cuda"),
                                      max_kv=max_kv)
    assert pli_hip.last_route() == "attn_decode_paged+attn_decode_paged_combine" and torch.equal(out, dense)


@pytest.mark.parametrize("D,bs,fast_too", [(64, 16, True), (96, 24, False)])
def test_generic_route(D, bs, fast_too):
    """fp32 q (and a head_dim / block size the MFMA kernel does not take) against the oracle at 1e-3; on the shared
    case the MFMA kernel against the generic one within the 16-bit tolerance"""
    max_kv = 120 if bs == 24 else 128
    h = lay_out(bs, HKV, D, LENS, max_kv // bs, 31)
    qh = seeded_normal((len(LENS), 2, H, D), 32, "bf16")
    gen, route = run(h, torch.from_numpy(qh).cuda(), LENS, True, max_kv)
    assert route == "attn_decode_paged_generic_mxfp4" and gen.dtype == torch.float32
    err = np.abs(gen.cpu().numpy() - reference(qh, h, LENS, True)).max()
    print(f"generic D{D} bs{bs}: max |err| {err:.3e}")
    assert err <= TOL["fp32"]
    if fast_too:
        fast, route = run(h, torch.from_numpy(qh).cuda().bfloat16(), LENS, True, max_kv)
        assert route == "attn_decode_paged_mxfp4" and (fast.float() - gen).abs().max().item() <= TOL["bf16"]


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("side", ["k", "v"])
def test_nan_rule(side, dt):
    """a 0xFF scale byte in the last key of sequence 1: its second query row (the one that sees the key) is NaN in every
    element, its first row is not, sequences 0 and 2 are bitwise what they were"""
    D, bs, lens = 128, 16, (33, 100, 20)
    h = dict(lay_out(bs, HKV, D, lens, 8, 41))
    q = torch.from_numpy(seeded_normal((3, 2, H, D), 42, "bf16")).cuda().to(TDT[dt])
    clean, _ = run(h, q, lens, True, 128)
    exp = h[side + "e"].clone()
    exp[int(h["table"][1, 99 // bs]), 99 % bs, 1, 2] = 0xFF
    h[side + "e"] = exp
    bad, route = run(h, q, lens, True, 128)
    assert route == ("attn_decode_paged_mxfp4" if dt == "bf16" else "attn_decode_paged_generic_mxfp4")
    assert torch.equal(bad[0], clean[0]) and torch.equal(bad[2], clean[2])
    hit = slice(4, 8)  # the query heads of kv head 1
    assert bool(torch.isnan(bad[1, 1, hit]).all()) and bool(torch.isfinite(bad[1, 0]).all())
    assert torch.equal(bad[1, 1, :4], clean[1, 1, :4])


# ------------------------------------------------------------------ appends --
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
def test_append_is_bitwise(dt, D, packed):
    """rows land where the 16-bit appends put them, as the mirror's codes and bytes; every other byte keeps its sentinel.
    Starts [15, 16, 0, 30]: across a page boundary, a fresh page, an empty sequence, past the table row (dropped)"""
    import pli_hip
    bs, mb, nb, T, start = 16, 2, 11, 5, [15, 16, 0, 30]
    B = len(start)
    table = torch.from_numpy(np.random.default_rng(3).permutation(nb)[:B * mb].reshape(B, mb).astype(np.int32))
    src = [(torch.from_numpy(seeded_normal((B, T, HKV, D), s)) * torch.logspace(-6, 3, T)[None, :, None, None]).to(TDT[dt])
           for s in (51, 52)]
    src[0][0, 0, 0, :32] = 0  # an all-zero block: scale byte 127
    pools = [torch.full((nb, bs, HKV, w), 0xA5, dtype=torch.uint8) for w in (D // 2, D // 2, D // 32, D // 32)]
    want = [p.clone() for p in pools]
    for x, wc, we in ((src[0], want[0], want[2]), (src[1], want[1], want[3])):
        c, e, _ = quant(x)
        for b in range(B):
            for t in range(T):
                pos = start[b] + t
                if pos < mb * bs:
                    wc[int(table[b, pos // bs]), pos % bs], we[int(table[b, pos // bs]), pos % bs] = c[b, t], e[b, t]
    dev = [p.cuda() for p in pools]
    if packed:
        lens = torch.tensor([s + T for s in start], dtype=torch.int32, device="cuda")
        cu = torch.arange(0, (B + 1) * T, T, dtype=torch.int32, device="cuda")
        pli_hip.kv_append_varlen_paged_mxfp4(src[0].reshape(B * T, HKV, D).cuda(), src[1].reshape(B * T, HKV, D).cuda(), *dev,
                                             table.cuda(), lens, cu)
    else:
        pli_hip.kv_append_paged_mxfp4(src[0].cuda(), src[1].cuda(), *dev, table.cuda(),
                                      torch.tensor(start, dtype=torch.int32, device="cuda"))
    assert pli_hip.last_route() == ("kv_append_varlen_paged_mxfp4" if packed else "kv_append_paged_mxfp4")
    for got, exp_ in zip(dev, want):
        assert torch.equal(got.cpu(), exp_)
    assert int(want[2].min()) == 127 - 13 and int(want[2].max()) > 127  # the lower clamp and a large block are in the case


def test_append_nan_and_inf():
    """a NaN element: code 0, outside amax, block byte 0xFF; +-inf: the code of +-6, outside amax; the rest of the block
    as the mirror quantises it without them"""
    import pli_hip
    D = 64
    x = torch.from_numpy(seeded_normal((1, 1, 1, D), 61)) * 3
    x[..., 3], x[..., 5], x[..., 6], x[..., 40] = float("nan"), float("inf"), float("-inf"), float("inf")
    finite = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    c, e, _ = quant(finite)
    c, e = c.reshape(-1).clone(), e.reshape(-1).clone()
    c[1] = c[1] & 0x0F                       # element 3 (NaN): code 0
    c[2] = (c[2] & 0x0F) | 0x70              # element 5 (+inf): code 7
    c[3] = (c[3] & 0xF0) | 0x0F              # element 6 (-inf): code 15
    c[20] = (c[20] & 0xF0) | 0x07            # element 40 (+inf), second block: its byte stays the finite amax's
    e[0] = 0xFF
    pools = [torch.zeros(1, 16, 1, w, dtype=torch.uint8, device="cuda") for w in (D // 2, D // 2, D // 32, D // 32)]
    zero = torch.zeros(1, 1, dtype=torch.int32, device="cuda")
    pli_hip.kv_append_paged_mxfp4(x.cuda(), x.cuda(), *pools, zero, zero[0])
    for codes, exps in ((pools[0], pools[2]), (pools[1], pools[3])):
        assert torch.equal(codes[0, 0, 0].cpu(), c) and torch.equal(exps[0, 0, 0].cpu(), e)


# ------------------------------------------------------------ graph replay --
def test_graph_replay_reads_table_lengths_and_pools_on_the_device():
    """append + attend (split-K, n_kv_add=1) captured once; before each replay the table, the lengths and the pool
    bytes are rewritten in place: every replay equals the eager calls on the same contents bitwise"""
    import pli_hip
    B, D, bs, mb, nb = 2, 128, 16, 16, 40
    torch.manual_seed(9)
    dt = torch.bfloat16
    shapes = [(nb, bs, HKV, D // 2), (nb, bs, HKV, D // 2), (nb, bs, HKV, D // 32), (nb, bs, HKV, D // 32)]
    g_pools, e_pools = ([torch.zeros(s, dtype=torch.uint8, device="cuda") for s in shapes] for _ in range(2))
    table = torch.zeros(B, mb, dtype=torch.int32, device="cuda")
    g_lens = torch.zeros(B, dtype=torch.int32, device="cuda")
    q_s, kn_s, vn_s = (torch.zeros(B, 1, h, D, device="cuda", dtype=dt) for h in (H, HKV, HKV))
    out_s = torch.empty(B, 1, H, D, device="cuda", dtype=dt)
    ws_bytes = pli_hip.attn_decode_paged_workspace_bytes(B, H, HKV, 1, mb * bs, D)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes // 4, device="cuda")

    def step(q, kn, vn, pools, lens, out):
        pli_hip.kv_append_paged_mxfp4(kn, vn, *pools, table, lens)
        pli_hip.attn_decode_paged_mxfp4(q, *pools, table, lens, n_kv_add=1, out=out, workspace=ws)
        lens.add_(1)

    def load(i, start):
        """new table, lengths and pool contents (random codes under scale bytes of the write range), in place"""
        g = torch.Generator().manual_seed(100 + i)
        table.copy_(torch.randperm(nb, generator=g)[:B * mb].reshape(B, mb).to(torch.int32))
        g_lens.copy_(torch.tensor(start, dtype=torch.int32))
        for s, gp, ep in zip(shapes, g_pools, e_pools):
            lo, hi = (0, 256) if s[-1] == D // 2 else (114, 141)
            fresh = torch.randint(lo, hi, s, generator=g).to(torch.uint8).cuda()
            gp.copy_(fresh), ep.copy_(fresh)
        return g_lens.clone()

    step(q_s, kn_s, vn_s, [p.clone() for p in g_pools], load(0, [3, 5]), torch.empty_like(out_s))  # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(q_s, kn_s, vn_s, g_pools, g_lens, out_s)
    for i, start in enumerate(([14, 31], [200, 47], [255, 0])):
        e_lens = load(i, start)
        q, kn, vn = (torch.randn(B, 1, h, D, device="cuda").to(dt) for h in (H, HKV, HKV))
        out_e = torch.empty_like(out_s)
        step(q, kn, vn, e_pools, e_lens, out_e)
        assert pli_hip.last_route() == "attn_decode_paged_mxfp4+attn_decode_paged_combine"
        q_s.copy_(q), kn_s.copy_(kn), vn_s.copy_(vn)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_s, out_e) and bool(torch.isfinite(out_s.float()).all()), f"replay {i}"
        assert g_lens.tolist() == e_lens.tolist() == [n + 1 for n in start]
        assert all(torch.equal(a, b) for a, b in zip(g_pools, e_pools))


# ---------------------------------------------------------- PagedKVCache --
def test_mxfp4_cache_round_trip():
    """two prompts through append_packed, then three decode steps of extend_blocks / tables / append / attend on both
    layers, against float64 attention over the mirror-quantised history"""
    from ch07 import PagedKVCache
    D, bs, layers = 64, 16, 2
    cache = PagedKVCache(num_blocks=6, block_size=bs, num_layers=layers, num_heads=HKV, head_dim=D, dtype=torch.bfloat16,
                         device="cuda", kv_dtype=MX)
    assert cache.k_cache.shape == (6, layers, bs, HKV, D // 2) and cache.k_cache.dtype == torch.uint8
    assert cache.v_exp_cache.shape == (6, layers, bs, HKV, D // 32) and cache.k_scale is None
    bf = lambda a: torch.from_numpy(a).cuda().bfloat16()  # noqa: E731
    deq = lambda a: quant(torch.from_numpy(a))[2].double().numpy()  # noqa: E731
    seeds = iter(range(60_000, 61_000))
    rids, prompts = [1, 2], [20, 7]
    for rid, n in zip(rids, prompts):
        cache.allocate_blocks(rid, n)
    table, lens, cu = cache.tables_packed(rids, prompts)
    cu_h, hist = cu.tolist(), {}
    for layer in range(layers):
        k, v = (seeded_normal((27, HKV, D), next(seeds), "bf16") for _ in range(2))
        cache.append_packed(layer, bf(k), bf(v), table, lens, cu)
        for i, rid in enumerate(rids):
            hist[rid, layer] = ([deq(k)[cu_h[i]:cu_h[i + 1]]], [deq(v)[cu_h[i]:cu_h[i + 1]]])
    with pytest.raises(NotImplementedError, match="kv_dtype"):
        cache.attend_packed(0, bf(k)[:, :1].repeat(1, H, 1), table, lens, cu)
    worst = 0.0
    for _ in range(3):
        for rid in rids:
            cache.extend_blocks(rid, 1)
        table, lens = cache.tables(rids, max_blocks=2)
        for layer in range(layers):
            q, k, v = (seeded_normal((2, 1, s, D), next(seeds), "bf16") for s in (H, HKV, HKV))
            cache.append(layer, bf(k), bf(v), table, lens)
            out = cache.attend(layer, bf(q), table, lens).float().cpu().numpy()
            for i, rid in enumerate(rids):
                hist[rid, layer][0].append(deq(k)[i])
                hist[rid, layer][1].append(deq(v)[i])
                ks, vs = (np.concatenate(x)[None].transpose(0, 2, 1, 3) for x in hist[rid, layer])
                ref = oatt.naive_attention(q[i:i + 1].transpose(0, 2, 1, 3), ks, vs, causal=True)
                worst = max(worst, np.abs(out[i:i + 1].transpose(0, 2, 1, 3) - ref).max())
    print(f"max |err| over 3 decode steps {worst:.3e}")
    assert worst <= TOL["bf16"]
    assert [cache.block_tables[r].num_tokens for r in rids] == [23, 10]
