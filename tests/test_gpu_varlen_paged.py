"""GPU parity of packed variable-length paged attention
(pli_attn_varlen_paged), the packed append (pli_kv_append_varlen_paged) and
ch07.PagedKVCache's packed methods.

Oracle: each sequence's pages are gathered on the host with numpy and
oracle.attention.naive_attention runs in float64 per sequence on the same
rounded inputs, with the sequence's own q_len and n_kv (its causal mask is
bottom-right); rows that see no key are 0.  Tolerance: the project's own
(tests/test_gpu_paged.py), 1e-2 for bf16 / fp16 outputs, 1e-3 for fp32.

Layout as in tests/test_gpu_paged.py: two-layer 5-D pools attended over layer
1, a randomly permuted table over a pool with spare pages, K = 300 / V = 1e4 in
every page no sequence owns, in last-page tails, in the other layer and (through
a spare page) behind every unused table entry; q and o carry three sentinel
rows past cu[batch], which must stay untouched.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np
import pytest
import torch

from oracle import attention as oatt
from oracle.numerics import seeded_normal
from varlen_cases import APPEND, CASES, FAST, GENERIC, VCase, max_kv_of

pytestmark = pytest.mark.gpu
TDT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
TOL = {"fp32": 1e-3, "fp16": 1e-2, "bf16": 1e-2}
POISON_K, POISON_V = 300.0, 1e4
LAYERS, LAYER = 2, 1
EXTRA, SENTINEL = 3, 77.0


def lay_out(c: VCase, seed: int, identity: bool = False, spare: int = 5):
    """host arrays of a case: packed q [T + EXTRA, H, D], the 5-D pools, the table, cu, per-sequence K / V"""
    rng = np.random.default_rng(seed)
    B = len(c.q_lens)
    owned = [-(-n // c.bs) for n in c.kv_lens]
    nb = sum(owned) + spare
    order = np.arange(nb) if identity else rng.permutation(nb)
    pages, at = [], 0
    for n in owned:
        pages.append(order[at:at + n])
        at += n
    table = np.full((B, c.max_blocks), order[at], dtype=np.int32)  # unused entries: a page nobody owns
    kpool = np.full((nb, LAYERS, c.bs, c.Hkv, c.D), POISON_K, dtype=np.float32)
    vpool = np.full((nb, LAYERS, c.bs, c.Hkv, c.D), POISON_V, dtype=np.float32)
    longest = max(max(c.kv_lens), 1)
    ks = seeded_normal((B, longest, c.Hkv, c.D), seed + 1, c.dt)
    vs = seeded_normal((B, longest, c.Hkv, c.D), seed + 2, c.dt)
    for b, n in enumerate(c.kv_lens):
        table[b, :owned[b]] = pages[b]
        for i, p in enumerate(pages[b]):
            rows = slice(i * c.bs, min((i + 1) * c.bs, n))
            kpool[p, LAYER, :rows.stop - rows.start] = ks[b, rows]
            vpool[p, LAYER, :rows.stop - rows.start] = vs[b, rows]
    cu = np.concatenate([[0], np.cumsum(c.q_lens)]).astype(np.int32)
    q = seeded_normal((int(cu[-1]) + EXTRA, c.H, c.D), seed, c.dt)
    return dict(q=q, kpool=kpool, vpool=vpool, table=table, cu=cu, ks=ks, vs=vs, pages=pages)


def oracle_rows(q, ks, vs, n_kv, causal):
    """[q_len, H, D] float64 of one sequence: q [q_len, H, D] over its first n_kv keys; no key -> 0"""
    q_len = q.shape[0]
    ref = np.zeros(q.shape)
    first = max(0, q_len - n_kv) if causal else 0  # bottom-right: rows before `first` see nothing
    if n_kv > 0 and q_len > first:
        ref[first:] = oatt.naive_attention(q[None, first:].transpose(0, 2, 1, 3), ks[None, :n_kv].transpose(0, 2, 1, 3),
                                           vs[None, :n_kv].transpose(0, 2, 1, 3), causal=causal)[0].transpose(1, 0, 2)
    return ref


def oracle_of(c: VCase, h):
    cu = h["cu"]
    ref = np.zeros((int(cu[-1]), c.H, c.D))
    for b, n in enumerate(c.kv_lens):
        ref[cu[b]:cu[b + 1]] = oracle_rows(h["q"][cu[b]:cu[b + 1]], h["ks"][b], h["vs"][b], n, c.causal)
    return ref


@functools.lru_cache(maxsize=None)
def prepared(name: str, identity: bool = False):
    """a case's layout and reference, computed once and shared (treated as read-only)"""
    c = CASES[name]
    seed = zlib.crc32(("varlen" + name).encode()) % 1000
    h = lay_out(c, seed, identity)
    h["ref"] = oracle_of(c, h)
    for a in h.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return h


def run_varlen(c: VCase, h, cu=None, lens=None, q=None, table=None):
    """the call on a case's layout; cu / lens / q / table override the case's own (a subset of its sequences)"""
    import pli_hip
    dev = lambda a: torch.from_numpy(np.array(a)).cuda().to(TDT[c.dt])  # noqa: E731 (a copy: the shared arrays are read-only)
    kpool, vpool = dev(h["kpool"]), dev(h["vpool"])
    i32 = lambda a: torch.from_numpy(np.array(a, dtype=np.int32)).cuda()  # noqa: E731
    qd = dev(h["q"] if q is None else q)
    out = torch.full_like(qd, SENTINEL)
    got = pli_hip.attn_varlen_paged(qd, kpool[:, LAYER], vpool[:, LAYER], i32(h["table"] if table is None else table),
                                    i32(c.kv_lens if lens is None else lens), i32(h["cu"] if cu is None else cu),
                                    max_kv=max_kv_of(c), causal=c.causal, out=out)
    assert got is out
    return out, pli_hip.last_route()


@pytest.mark.parametrize("name", CASES)
def test_varlen_vs_oracle(name):
    c, h = CASES[name], prepared(name)
    out, route = run_varlen(c, h)
    assert route == c.route, route
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


def test_routes_and_blind_rows():
    assert all(CASES[k].route == FAST for k in "1234568") and all(CASES[k].route == GENERIC for k in ("7a", "7b", "7c", "7d"))
    c = CASES["4"]
    assert c.q_lens == [20] and c.kv_lens == [12]  # the first 8 tokens' rows are exactly 0 (asserted above)
    assert any(ql > n for ql, n in zip(CASES["6"].q_lens, CASES["6"].kv_lens))  # and a blind sequence among the 128


def test_permutation_invariance():
    """case 1 under an identity and under a permuted table: same tiles, same arithmetic, only the addresses
    differ -- bitwise equal outputs"""
    c = CASES["1"]
    a, ra = run_varlen(c, prepared("1", identity=True))
    b, rb = run_varlen(c, prepared("1"))
    assert ra == rb == FAST
    assert not np.array_equal(prepared("1", identity=True)["table"], prepared("1")["table"])
    assert torch.equal(a, b), (a.float() - b.float()).abs().max().item()


def test_each_sequence_alone_is_bitwise_its_rows_in_the_batch():
    """every sequence starts its own tiles, so its arithmetic does not depend on its batch mates: run alone
    (batch 1, same pools, its own table row) it gives bitwise the rows it gets in the batch"""
    c, h = CASES["1"], prepared("1")
    full, _ = run_varlen(c, h)
    cu = h["cu"]
    for b, ql in enumerate(c.q_lens):
        q1 = np.concatenate([h["q"][cu[b]:cu[b + 1]], h["q"][-EXTRA:]])
        alone, route = run_varlen(c, h, cu=[0, ql], lens=[c.kv_lens[b]], q=q1, table=h["table"][b:b + 1])
        assert route == FAST
        assert torch.equal(alone[:ql], full[cu[b]:cu[b + 1]]), f"sequence {b}"
        assert (alone[ql:] == SENTINEL).all()


# ------------------------------------------------------------------ append --
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_append_matches_a_host_scatter(dt):
    import pli_hip
    Hkv, D, bs, mb, nb = 2, 64, 16, 2, 12
    torch.manual_seed(3)
    table_h = torch.randperm(nb)[:4 * mb].reshape(4, mb).to(torch.int32)
    table = table_h.cuda()
    # (q_lens, seq_lens after the step): across a page boundary, a fresh page, a sequence sitting out, one token;
    # then tokens past max_blocks * block_size = 32 and positions below 0 (seq_len < q_len) are dropped
    for q_lens, lens_h in (([5, 16, 0, 1], [18, 32, 7, 1]), ([6, 3, 2, 4], [35, 33, 32, 2])):
        kpool = torch.full((nb, LAYERS, bs, Hkv, D), POISON_K, device="cuda").to(TDT[dt])
        vpool = torch.full((nb, LAYERS, bs, Hkv, D), POISON_V, device="cuda").to(TDT[dt])
        cu_h = [0] + list(np.cumsum(q_lens))
        total = cu_h[-1]
        kn = torch.randn(total + EXTRA, Hkv, D, device="cuda").to(TDT[dt])
        vn = torch.randn_like(kn)
        want_k, want_v = kpool.clone(), vpool.clone()
        written = 0
        for b, ql in enumerate(q_lens):
            for i in range(ql):
                pos = lens_h[b] - ql + i
                if 0 <= pos < mb * bs:
                    want_k[table_h[b, pos // bs], LAYER, pos % bs] = kn[cu_h[b] + i]
                    want_v[table_h[b, pos // bs], LAYER, pos % bs] = vn[cu_h[b] + i]
                    written += 1
        lens = torch.tensor(lens_h, dtype=torch.int32, device="cuda")
        cu = torch.tensor(cu_h, dtype=torch.int32, device="cuda")
        pli_hip.kv_append_varlen_paged(kn, vn, kpool[:, LAYER], vpool[:, LAYER], table, lens, cu)
        assert pli_hip.last_route() == APPEND
        # every element of both pools: the scattered rows exactly, the poison (layer 0 too) intact everywhere else
        assert torch.equal(kpool, want_k) and torch.equal(vpool, want_v)
        assert int((kpool[:, LAYER, :, 0, 0].float() != POISON_K).sum()) == written
        assert lens.tolist() == lens_h and cu.tolist() == cu_h
        assert written == (total if lens_h[0] == 18 else 3 + 2 + 2 + 2)


# ------------------------------------------------------------ graph replay --
def test_graph_replay_with_a_different_mix():
    """one append + attend pair captured, then replayed after cu_seqlens_q, seq_lens and the table are rewritten in
    place to a different mix with the same batch and max_tokens: bitwise equal to eager, rows past the new cu[batch]
    untouched"""
    import pli_hip
    B, H, Hkv, D, bs, mb, nb, T = 4, 8, 2, 128, 16, 8, 40, 48
    dt = torch.bfloat16
    torch.manual_seed(11)
    pools = [torch.randn(nb, LAYERS, bs, Hkv, D, device="cuda").to(dt) for _ in range(2)]
    mixes = [  # (q_lens, seq_lens after the step); the second fills fewer packed rows than the first
        ([40, 1, 0, 7], [40, 100, 50, 64]),
        ([1, 20, 3, 1], [128, 33, 3, 17]),
    ]
    tables = [torch.randperm(nb)[:B * mb].reshape(B, mb).to(torch.int32).cuda() for _ in mixes]
    g_k, g_v = (p.clone() for p in pools)
    cu_s = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    lens_s = torch.zeros(B, dtype=torch.int32, device="cuda")
    table_s = torch.zeros(B, mb, dtype=torch.int32, device="cuda")
    q_s, kn_s, vn_s = (torch.zeros(T, h, D, device="cuda", dtype=dt) for h in (H, Hkv, Hkv))
    out_s = torch.empty(T, H, D, device="cuda", dtype=dt)

    def step(q, kn, vn, k, v, table, lens, cu, out):
        pli_hip.kv_append_varlen_paged(kn, vn, k[:, LAYER], v[:, LAYER], table, lens, cu)
        pli_hip.attn_varlen_paged(q, k[:, LAYER], v[:, LAYER], table, lens, cu, out=out)

    def load(i):
        q_lens, lens_h = mixes[i]
        cu_s.copy_(torch.tensor([0] + list(np.cumsum(q_lens)), dtype=torch.int32))
        lens_s.copy_(torch.tensor(lens_h, dtype=torch.int32))
        table_s.copy_(tables[i])
        return int(sum(q_lens))

    # warm-up on throwaway state (code objects loaded before the capture)
    load(0)
    step(q_s, kn_s, vn_s, pools[0].clone(), pools[1].clone(), table_s, lens_s, cu_s, torch.empty_like(out_s))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(q_s, kn_s, vn_s, g_k, g_v, table_s, lens_s, cu_s, out_s)
    assert torch.equal(g_k, pools[0])  # a capture runs nothing
    e_k, e_v = (p.clone() for p in pools)
    for i in (0, 1, 0):
        total = load(i)
        q, kn, vn = (torch.randn(T, h, D, device="cuda").to(dt) for h in (H, Hkv, Hkv))
        q_s.copy_(q), kn_s.copy_(kn), vn_s.copy_(vn)
        out_s.fill_(SENTINEL)
        out_e = torch.full_like(out_s, SENTINEL)
        step(q, kn, vn, e_k, e_v, table_s, lens_s, cu_s, out_e)
        assert pli_hip.last_route() == FAST
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_s, out_e), f"replay of mix {i}"
        assert (out_s[total:] == SENTINEL).all() and not (out_s[:total] == SENTINEL).all()
        assert torch.equal(g_k, e_k) and torch.equal(g_v, e_v)
    assert not torch.equal(g_k, pools[0])


# ---------------------------------------------------------- PagedKVCache --
def test_paged_kv_cache_packed_step():
    """three requests (histories 30, 17, 9) grown by [40, 1, 0] tokens in one packed step through extend_blocks /
    tables_packed / append_packed / attend_packed, on both layers, against the oracle over each request's history"""
    from ch07 import PagedKVCache
    H, Hkv, D, bs = 8, 2, 64, 16
    cache = PagedKVCache(num_blocks=12, block_size=bs, num_layers=LAYERS, num_heads=Hkv, head_dim=D,
                         dtype=torch.bfloat16, device="cuda")
    bf = lambda a: torch.from_numpy(a).cuda().bfloat16()  # noqa: E731
    seeds = iter(range(30_000, 31_000))
    rids, hist_n, grow = [5, 6, 7], [30, 17, 9], [40, 1, 0]
    hist = {}
    for rid, n in zip(rids, hist_n):  # the histories go in as one packed prompt step
        cache.allocate_blocks(rid, n)
    table, lens, cu = cache.tables_packed(rids, hist_n)
    assert lens.tolist() == hist_n and cu.tolist() == [0, 30, 47, 56]
    cu_h = cu.tolist()
    for layer in range(LAYERS):
        k, v = (seeded_normal((56, Hkv, D), next(seeds), "bf16") for _ in range(2))
        cache.append_packed(layer, bf(k), bf(v), table, lens, cu)
        for i, rid in enumerate(rids):
            hist[rid, layer] = (k[cu_h[i]:cu_h[i + 1]], v[cu_h[i]:cu_h[i + 1]])
    for rid, n in zip(rids, grow):
        cache.extend_blocks(rid, n)
    table, lens, cu = cache.tables_packed(rids, grow, max_blocks=5)
    assert table.shape == (3, 5) and lens.tolist() == [70, 18, 9] and cu.tolist() == [0, 40, 41, 41]
    cu_h, lens_h, worst = cu.tolist(), lens.tolist(), 0.0
    for layer in range(LAYERS):
        q, k, v = (seeded_normal((41, s, D), next(seeds), "bf16") for s in (H, Hkv, Hkv))
        cache.append_packed(layer, bf(k), bf(v), table, lens, cu)
        out = cache.attend_packed(layer, bf(q), table, lens, cu).float().cpu().numpy()
        assert out.shape == (41, H, D)
        for i, rid in enumerate(rids):
            rows = slice(cu_h[i], cu_h[i + 1])
            ks = np.concatenate([hist[rid, layer][0], k[rows]])
            vs = np.concatenate([hist[rid, layer][1], v[rows]])
            assert ks.shape[0] == lens_h[i]
            worst = max(worst, np.abs(out[rows] - oracle_rows(q[rows], ks, vs, ks.shape[0], True)).max(initial=0.0))
    assert worst <= TOL["bf16"], f"max |err| {worst:.3e}"
