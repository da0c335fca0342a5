"""GPU parity of paged decode attention (pli_attn_decode_paged), the paged
append (pli_kv_append_paged) and ch07.PagedKVCache's device half.

Oracle: each sequence's pages are gathered on the host with numpy and
oracle.attention.naive_attention runs in float64 on the same rounded inputs.
Tolerance: the project's own (tests/test_gpu_decode.py), 1e-2 for bf16 / fp16
outputs, 1e-3 for fp32.

Every case is laid out so that a wrong lookup or a missing mask shows as a
large error: tables are random permutations of a pool with more pages than
the sequences own; every page no sequence owns, the tail of every last page,
the whole of the layer the test does not attend over, and (through a spare
page) every unused table entry hold K = 300, V = 1e4 (as
test_decode_reads_cache_in_place_and_ignores_stale_tail does).  The pools
have the reference's 5-D layout with two layers and the test attends over
layer 1, so the page stride is exercised.  No table entry is out of range.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np
import pytest
import torch

from oracle import attention as oatt
from oracle.numerics import seeded_normal
from paged_cases import CASES, COMBINE, FAST, GENERIC, Case, max_kv_of

pytestmark = pytest.mark.gpu
TDT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
TOL = {"fp32": 1e-3, "fp16": 1e-2, "bf16": 1e-2}
POISON_K, POISON_V = 300.0, 1e4
LAYERS, LAYER = 2, 1


def lay_out(c: Case, seed: int, identity: bool = False, spare: int = 5):
    """host arrays of a case: q [B, Sq, H, D], the 5-D pools, the table, per-sequence K / V"""
    rng = np.random.default_rng(seed)
    owned = [-(-n // c.bs) for n in c.lens]
    nb = sum(owned) + spare
    order = np.arange(nb) if identity else rng.permutation(nb)
    pages, at = [], 0
    for n in owned:
        pages.append(order[at:at + n])
        at += n
    table = np.full((c.B, c.max_blocks), order[at], dtype=np.int32)  # unused entries: a page nobody owns
    kpool = np.full((nb, LAYERS, c.bs, c.Hkv, c.D), POISON_K, dtype=np.float32)
    vpool = np.full((nb, LAYERS, c.bs, c.Hkv, c.D), POISON_V, dtype=np.float32)
    longest = max(max(c.lens), 1)
    ks = seeded_normal((c.B, longest, c.Hkv, c.D), seed + 1, c.dt)
    vs = seeded_normal((c.B, longest, c.Hkv, c.D), seed + 2, c.dt)
    for b, n in enumerate(c.lens):
        table[b, :owned[b]] = pages[b]
        for i, p in enumerate(pages[b]):
            rows = slice(i * c.bs, min((i + 1) * c.bs, n))
            kpool[p, LAYER, :rows.stop - rows.start] = ks[b, rows]
            vpool[p, LAYER, :rows.stop - rows.start] = vs[b, rows]
    q = seeded_normal((c.B, c.Sq, c.H, c.D), seed, c.dt)
    return dict(q=q, kpool=kpool, vpool=vpool, table=table, ks=ks, vs=vs, pages=pages)


def oracle_of(c: Case, q, ks, vs, causal=True):
    """[B, Sq, H, D] float64: naive attention per sequence over its own length; no key -> 0"""
    ref = np.zeros((c.B, c.Sq, c.H, c.D))
    for b, n in enumerate(c.lens):
        if n > 0:
            ref[b] = oatt.naive_attention(q[b:b + 1].transpose(0, 2, 1, 3), ks[b:b + 1, :n].transpose(0, 2, 1, 3),
                                          vs[b:b + 1, :n].transpose(0, 2, 1, 3), causal=causal)[0].transpose(1, 0, 2)
    return ref


@functools.lru_cache(maxsize=None)
def prepared(name: str, identity: bool = False):
    """a case's layout and reference, computed once and shared (treated as read-only)"""
    c = CASES[name]
    seed = zlib.crc32(name.encode()) % 1000
    h = lay_out(c, seed, identity)
    h["ref"] = oracle_of(c, h["q"], h["ks"], h["vs"])
    for a in h.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return h


def run_paged(c: Case, h, **kw):
    import pli_hip
    dev = lambda a: torch.from_numpy(np.array(a)).cuda().to(TDT[c.dt])  # noqa: E731 (a copy: the shared arrays are read-only)
    kpool, vpool = dev(h["kpool"]), dev(h["vpool"])
    table = torch.from_numpy(np.array(h["table"])).cuda()
    lens = torch.tensor(c.lens, dtype=torch.int32, device="cuda")
    out = pli_hip.attn_decode_paged(dev(h["q"]), kpool[:, LAYER], vpool[:, LAYER], table, lens, max_kv=max_kv_of(c), **kw)
    return out, pli_hip.last_route()


@pytest.mark.parametrize("name", CASES)
def test_paged_vs_oracle(name):
    c, h = CASES[name], prepared(name)
    out, route = run_paged(c, h)
    assert route == c.route, route
    assert out.shape == (c.B, c.Sq, c.H, c.D) and out.dtype == TDT[c.dt]
    got = out.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - h["ref"]).max()
    print(f"case {name}: route {route}, max |err| {err:.3e} (tolerance {TOL[c.dt]:g})")
    assert err <= TOL[c.dt], f"max |err| {err:.3e}"
    for b, n in enumerate(c.lens):
        if n == 0:
            assert not got[b].any(), "an empty sequence's rows are 0"


def test_routes_cover_the_three_kernels():
    assert {c.route for c in CASES.values()} == {FAST, COMBINE, GENERIC}
    assert all(CASES[k].route != GENERIC for k in "123456") and all(CASES[k].route == GENERIC for k in ("7a", "7b", "7c", "7d"))


def test_permutation_invariance():
    """case 4 (split-K, empty chunks) under an identity and under a permuted table: same plan, same arithmetic,
    only the addresses differ -- bitwise equal outputs"""
    c = CASES["4"]
    a, ra = run_paged(c, prepared("4", identity=True))
    b, rb = run_paged(c, prepared("4"))
    assert ra == rb == COMBINE
    assert not np.array_equal(prepared("4", identity=True)["table"], prepared("4")["table"])
    assert torch.equal(a, b), (a.float() - b.float()).abs().max().item()


def test_agrees_with_the_contiguous_kernel():
    """case 5 under an identity table against pli_hip.attn_decode per sequence on the same values; the bound is
    the one test_decode_split_invariance uses for two chunkings of one head"""
    import pli_hip
    c, h = CASES["5"], prepared("5", identity=True)
    out, _ = run_paged(c, h)
    worst = 0.0
    for b, n in enumerate(c.lens):
        pages = h["pages"][b]
        assert (np.diff(pages) == 1).all()
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[pages[0]:pages[-1] + 1, LAYER])).cuda().to(  # noqa: E731
            TDT[c.dt]).reshape(1, len(pages) * c.bs, c.Hkv, c.D)
        q = torch.from_numpy(np.array(h["q"][b:b + 1])).cuda().to(TDT[c.dt])
        ref = pli_hip.attn_decode(q, dev(h["kpool"]), dev(h["vpool"]), n, causal=True)
        assert pli_hip.last_route().startswith("attn_decode_chunk")
        worst = max(worst, (out[b:b + 1].float() - ref.float()).abs().max().item())
    assert worst <= 2 ** -7, f"max |paged - contiguous| {worst:.3e} (bound 2^-7 = {2 ** -7:.3e})"


def test_unused_entries_may_hold_any_valid_page():
    """unused table entries may hold anything in range; here they hold the last valid page index and page 0"""
    c, h = CASES["1"], dict(prepared("1"))
    for fill in (0, h["kpool"].shape[0] - 1):
        t = np.array(h["table"])
        for b, n in enumerate(c.lens):
            t[b, -(-n // c.bs):] = fill
        out, _ = run_paged(c, dict(h, table=t))
        assert np.abs(out.float().cpu().numpy() - h["ref"]).max() <= TOL[c.dt]


# ------------------------------------------------------------------ append --
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("n_new", [1, 5])
def test_append_matches_a_host_scatter(n_new, dt):
    import pli_hip
    B, Hkv, D, bs, mb, nb = 3, 2, 64, 16, 2, 9
    torch.manual_seed(n_new)
    kpool = torch.randn(nb, LAYERS, bs, Hkv, D, device="cuda").to(TDT[dt])
    vpool = torch.randn_like(kpool)
    table_h = torch.randperm(nb)[:B * mb].reshape(B, mb).to(torch.int32)
    table = table_h.cuda()
    kn = torch.randn(B, n_new, Hkv, D, device="cuda").to(TDT[dt])
    vn = torch.randn_like(kn)
    # [15, 16, 0]: across a page boundary, the start of a fresh page, an empty sequence;
    # [30, 31, 32]: tokens past max_blocks * block_size = 32 are dropped
    for lens_h in ([15, 16, 0], [30, 31, 32]):
        lens = torch.tensor(lens_h, dtype=torch.int32, device="cuda")
        want_k, want_v = kpool.clone(), vpool.clone()
        written = 0
        for b in range(B):
            for t in range(n_new):
                pos = lens_h[b] + t
                if pos < mb * bs:
                    want_k[table_h[b, pos // bs], LAYER, pos % bs] = kn[b, t]
                    want_v[table_h[b, pos // bs], LAYER, pos % bs] = vn[b, t]
                    written += 1
        pli_hip.kv_append_paged(kn, vn, kpool[:, LAYER], vpool[:, LAYER], table, lens)
        assert pli_hip.last_route() == "kv_append_paged_kernel"
        # every element of both pools: the scattered rows exactly, everything else (layer 0 too) unchanged
        assert torch.equal(kpool, want_k) and torch.equal(vpool, want_v)
        assert lens.tolist() == lens_h  # the lengths are the caller's to advance
        assert written == (B * n_new if lens_h[0] == 15 else sum(max(0, min(n_new, 32 - n)) for n in lens_h))


# ---------------------------------------------------------- PagedKVCache --
def test_paged_kv_cache_end_to_end():
    """three requests (prompts 5, 16, 40), 20 decode steps of extend_blocks / tables / append / attend on both
    layers against the oracle over each request's history; request 2 is freed half-way and a fourth request takes
    over one of its pages, whose old contents past the new request's length must stay unseen"""
    from ch07 import PagedKVCache
    H, Hkv, D, bs = 4, 2, 64, 16
    cache = PagedKVCache(num_blocks=8, block_size=bs, num_layers=LAYERS, num_heads=Hkv, head_dim=D,
                         dtype=torch.bfloat16, device="cuda")
    assert cache.k_cache.shape == (8, LAYERS, bs, Hkv, D) and cache.k_cache.dtype == torch.bfloat16
    cache.allocate_blocks(0, 1)  # holds the one page the requests below never need before step 15
    hist = {}                    # (rid, layer) -> ([k rows], [v rows]) float32, bf16-rounded
    seeds = iter(range(10_000, 20_000))
    bf = lambda a: torch.from_numpy(a).cuda().bfloat16()  # noqa: E731

    def prompt(rid, n):
        cache.allocate_blocks(rid, n)
        table, lens = cache.tables([rid])
        assert table.is_cuda and table.dtype == torch.int32 and lens.tolist() == [n]
        for layer in range(LAYERS):
            k, v = (seeded_normal((1, n, Hkv, D), next(seeds), "bf16") for _ in range(2))
            cache.append(layer, bf(k), bf(v), table, lens)
            hist[rid, layer] = ([k[0]], [v[0]])

    for rid, n in ((1, 5), (2, 16), (3, 40)):
        prompt(rid, n)
    active, worst = [1, 2, 3], 0.0
    for step in range(20):
        if step == 10:
            old = set(cache.block_tables[2].block_indices)
            assert cache.get_num_free_blocks() == 0 and cache.free_blocks_for_request(2) == 2
            prompt(4, 7)
            assert set(cache.block_tables[4].block_indices) <= old  # a page request 2 wrote, stale past 7 tokens
            active = [1, 3, 4]
        if step == 15:
            cache.free_blocks_for_request(0)
        for rid in active:
            cache.extend_blocks(rid, 1)
        table, lens = cache.tables(active, max_blocks=4)
        n_tok = [cache.block_tables[r].num_tokens for r in active]
        assert lens.tolist() == n_tok and table.shape == (3, 4)
        for layer in range(LAYERS):
            q, k, v = (seeded_normal((3, 1, s, D), next(seeds), "bf16") for s in (H, Hkv, Hkv))
            cache.append(layer, bf(k), bf(v), table, lens)
            out = cache.attend(layer, bf(q), table, lens).float().cpu().numpy()
            for i, rid in enumerate(active):
                hist[rid, layer][0].append(k[i])
                hist[rid, layer][1].append(v[i])
                ks, vs = (np.concatenate(x)[None].transpose(0, 2, 1, 3) for x in hist[rid, layer])
                assert ks.shape[2] == n_tok[i]
                ref = oatt.naive_attention(q[i:i + 1].transpose(0, 2, 1, 3), ks, vs, causal=True)
                worst = max(worst, np.abs(out[i:i + 1].transpose(0, 2, 1, 3) - ref).max())
    assert worst <= TOL["bf16"], f"max |err| over 20 steps {worst:.3e}"
    assert [cache.block_tables[r].num_tokens for r in (1, 3, 4)] == [25, 60, 17]
    assert cache.get_num_free_blocks() == 0


# ------------------------------------------------------------ graph replay --
def test_graph_replay_across_page_boundaries():
    """kv_append_paged + attn_decode_paged(n_kv_add=1) + seq_lens.add_(1) captured once and replayed 20 times from
    lengths [14, 31]: both sequences cross page boundaries during replay, through table entries written beforehand;
    every replay equals the eager calls bitwise"""
    import pli_hip
    B, H, Hkv, D, bs, mb, nb, steps = 2, 8, 2, 128, 16, 16, 40, 20
    torch.manual_seed(7)
    dt = torch.bfloat16
    table = torch.randperm(nb)[:B * mb].reshape(B, mb).to(torch.int32).cuda()  # persistent, every page assigned
    start = torch.tensor([14, 31], dtype=torch.int32, device="cuda")
    pools = [torch.randn(nb, LAYERS, bs, Hkv, D, device="cuda").to(dt) for _ in range(2)]
    g_k, g_v = (p.clone() for p in pools)
    e_k, e_v = (p.clone() for p in pools)
    g_lens, e_lens = start.clone(), start.clone()
    q_s, kn_s, vn_s = (torch.zeros(B, 1, h, D, device="cuda", dtype=dt) for h in (H, Hkv, Hkv))
    out_s = torch.empty(B, 1, H, D, device="cuda", dtype=dt)
    ws_bytes = pli_hip.attn_decode_paged_workspace_bytes(B, H, Hkv, 1, mb * bs, D)
    assert ws_bytes > 0  # 256 keys over 4 (batch, kv head) pairs: split-K, so the combine kernel is in the graph
    ws = torch.empty(ws_bytes // 4, device="cuda", dtype=torch.float32)

    def step(q, kn, vn, k, v, lens, out):
        pli_hip.kv_append_paged(kn, vn, k[:, LAYER], v[:, LAYER], table, lens)
        pli_hip.attn_decode_paged(q, k[:, LAYER], v[:, LAYER], table, lens, n_kv_add=1, out=out, workspace=ws)
        lens.add_(1)

    # warm-up on throwaway state (code objects loaded before the capture)
    step(q_s, kn_s, vn_s, pools[0].clone(), pools[1].clone(), start.clone(), torch.empty_like(out_s))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(q_s, kn_s, vn_s, g_k, g_v, g_lens, out_s)
    assert g_lens.tolist() == [14, 31]  # a capture runs nothing
    out_e = torch.empty_like(out_s)
    for i in range(steps):
        q, kn, vn = (torch.randn(B, 1, h, D, device="cuda").to(dt) for h in (H, Hkv, Hkv))
        step(q, kn, vn, e_k, e_v, e_lens, out_e)
        assert pli_hip.last_route() == COMBINE
        q_s.copy_(q), kn_s.copy_(kn), vn_s.copy_(vn)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_s, out_e), f"replay {i}"
        assert g_lens.tolist() == e_lens.tolist() == [15 + i, 32 + i]
    assert torch.equal(g_k, e_k) and torch.equal(g_v, e_v)
    assert not torch.equal(g_k, pools[0])
