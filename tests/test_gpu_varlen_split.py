"""GPU parity of split-K packed variable-length paged attention
(pli_attn_varlen_paged_ws / pli_attn_varlen_paged_fp8_ws: attn_varlen_paged_split
[_fp8] + attn_varlen_paged_combine) and ch07.PagedKVCache's workspace path.

Layouts, oracle and tolerance are those of tests/test_gpu_varlen_paged.py (16-bit
pools: float64 naive attention over the gathered pages, 1e-2 for bf16 / fp16) and
tests/test_gpu_fp8_kv.py (fp8 pools: the same oracle over the dequantised pool,
the same tolerance); the cases are tests/varlen_cases.py's plus boundary cases
of the chunking.  A merged row differs from the plain call's by fp32 rounding in
the merge only, so the tolerance is not widened.  Every call carries three
sentinel rows past cu[batch], which must stay untouched.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np
import pytest
import torch

import test_gpu_fp8_kv as f8
import test_gpu_varlen_paged as vp
from oracle.numerics import seeded_normal
from varlen_cases import CASES, FAST, GENERIC, VCase, max_kv_of

pytestmark = pytest.mark.gpu
TDT, TOL, EXTRA, SENTINEL, LAYERS, LAYER = vp.TDT, vp.TOL, vp.EXTRA, vp.SENTINEL, vp.LAYERS, vp.LAYER
POOLS = ("bf16", "fp8")  # "bf16": pools of q's 16-bit type
SPLIT = {"bf16": "attn_varlen_paged_split+attn_varlen_paged_combine",
         "fp8": "attn_varlen_paged_split_fp8+attn_varlen_paged_combine"}
PLAIN = {"bf16": {FAST: FAST, GENERIC: GENERIC}, "fp8": f8.VARLEN_ROUTE}

BOUNDARY = {
    # row i's limit is 96 + i: rows 0-31 see nothing of chunk [128, 160), an empty last chunk inside a live tile
    "b1": VCase(2, 2, 16, 64, "bf16", [64], [160], 10, True, FAST),
    # tokens 0-7 see nothing of [128, 136)
    "b2": VCase(8, 2, 16, 128, "bf16", [16], [136], 9, True, FAST),
    # kv = 128 exactly: no trailing chunk; kv = 129: a one-key chunk
    "b3": VCase(8, 2, 16, 128, "fp16", [3, 1], [128, 128], 8, True, FAST),
    "b4": VCase(8, 2, 16, 128, "fp16", [3, 1], [129, 129], 9, True, FAST),
    # a sequence that sits the step out, and one with tokens and no key, beside split ones
    "b5": VCase(8, 2, 16, 64, "bf16", [1, 0, 5, 2], [300, 200, 0, 130], 19, True, FAST),
    # b1 without the causal mask
    "b6": VCase(2, 2, 16, 64, "bf16", [64], [160], 10, False, FAST),
}


def case_of(name) -> VCase:
    return CASES[name] if name in CASES else BOUNDARY[name]


def make(c: VCase, pool: str, seed: int):
    """a case's host layout with its float64 reference, for 16-bit or fp8 pools"""
    if pool == "bf16":
        h = vp.lay_out(c, seed)
        h["ref"] = vp.oracle_of(c, h)
        return h
    h = f8.lay_out(c.bs, c.Hkv, c.D, c.kv_lens, c.max_blocks, seed)
    cu = np.concatenate([[0], np.cumsum(c.q_lens)]).astype(np.int32)
    h["cu"] = cu
    h["q"] = seeded_normal((int(cu[-1]) + EXTRA, c.H, c.D), seed, c.dt)
    h["ref"] = np.zeros((int(cu[-1]), c.H, c.D))
    for b, n in enumerate(c.kv_lens):
        h["ref"][cu[b]:cu[b + 1]] = vp.oracle_rows(h["q"][cu[b]:cu[b + 1]], h["kd"][b], h["vd"][b], n, c.causal)
    return h


@functools.lru_cache(maxsize=None)
def prepared(name: str, pool: str):
    """computed once and shared (read-only); the existing cases reuse the existing tests' layouts and references"""
    if name in CASES:
        return vp.prepared(name) if pool == "bf16" else f8.prepared_varlen(name)
    return f8.freeze(make(BOUNDARY[name], pool, zlib.crc32(("split" + name).encode()) % 1000))


def run(c: VCase, h, pool: str, split_keys=None, fill=float("nan"), cu=None, lens=None, q=None, table=None, max_kv=None):
    """split_keys None: the plain call; an int: the _ws call over a workspace of exactly the size asked for,
    pre-filled with `fill`.  cu / lens / q / table override the case's own.  -> (out, route)"""
    import pli_hip
    i32 = lambda a: torch.from_numpy(np.array(a, dtype=np.int32)).cuda()  # noqa: E731
    qd = torch.from_numpy(np.array(h["q"] if q is None else q)).cuda().to(TDT[c.dt])
    table, lens, cu = (i32(h["table"] if table is None else table), i32(c.kv_lens if lens is None else lens),
                       i32(h["cu"] if cu is None else cu))
    max_kv = max_kv_of(c) if max_kv is None else max_kv
    out = torch.full_like(qd, SENTINEL)
    kw = dict(max_kv=max_kv, causal=c.causal, out=out)
    if split_keys is not None:
        need = pli_hip.attn_varlen_paged_workspace_bytes(len(lens), qd.shape[0], c.H, c.Hkv, max_kv, c.D, split_keys)
        assert need % 16 == 0
        kw.update(workspace=torch.full((max(need // 4, 1),), fill, device="cuda"), split_keys=split_keys)
    if pool == "bf16":
        dev = lambda a: torch.from_numpy(np.array(a)).cuda().to(TDT[c.dt])  # noqa: E731
        got = pli_hip.attn_varlen_paged(qd, dev(h["kpool"])[:, LAYER], dev(h["vpool"])[:, LAYER], table, lens, cu, **kw)
    else:
        kp, vpl, _, ksc, vsc = f8.on_gpu(h)
        got = pli_hip.attn_varlen_paged_fp8(qd, kp, vpl, table, lens, cu, ksc, vsc, **kw)
    assert got is out
    return out, pli_hip.last_route()


def check(c: VCase, h, out):
    total = int(h["cu"][-1])
    assert out.shape == (total + EXTRA, c.H, c.D) and out.dtype == TDT[c.dt]
    got = out.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    assert (got[total:] == SENTINEL).all(), "rows past cu[batch] are not written"
    err = np.abs(got[:total] - h["ref"]).max(initial=0.0)
    print(f"max |err| {err:.3e} (tolerance {TOL[c.dt]:g})")
    assert err <= TOL[c.dt], f"max |err| {err:.3e}"
    if c.causal:
        for b, (ql, n) in enumerate(zip(c.q_lens, c.kv_lens)):
            blind = max(0, min(ql, ql - n))
            assert not got[h["cu"][b]:h["cu"][b] + blind].any(), "rows that see no key are exactly 0"
    return got


# ------------------------------------------------------- the existing cases --
@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("split_keys", [64, 128])
@pytest.mark.parametrize("name", ["1", "2", "3", "4", "5", "6", "8"])
def test_existing_fast_cases_split(name, split_keys, pool):
    import pli_hip
    c, h = CASES[name], prepared(name, pool)
    span, splits = pli_hip.attn_varlen_paged_split_plan(len(c.q_lens), int(h["cu"][-1]) + EXTRA, c.H, c.Hkv, max_kv_of(c),
                                                       c.D, split_keys)
    assert span == split_keys and splits == -(-max_kv_of(c) // split_keys)
    out, route = run(c, h, pool, split_keys)
    assert route == (SPLIT[pool] if splits > 1 else PLAIN[pool][FAST]), route
    check(c, h, out)


def test_what_the_existing_cases_exercise():
    assert -(-max(CASES["1"].kv_lens) // 64) == 9  # case 1: 9 chunks of 64 keys
    assert CASES["4"].q_lens == [20] and CASES["4"].kv_lens == [12]  # blind rows, checked exactly 0 above
    assert CASES["5"].bs == 256 and CASES["5"].kv_lens == [1100]  # chunks of 64 / 128 inside pages; 5 pages walked
    assert len(CASES["6"].q_lens) == 128


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("name", ["7a", "7b", "7c", "7d"])
def test_generic_cases_through_the_ws_call(name, pool):
    c, h = CASES[name], prepared(name, pool)
    plain, route_p = run(c, h, pool)
    ws, route = run(c, h, pool, 64)
    assert route == route_p == PLAIN[pool][GENERIC]
    assert torch.equal(ws, plain)


# --------------------------------------------------------- boundary cases --
@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("name", BOUNDARY)
def test_boundary_cases(name, pool):
    c, h = BOUNDARY[name], prepared(name, pool)
    out, route = run(c, h, pool, 64)
    assert route == SPLIT[pool]
    got = check(c, h, out)
    if name == "b5":
        cu = h["cu"]
        assert cu[1] == cu[2] and not got[cu[2]:cu[3]].any()  # one sits out; the one without keys is written as 0


# ------------------------------------------------------- the plan's own choice --
@pytest.mark.parametrize("pool", POOLS)
def test_the_plans_own_span(pool):
    """split_keys = 0: the span comes from the plan call; decode rows at three lengths, one of them past the span"""
    import pli_hip
    H, Hkv, D, bs = 8, 2, 128, 16
    span_min, one = pli_hip.attn_varlen_paged_split_plan(3, 3 + EXTRA, H, Hkv, bs, D, 0)
    assert one == 1 and span_min % 64 == 0
    mb = (2 * span_min + 64) // bs
    span, splits = pli_hip.attn_varlen_paged_split_plan(3, 3 + EXTRA, H, Hkv, mb * bs, D, 0)
    assert splits > 1 and span % 64 == 0 and span < mb * bs
    c = VCase(H, Hkv, bs, D, "bf16", [1, 1, 1], [span // 2, span, span + 70], mb, True, FAST)
    h = make(c, pool, 321)
    out, route = run(c, h, pool, 0)
    assert route == SPLIT[pool]
    check(c, h, out)
    plain, _ = run(c, h, pool)
    assert torch.equal(out[:2], plain[:2]), "the rows within one span are the plain call's"
    assert (out[2].float() - plain[2].float()).abs().max() <= 2 * TOL["bf16"]


# ------------------------------------------------------- bitwise properties --
@pytest.mark.parametrize("pool", POOLS)
def test_bitwise_properties(pool):
    c, h = CASES["1"], prepared("1", pool)
    cu, K = h["cu"], 128
    chunks = [max(1, -(-n // K)) for n in c.kv_lens]  # an upper bound per sequence; 1: every tile has one chunk
    assert chunks == [5, 1, 1, 1, 2]
    plain, _ = run(c, h, pool)
    a, route = run(c, h, pool, K, fill=float("nan"))
    assert route == SPLIT[pool]
    for b in (1, 2):  # one-chunk tiles: the plain call's rows, bit for bit
        assert cu[b + 1] > cu[b] and torch.equal(a[cu[b]:cu[b + 1]], plain[cu[b]:cu[b + 1]]), f"sequence {b}"
    b2, _ = run(c, h, pool, K, fill=float("nan"))
    assert torch.equal(a, b2), "two calls are bitwise equal"
    z, _ = run(c, h, pool, K, fill=0.0)
    assert torch.equal(a, z), "the workspace's old contents do not matter"
    assert (a[int(cu[-1]):] == SENTINEL).all()
    for b, ql in enumerate(c.q_lens):  # each sequence alone: bitwise its rows in the batch
        q1 = np.concatenate([h["q"][cu[b]:cu[b + 1]], h["q"][-EXTRA:]])
        alone, _ = run(c, h, pool, K, cu=[0, ql], lens=[c.kv_lens[b]], q=q1, table=h["table"][b:b + 1])
        assert torch.equal(alone[:ql], a[cu[b]:cu[b + 1]]), f"sequence {b}"
        assert (alone[ql:] == SENTINEL).all()


# ------------------------------------------------------ PagedKVCache, graph replay --
def _cache(kv_dtype, nb, H_kv, D, bs=16):
    from ch07 import PagedKVCache
    kw = {} if kv_dtype is None else dict(kv_dtype=kv_dtype)
    return PagedKVCache(num_blocks=nb, block_size=bs, num_layers=LAYERS, num_heads=H_kv, head_dim=D,
                        dtype=torch.bfloat16, device="cuda", **kw)


def _fill(cache, seed):
    """random finite contents for both pools: normal values, or codes of magnitude 2^-3 .. 4 with a random sign"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    for p in (cache.k_cache, cache.v_cache):
        if p.dtype == torch.float8_e4m3fn:
            codes = torch.randint(0x20, 0x48, p.shape, device="cuda", generator=g, dtype=torch.uint8)
            sign = torch.randint(0, 2, p.shape, device="cuda", generator=g, dtype=torch.uint8) << 7
            p.view(torch.uint8).copy_(codes | sign)
        else:
            p.copy_(torch.randn(p.shape, device="cuda", generator=g).to(p.dtype))


def _pool_values(p):
    """float64 host values of a layer view of a pool (an fp8 pool's scales are 1 here)"""
    if p.dtype == torch.float8_e4m3fn:
        return f8.decode_table().double()[p.contiguous().view(torch.uint8).cpu().long()].numpy()
    return p.float().cpu().numpy().astype(np.float64)


def _span_of(cache, B, T, H, mb):
    import pli_hip
    return pli_hip.attn_varlen_paged_split_plan(B, T, H, cache.num_heads, mb * cache.block_size, cache.head_dim, 0)


@pytest.mark.parametrize("kv_dtype", [None, torch.float8_e4m3fn])
def test_graph_replay_with_a_different_mix(kv_dtype):
    """append_packed + attend_packed(workspace=) captured once, replayed after cu_seqlens_q, seq_lens and the table are
    rewritten in place to a different mix (other sequences split, other chunk counts): bitwise equal to eager"""
    import pli_hip
    B, H, Hkv, D, bs, T = 4, 8, 2, 128, 16, 48
    span_min, _ = pli_hip.attn_varlen_paged_split_plan(B, T, H, Hkv, bs, D, 0)
    mb = (2 * span_min + 128) // bs
    nb = B * mb + 8
    cache, eager = _cache(kv_dtype, nb, Hkv, D), _cache(kv_dtype, nb, Hkv, D)
    span, splits = _span_of(cache, B, T, H, mb)
    assert splits > 1
    torch.manual_seed(12)
    _fill(cache, 5), _fill(eager, 5)  # the histories: the same random pool contents in both
    assert torch.equal(cache.k_cache.view(torch.uint8), eager.k_cache.view(torch.uint8))
    mixes = [  # (q_lens, seq_lens after the step)
        ([40, 1, 0, 7], [40, 2 * span + 5, 50, span + 64]),
        ([1, 20, 3, 1], [span + 100, 33, 3, 17]),
    ]
    tables = [torch.randperm(nb)[:B * mb].reshape(B, mb).to(torch.int32).cuda() for _ in mixes]
    cu_s = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    lens_s = torch.zeros(B, dtype=torch.int32, device="cuda")
    table_s = torch.zeros(B, mb, dtype=torch.int32, device="cuda")
    q_s, kn_s, vn_s = (torch.zeros(T, h, D, device="cuda", dtype=torch.bfloat16) for h in (H, Hkv, Hkv))
    ws = cache.packed_workspace(B, T, H, max_blocks=mb)
    assert ws.numel() * 4 == pli_hip.attn_varlen_paged_workspace_bytes(B, T, H, Hkv, mb * bs, D) > 0
    ws_e = torch.full_like(ws, float("nan"))
    out_s = torch.empty(T, H, D, device="cuda", dtype=torch.bfloat16)

    def step(c, q, kn, vn, w):
        c.append_packed(LAYER, kn, vn, table_s, lens_s, cu_s)
        return c.attend_packed(LAYER, q, table_s, lens_s, cu_s, workspace=w)

    def load(i):
        q_lens, lens_h = mixes[i]
        cu_s.copy_(torch.tensor([0] + list(np.cumsum(q_lens)), dtype=torch.int32))
        lens_s.copy_(torch.tensor(lens_h, dtype=torch.int32))
        table_s.copy_(tables[i])
        return int(sum(q_lens))

    load(0)
    warm = _cache(kv_dtype, nb, Hkv, D)  # warm-up on throwaway state (code objects loaded before the capture)
    step(warm, q_s, kn_s, vn_s, torch.empty_like(ws))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s.copy_(step(cache, q_s, kn_s, vn_s, ws))
    for i in (0, 1, 0):
        total = load(i)
        q, kn, vn = (torch.randn(T, h, D, device="cuda").to(torch.bfloat16) for h in (H, Hkv, Hkv))
        q_s.copy_(q), kn_s.copy_(kn), vn_s.copy_(vn)
        out_e = step(eager, q, kn, vn, ws_e)
        assert pli_hip.last_route() == SPLIT["bf16" if kv_dtype is None else "fp8"]
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_s[:total], out_e[:total]), f"replay of mix {i}"
        assert torch.isfinite(out_s[:total].float()).all()
        assert torch.equal(cache.k_cache.view(torch.uint8), eager.k_cache.view(torch.uint8))


@pytest.mark.parametrize("kv_dtype", [None, torch.float8_e4m3fn])
def test_paged_kv_cache_packed_step_with_a_workspace(kv_dtype):
    """three requests with histories, one of them past the plan's span, grown in one packed step through
    packed_workspace / attend_packed(workspace=), against the oracle over what the pool holds"""
    import pli_hip
    H, Hkv, D, bs = 8, 2, 64, 16
    span_min, _ = pli_hip.attn_varlen_paged_split_plan(3, 8, H, Hkv, bs, D, 0)
    hist_n, grow = [span_min + 90, 17, 200], [5, 1, 2]
    mb = (2 * span_min + 128) // bs
    cache = _cache(kv_dtype, 3 * mb, Hkv, D)
    bf = lambda a: torch.from_numpy(a).cuda().bfloat16()  # noqa: E731
    rids = [5, 6, 7]
    for rid, n in zip(rids, hist_n):
        cache.allocate_blocks(rid, n)
    table, lens, cu = cache.tables_packed(rids, hist_n, max_blocks=mb)
    k, v = (seeded_normal((sum(hist_n), Hkv, D), s, "bf16") for s in (41, 42))
    cache.append_packed(LAYER, bf(k), bf(v), table, lens, cu)
    for rid, n in zip(rids, grow):
        cache.extend_blocks(rid, n)
    table, lens, cu = cache.tables_packed(rids, grow, max_blocks=mb)
    T = sum(grow)
    q, k, v = (seeded_normal((T, s, D), sd, "bf16") for s, sd in ((H, 43), (Hkv, 44), (Hkv, 45)))
    cache.append_packed(LAYER, bf(k), bf(v), table, lens, cu)
    ws = cache.packed_workspace(3, T, H, max_blocks=mb)
    assert ws.numel() * 4 == cache.packed_workspace_bytes(3, T, H, max_blocks=mb) > 0
    ws.fill_(float("nan"))
    out = cache.attend_packed(LAYER, bf(q), table, lens, cu, workspace=ws)
    assert pli_hip.last_route() == SPLIT["bf16" if kv_dtype is None else "fp8"]
    plain = cache.attend_packed(LAYER, bf(q), table, lens, cu)
    assert pli_hip.last_route() == PLAIN["bf16" if kv_dtype is None else "fp8"][FAST]
    got = out.float().cpu().numpy().astype(np.float64)
    kp, vpl = (_pool_values(p[:, LAYER]) for p in (cache.k_cache, cache.v_cache))
    cu_h, lens_h, worst = cu.tolist(), lens.tolist(), 0.0
    for i, rid in enumerate(rids):
        pages = cache.block_tables[rid].block_indices
        ks, vs = (p[pages].reshape(-1, Hkv, D)[:lens_h[i]] for p in (kp, vpl))
        rows = slice(cu_h[i], cu_h[i + 1])
        worst = max(worst, np.abs(got[rows] - vp.oracle_rows(q[rows], ks, vs, lens_h[i], True)).max(initial=0.0))
    print(f"max |err| {worst:.3e}")
    assert worst <= TOL["bf16"], f"max |err| {worst:.3e}"
    assert torch.equal(out[cu_h[1]:], plain[cu_h[1]:]), "requests within one span: the plain call's rows"
