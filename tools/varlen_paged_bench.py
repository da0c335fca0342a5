#!/usr/bin/env python3
"""Packed variable-length paged attention against what the library could do
for the same work before it, in one process.

    python tools/varlen_paged_bench.py [--shapes a,b,c] [--out FILE]

Shapes (32 q / 8 kv heads, D 128, bf16, block size 16, permuted tables):
  a  chunked prefill: one request, 512 new tokens over 32k keys
  b  mixed: 4 requests x 256 new tokens over 4k keys + 60 decoding requests
     at 4k keys
  c  decode only: 8 requests x 32k keys (the shape of paged_decode_bench.py)

Legs, timed with device events, warmed, alternating (leg 1, 2, 3, 1, 2, 3, ..):
  varlen        pli_hip.attn_varlen_paged, one launch for the whole step
  generic       a, b: pli_hip.attn_decode_paged once per distinct n_q (the
                prompt chunks take attn_decode_paged_generic)
  gather_flash  a, b: per prefilling request, gather its pages into a
                contiguous tensor and run pli_hip.flash_attn_fwd(causal);
                attn_decode_paged for the decoding requests
  decode        c: pli_hip.attn_decode_paged

Prints ONE JSON line: per shape and leg the median time per step, the spread
over the repeats ((max - min) / median), the routes, the ratios other / varlen
(> 1: the single launch is faster) with whether the difference exceeds both
legs' spreads, and the largest difference between the legs' outputs.  There is
no CPU path: without a ROCm device the tool fails.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "physics-llm-inference_amd"))

import torch  # noqa: E402

import pli_hip  # noqa: E402

H, HKV, D, BS = 32, 8, 128, 16
DT, DEV = torch.bfloat16, "cuda"

SHAPES = {  # (q_lens, kv_lens after the step)
    "a": ([512], [32768]),
    "b": ([256] * 4 + [1] * 60, [4096] * 64),
    "c": ([1] * 8, [32768] * 8),
}


def timed(fn, iters: int) -> float:
    """seconds per call over `iters` back-to-back calls, device events"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / iters


def build(name: str):
    """the step's tensors and its legs: {leg: (callable, output [tokens, H, D])}"""
    q_lens, kv_lens = SHAPES[name]
    B, T = len(q_lens), sum(q_lens)
    per_seq = [n // BS for n in kv_lens]
    assert all(n % BS == 0 for n in kv_lens)
    nb, mb = sum(per_seq), max(per_seq)
    g = torch.Generator(device="cpu").manual_seed(ord(name))
    torch.manual_seed(ord(name))
    k_pool = torch.randn(nb, BS, HKV, D, device=DEV).to(DT)
    v_pool = torch.randn(nb, BS, HKV, D, device=DEV).to(DT)
    q = torch.randn(T, H, D, device=DEV).to(DT)
    perm = torch.randperm(nb, generator=g).to(torch.int32)
    table_h = torch.zeros(B, mb, dtype=torch.int32)
    at = 0
    for b, n in enumerate(per_seq):
        table_h[b, :n] = perm[at:at + n]
        table_h[b, n:] = perm[at + n - 1]
        at += n
    table = table_h.to(DEV)
    lens = torch.tensor(kv_lens, dtype=torch.int32, device=DEV)
    cu_h = [0]
    for n in q_lens:
        cu_h.append(cu_h[-1] + n)
    cu = torch.tensor(cu_h, dtype=torch.int32, device=DEV)
    outs = {}

    def out_of(leg):
        outs[leg] = torch.zeros(T, H, D, device=DEV, dtype=DT)
        return outs[leg]

    legs = {}
    o_v = out_of("varlen")
    legs["varlen"] = lambda: pli_hip.attn_varlen_paged(q, k_pool, v_pool, table, lens, cu, out=o_v)

    # groups of sequences with the same n_q, each a contiguous run of the packed rows: [B', n_q, H, D] views
    groups, b0 = [], 0
    while b0 < B:
        b1 = b0
        while b1 < B and q_lens[b1] == q_lens[b0]:
            b1 += 1
        groups.append((b0, b1, q_lens[b0]))
        b0 = b1

    def view(t, b0, b1, n_q):
        return t[cu_h[b0]:cu_h[b1]].view(b1 - b0, n_q, H, D)

    def paged_call(out, b0, b1, n_q):
        ws = torch.empty(max(pli_hip.attn_decode_paged_workspace_bytes(b1 - b0, H, HKV, n_q, mb * BS, D) // 4, 1), device=DEV)
        qq, oo, tt, ll = view(q, b0, b1, n_q), view(out, b0, b1, n_q), table[b0:b1].contiguous(), lens[b0:b1].contiguous()
        return lambda: pli_hip.attn_decode_paged(qq, k_pool, v_pool, tt, ll, out=oo, workspace=ws)

    def gather_flash_call(out, b):
        pages = table[b, :per_seq[b]].long()
        qq = q[cu_h[b]:cu_h[b + 1]].unsqueeze(0).permute(0, 2, 1, 3)          # [1, H, n_q, D] view
        oo = out[cu_h[b]:cu_h[b + 1]].unsqueeze(0).permute(0, 2, 1, 3)

        def run():
            kc = k_pool[pages].view(1, kv_lens[b], HKV, D).permute(0, 2, 1, 3)  # the copy the pool exists to avoid
            vc = v_pool[pages].view(1, kv_lens[b], HKV, D).permute(0, 2, 1, 3)
            pli_hip.flash_attn_fwd(qq, kc, vc, causal=True, out=oo)
        return run

    if name == "c":
        legs["decode"] = paged_call(out_of("decode"), 0, B, 1)
    else:
        o_g = out_of("generic")
        calls = [paged_call(o_g, *grp) for grp in groups]
        legs["generic"] = lambda: [c() for c in calls]
        o_f = out_of("gather_flash")
        calls_f = [gather_flash_call(o_f, b) for b0, b1, n_q in groups if n_q > 1 for b in range(b0, b1)]
        calls_f += [paged_call(o_f, *grp) for grp in groups if grp[2] == 1]
        legs["gather_flash"] = lambda: [c() for c in calls_f]
    return legs, outs, dict(batch=B, tokens=T, q_lens=sorted(set(q_lens)), keys=kv_lens[0], launch_groups=len(groups))


def one_shape(a, name: str) -> dict:
    legs, outs, info = build(name)
    routes, iters = {}, {}
    for leg, fn in legs.items():  # warm-up: code objects, allocator, clocks; and the size of a timed window
        fn()
        routes[leg] = pli_hip.last_route()
        torch.cuda.synchronize()
        est = timed(fn, 2)
        iters[leg] = max(2, min(a.max_iters, int(a.window / max(est, 1e-7))))
        timed(fn, max(2, iters[leg] // 4))
    times = {leg: [] for leg in legs}
    for _ in range(a.repeats):
        for leg, fn in legs.items():
            times[leg].append(timed(fn, iters[leg]))
    res = dict(info, routes=routes, iters=iters)
    for leg, t in times.items():
        med = statistics.median(t)
        res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4)}
    for leg in legs:
        if leg == "varlen":
            continue
        ratio = res[leg]["us"] / res["varlen"]["us"]
        margin = max(res[leg]["spread"], res["varlen"]["spread"])
        res[f"{leg}_over_varlen"] = round(ratio, 4)
        res[f"{leg}_vs_varlen"] = ("varlen faster" if ratio > 1 + margin else "varlen slower" if ratio < 1 - margin
                                   else "within the spread")
        res[f"max_abs_diff_{leg}"] = float((outs[leg].float() - outs["varlen"].float()).abs().max())
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--max-iters", type=int, default=2000, help="cap on calls per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per leg, alternating")
    ap.add_argument("--out", help="also append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("varlen_paged_bench: no ROCm device (there is no CPU path)", file=sys.stderr)
        return 1
    result = {"tool": "varlen_paged_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16",
              "heads": [H, HKV], "D": D, "block_size": BS, "repeats": a.repeats, "window_s": a.window,
              "shapes": {s: one_shape(a, s) for s in a.shapes.split(",")}}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
