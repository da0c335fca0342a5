#!/usr/bin/env python3
"""Paged decode attention against the contiguous kernel, in one process.

    python tools/paged_decode_bench.py [--out FILE]

Shape: the decode shape README quotes -- B 8, 32 q / 8 kv heads, 32k keys,
D 128, bf16 -- at block sizes 16 and 128.  Three legs per block size, timed
with device events, warmed, alternating (leg a, b, c, a, b, c, ...):

  paged_permuted    pli_hip.attn_decode_paged over a randomly permuted table
  paged_identity    the same kernel over the identity table
  contiguous        pli_hip.attn_decode on a contiguous [B, S, Hkv, D] cache

Prints ONE JSON line: per block size and leg the median TB/s (K and V bytes
of the valid keys over the call's time, combine kernel included), the spread
over the repeats ((max - min) / median of the per-repeat times), the ratio
paged / contiguous, and a check that the three legs computed the same thing.
The comparison that counts is paged against contiguous in this process, with
the contiguous leg's own spread as the margin; no figure from elsewhere.
There is no CPU path: without a ROCm device the tool fails.
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


def timed(fn, iters: int) -> float:
    """seconds per call over `iters` back-to-back calls, device events"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / iters


def one_block_size(a, bs: int) -> dict:
    B, H, Hkv, D, S = a.batch, a.heads, a.kv_heads, a.head_dim, a.keys
    dt, dev = torch.bfloat16, "cuda"
    assert S % bs == 0
    per_seq = S // bs
    nb = B * per_seq
    g = torch.Generator(device="cpu").manual_seed(bs)
    torch.manual_seed(bs)
    q = torch.randn(B, 1, H, D, device=dev).to(dt)
    # the contiguous cache and, as the same bytes seen [nb, bs, Hkv, D], the identity-table pool
    kc = torch.randn(B, S, Hkv, D, device=dev).to(dt)
    vc = torch.randn(B, S, Hkv, D, device=dev).to(dt)
    k_id, v_id = kc.view(nb, bs, Hkv, D), vc.view(nb, bs, Hkv, D)
    ident = torch.arange(nb, dtype=torch.int32).reshape(B, per_seq)
    perm = torch.randperm(nb, generator=g).to(torch.int32)
    # page perm[i] of the permuted pool holds what page i of the identity pool holds
    k_pm, v_pm = torch.empty_like(k_id), torch.empty_like(v_id)
    k_pm[perm.long().to(dev)] = k_id
    v_pm[perm.long().to(dev)] = v_id
    t_id, t_pm = ident.to(dev), perm.reshape(B, per_seq).to(dev)
    lens = torch.full((B,), S, dtype=torch.int32, device=dev)
    ws = torch.empty(max(pli_hip.attn_decode_paged_workspace_bytes(B, H, Hkv, 1, S, D) // 4, 1), device=dev)
    outs = {n: torch.empty(B, 1, H, D, device=dev, dtype=dt) for n in ("paged_permuted", "paged_identity", "contiguous")}
    legs = {
        "paged_permuted": lambda: pli_hip.attn_decode_paged(q, k_pm, v_pm, t_pm, lens, out=outs["paged_permuted"], workspace=ws),
        "paged_identity": lambda: pli_hip.attn_decode_paged(q, k_id, v_id, t_id, lens, out=outs["paged_identity"], workspace=ws),
        "contiguous": lambda: pli_hip.attn_decode(q, kc, vc, S, out=outs["contiguous"]),
    }
    routes = {}
    for name, fn in legs.items():  # warm-up: code objects, allocator, clocks
        for _ in range(a.warmup):
            fn()
        routes[name] = pli_hip.last_route()
    torch.cuda.synchronize()
    times = {n: [] for n in legs}
    for _ in range(a.repeats):
        for name, fn in legs.items():
            times[name].append(timed(fn, a.iters))
    nbytes = 2 * B * S * Hkv * D * kc.element_size()  # K and V of every valid key, once
    res = {"block_size": bs, "num_blocks": nb, "routes": routes,
           "seconds_per_leg": {n: round(sum(t) * a.iters, 3) for n, t in times.items()}}
    for name, t in times.items():
        med = statistics.median(t)
        res[name] = {"tbps": round(nbytes / med / 1e12, 4), "us": round(med * 1e6, 2),
                     "spread": round((max(t) - min(t)) / med, 4)}
    for name in ("paged_permuted", "paged_identity"):
        res[f"ratio_{name}_over_contiguous"] = round(res[name]["tbps"] / res["contiguous"]["tbps"], 4)
    res["permuted_equals_identity_bitwise"] = bool(torch.equal(outs["paged_permuted"], outs["paged_identity"]))
    res["max_abs_diff_paged_vs_contiguous"] = float((outs["paged_identity"].float() - outs["contiguous"].float()).abs().max())
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--keys", type=int, default=32768)
    ap.add_argument("--block-sizes", default="16,128")
    ap.add_argument("--iters", type=int, default=1000, help="calls per timed window")
    ap.add_argument("--repeats", type=int, default=10, help="timed windows per leg, alternating")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", help="also append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("paged_decode_bench: no ROCm device (there is no CPU path)", file=sys.stderr)
        return 1
    result = {"tool": "paged_decode_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16",
              "shape": {"B": a.batch, "Hq": a.heads, "Hkv": a.kv_heads, "D": a.head_dim, "keys": a.keys},
              "iters": a.iters, "repeats": a.repeats,
              "block_sizes": {str(bs): one_block_size(a, bs) for bs in map(int, a.block_sizes.split(","))}}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
