#!/usr/bin/env python3
"""Split-K packed variable-length paged attention (pli_attn_varlen_paged_ws)
against the plain packed call and what else the library has for the same
work, in one process.

    python tools/varlen_split_bench.py [--shapes a,b,c,e,b32k,c_fp8,e_fp8]
                                       [--split-keys 0,1024] [--out FILE]

Shapes (32 q / 8 kv heads, D 128, bf16 q, block size 16, permuted tables; a, b,
c are those of tools/varlen_paged_bench.py):
  a      chunked prefill: one request, 512 new tokens over 32k keys
  b      mixed: 4 requests x 256 new tokens over 4k keys + 60 decoding
         requests at 4k keys
  c      decode only: 8 requests x 32k keys
  e      mixed: 4 requests x 256 new tokens over 4k keys + 8 decoding requests
         at 32k keys
  b32k   b with the table (max_kv) widened to 32k keys: the cost of the
         workgroups that find no chunk
  c_fp8, e_fp8   c and e over fp8 e4m3 pools

Legs, timed with device events, warmed, alternating, --repeats windows of
--window seconds each (the protocol of tools/varlen_paged_bench.py):
  plain         pli_hip.attn_varlen_paged[_fp8], one workgroup per tile
  ws_<k>        the same call with workspace= and split_keys=<k> (0: the plan's
                own span), one leg per entry of --split-keys
  decode        c, c_fp8: pli_hip.attn_decode_paged[_fp8]
  gather_flash  a: gather the pages, pli_hip.flash_attn_fwd(causal)

Prints ONE JSON line: per shape and leg the median time per step, the spread
((max - min) / median), the route, the span and chunk count of each ws leg, the
ratios plain / ws (> 1: the split call is faster) with whether the difference
exceeds both legs' spreads, the other legs' ratios to ws_0, and the largest
|difference| between each leg's output and the plain leg's.  There is no CPU
path: without a ROCm device the tool fails.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import varlen_paged_bench as vb  # noqa: E402  (puts the package on sys.path)

import pli_hip  # noqa: E402

H, HKV, D, BS, DT, DEV = vb.H, vb.HKV, vb.D, vb.BS, vb.DT, vb.DEV

SHAPES = dict(vb.SHAPES)  # (q_lens, kv_lens after the step)
SHAPES["e"] = ([256] * 4 + [1] * 8, [4096] * 4 + [32768] * 8)
VARIANTS = {"b32k": ("b", dict(max_kv=32768)), "c_fp8": ("c", dict(fp8=True)), "e_fp8": ("e", dict(fp8=True))}


def build(name: str, split_keys):
    """the step's tensors and its legs: {leg: callable}, {leg: output [tokens, H, D]}, info"""
    base, opt = VARIANTS.get(name, (name, {}))
    fp8 = opt.get("fp8", False)
    q_lens, kv_lens = SHAPES[base]
    B, T = len(q_lens), sum(q_lens)
    per_seq = [n // BS for n in kv_lens]
    assert all(n % BS == 0 for n in kv_lens)
    max_kv = opt.get("max_kv", max(kv_lens))
    nb, mb = sum(per_seq), max_kv // BS
    g = torch.Generator(device="cpu").manual_seed(ord(base))
    torch.manual_seed(ord(base))
    k_pool = torch.randn(nb, BS, HKV, D, device=DEV).to(DT)
    v_pool = torch.randn(nb, BS, HKV, D, device=DEV).to(DT)
    scales = ()
    if fp8:  # codes of the same values under per-head scales
        ksc = torch.linspace(0.5, 1.5, HKV, device=DEV)
        vsc = torch.linspace(1.5, 0.5, HKV, device=DEV)
        k_pool = (k_pool.float() / ksc[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
        v_pool = (v_pool.float() / vsc[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
        scales = (ksc, vsc)
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
    varlen = pli_hip.attn_varlen_paged_fp8 if fp8 else pli_hip.attn_varlen_paged
    outs, legs, plans = {}, {}, {}

    def out_of(leg):
        outs[leg] = torch.zeros(T, H, D, device=DEV, dtype=DT)
        return outs[leg]

    def varlen_leg(leg, **kw):
        o = out_of(leg)
        legs[leg] = lambda: varlen(q, k_pool, v_pool, table, lens, cu, *scales, max_kv=max_kv, out=o, **kw)

    varlen_leg("plain")
    for k in split_keys:
        need = pli_hip.attn_varlen_paged_workspace_bytes(B, T, H, HKV, max_kv, D, k)
        span, splits = pli_hip.attn_varlen_paged_split_plan(B, T, H, HKV, max_kv, D, k)
        plans[f"ws_{k}"] = dict(span=span, splits_max=splits, workspace_mb=round(need / 2 ** 20, 2))
        varlen_leg(f"ws_{k}", workspace=torch.empty(max(need // 4, 1), device=DEV), split_keys=k)
    if base == "c":
        decode = pli_hip.attn_decode_paged_fp8 if fp8 else pli_hip.attn_decode_paged
        ws = torch.empty(max(pli_hip.attn_decode_paged_workspace_bytes(B, H, HKV, 1, max_kv, D) // 4, 1), device=DEV)
        qq, oo = q.view(B, 1, H, D), out_of("decode").view(B, 1, H, D)
        legs["decode"] = lambda: decode(qq, k_pool, v_pool, table, lens, *scales, max_kv=max_kv, out=oo, workspace=ws)
    if name == "a":
        pages = table[0, :per_seq[0]].long()
        qq = q.unsqueeze(0).permute(0, 2, 1, 3)
        oo = out_of("gather_flash").unsqueeze(0).permute(0, 2, 1, 3)

        def gather_flash():
            kc = k_pool[pages].view(1, kv_lens[0], HKV, D).permute(0, 2, 1, 3)
            vc = v_pool[pages].view(1, kv_lens[0], HKV, D).permute(0, 2, 1, 3)
            pli_hip.flash_attn_fwd(qq, kc, vc, causal=True, out=oo)
        legs["gather_flash"] = gather_flash
    info = dict(batch=B, tokens=T, q_lens=sorted(set(q_lens)), keys=sorted(set(kv_lens)), max_kv=max_kv,
                pool="fp8" if fp8 else "bf16", plans=plans)
    return legs, outs, info


def verdict(ratio, a, b, faster, slower):
    margin = max(a["spread"], b["spread"])
    return faster if ratio > 1 + margin else slower if ratio < 1 - margin else "within the spread"


def one_shape(a, name: str, split_keys) -> dict:
    legs, outs, info = build(name, split_keys)
    routes, iters = {}, {}
    for leg, fn in legs.items():  # warm-up: code objects, allocator, clocks; and the size of a timed window
        fn()
        routes[leg] = pli_hip.last_route()
        torch.cuda.synchronize()
        est = vb.timed(fn, 2)
        iters[leg] = max(2, min(a.max_iters, int(a.window / max(est, 1e-7))))
        vb.timed(fn, max(2, iters[leg] // 4))
    times = {leg: [] for leg in legs}
    for _ in range(a.repeats):
        for leg, fn in legs.items():
            times[leg].append(vb.timed(fn, iters[leg]))
    res = dict(info, routes=routes, iters=iters)
    for leg, t in times.items():
        med = statistics.median(t)
        res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4)}
    for leg in legs:
        if leg != "plain":
            res[f"max_abs_diff_{leg}"] = float((outs[leg].float() - outs["plain"].float()).abs().max())
        if leg.startswith("ws_"):
            ratio = res["plain"]["us"] / res[leg]["us"]
            res[f"plain_over_{leg}"] = round(ratio, 4)
            res[f"{leg}_vs_plain"] = verdict(ratio, res["plain"], res[leg], "ws faster", "ws slower")
    ref = "ws_0" if "ws_0" in legs else next((leg for leg in legs if leg.startswith("ws_")), None)
    for leg in ("decode", "gather_flash"):
        if leg in legs and ref:
            ratio = res[leg]["us"] / res[ref]["us"]
            res[f"{leg}_over_{ref}"] = round(ratio, 4)
            res[f"{ref}_vs_{leg}"] = verdict(ratio, res[leg], res[ref], "ws faster", "ws slower")
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="a,b,c,e,b32k,c_fp8,e_fp8")
    ap.add_argument("--split-keys", default="0", help="comma-separated split_keys values, one ws leg each (0: the plan's)")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--max-iters", type=int, default=2000, help="cap on calls per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per leg, alternating")
    ap.add_argument("--out", help="also append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("varlen_split_bench: no ROCm device (there is no CPU path)", file=sys.stderr)
        return 1
    split_keys = [int(k) for k in a.split_keys.split(",")]
    result = {"tool": "varlen_split_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16",
              "heads": [H, HKV], "D": D, "block_size": BS, "repeats": a.repeats, "window_s": a.window,
              "split_keys": split_keys, "shapes": {s: one_shape(a, s, split_keys) for s in a.shapes.split(",")}}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
