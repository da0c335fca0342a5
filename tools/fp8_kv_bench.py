#!/usr/bin/env python3
"""The 1-byte (fp8 e4m3) paged KV cache against the bf16 one, in one process.

    python tools/fp8_kv_bench.py [--sections decode,varlen] [--out FILE]

Sections (32 q / 8 kv heads, D 128, bf16 q, block size 16, permuted tables):
  decode  B 8 x 32k keys (the shape of paged_decode_bench.py):
          pli_hip.attn_decode_paged on a bf16 pool against
          pli_hip.attn_decode_paged_fp8 on the same values quantised
  varlen  shape b of varlen_paged_bench.py (4 requests x 256 new tokens over 4k
          keys + 60 decoding requests at 4k keys): pli_hip.attn_varlen_paged
          against pli_hip.attn_varlen_paged_fp8

The fp8 pools are made from the bf16 ones by the library's own quantising
append (pli_hip.kv_append_paged_fp8, unit scales passed as device tensors).
Every leg owns --sets copies of its pools and walks them round-robin, so no
call finds the bytes the previous call of that leg read in the 256 MB
Infinity Cache.  Legs are timed with device events, warmed, alternating
(bf16, fp8, bf16, fp8, ...).

Prints ONE JSON line: per section and leg the median time per call, the
spread over the repeats ((max - min) / median), the K and V bytes of the valid
keys a call reads over that time (decode), the routes, the ratio bf16 / fp8
(> 1: the fp8 pool is faster) with whether the difference exceeds both legs'
spreads, and max |o_fp8 - o_bf16|, the error of quantising the pool at this
shape (unit-normal K and V).  There is no CPU path: without a ROCm device the
tool fails.
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


def timed(fn, iters: int) -> float:
    """seconds per call over `iters` back-to-back calls, device events"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / iters


def make_pools(kv_lens, seed: int, sets: int):
    """`sets` x (bf16 K, V pools [nb, BS, HKV, D] of unit-normal values, their fp8 quantisation), one permuted
    table for all of them, the lengths"""
    B = len(kv_lens)
    per_seq = [n // BS for n in kv_lens]
    assert all(n % BS == 0 for n in kv_lens) and len(set(kv_lens)) == 1
    nb, mb, S = sum(per_seq), per_seq[0], kv_lens[0]
    g = torch.Generator(device="cpu").manual_seed(seed)
    torch.manual_seed(seed)
    table = torch.randperm(nb, generator=g).to(torch.int32).reshape(B, mb).to(DEV)
    lens = torch.tensor(kv_lens, dtype=torch.int32, device=DEV)
    zero = torch.zeros(B, dtype=torch.int32, device=DEV)
    one = torch.ones(HKV, device=DEV)
    pools = []
    for _ in range(sets):
        k16, v16 = (torch.empty(nb, BS, HKV, D, device=DEV, dtype=DT) for _ in range(2))
        k8, v8 = (torch.empty(nb, BS, HKV, D, device=DEV, dtype=torch.float8_e4m3fn) for _ in range(2))
        kc, vc = (torch.randn(B, S, HKV, D, device=DEV).to(DT) for _ in range(2))
        pli_hip.kv_append_paged(kc, vc, k16, v16, table, zero)
        pli_hip.kv_append_paged_fp8(kc, vc, k8, v8, table, zero, one, one)
        pools.append((k16, v16, k8, v8))
        del kc, vc
    return pools, table, lens, one, nb, mb


def measure(a, legs, outs, nbytes=None) -> dict:
    routes, iters = {}, {}
    for leg, fn in legs.items():  # warm-up: code objects, allocator, clocks; and the size of a timed window
        fn()
        routes[leg] = pli_hip.last_route()
        torch.cuda.synchronize()
        est = timed(fn, 2 * a.sets)
        iters[leg] = max(2 * a.sets, min(a.max_iters, int(a.window / max(est, 1e-7))))
        timed(fn, max(2, iters[leg] // 4))
    times = {leg: [] for leg in legs}
    for _ in range(a.repeats):
        for leg, fn in legs.items():
            times[leg].append(timed(fn, iters[leg]))
    res = dict(routes=routes, iters=iters)
    for leg, t in times.items():
        med = statistics.median(t)
        res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4)}
        if nbytes:
            res[leg]["bytes_read"] = nbytes[leg]
            res[leg]["tbps"] = round(nbytes[leg] / med / 1e12, 4)
    ratio = res["bf16"]["us"] / res["fp8"]["us"]
    margin = max(res["bf16"]["spread"], res["fp8"]["spread"])
    res["bf16_over_fp8"] = round(ratio, 4)
    res["verdict"] = "fp8 faster" if ratio > 1 + margin else "fp8 slower" if ratio < 1 - margin else "within the spread"
    for fn in legs.values():  # the outputs of set 0, for the accuracy figure
        for _ in range(a.sets):
            fn()
    res["max_abs_diff_fp8_vs_bf16"] = float((outs["fp8"][0].float() - outs["bf16"][0].float()).abs().max())
    res["max_abs_bf16_output"] = float(outs["bf16"][0].float().abs().max())
    return res


def rotating(calls):
    """a leg that walks its calls round-robin"""
    state = {"i": 0}

    def run():
        calls[state["i"]]()
        state["i"] = (state["i"] + 1) % len(calls)
    return run


def decode_section(a) -> dict:
    B, S = a.batch, a.keys
    pools, table, lens, one, nb, mb = make_pools([S] * B, 16, a.sets)
    q = torch.randn(B, 1, H, D, device=DEV).to(DT)
    ws = torch.empty(max(pli_hip.attn_decode_paged_workspace_bytes(B, H, HKV, 1, S, D) // 4, 1), device=DEV)
    outs = {leg: [torch.empty(B, 1, H, D, device=DEV, dtype=DT) for _ in range(a.sets)] for leg in ("bf16", "fp8")}
    legs = {
        "bf16": rotating([lambda p=p, o=o: pli_hip.attn_decode_paged(q, p[0], p[1], table, lens, out=o, workspace=ws)
                          for p, o in zip(pools, outs["bf16"])]),
        "fp8": rotating([lambda p=p, o=o: pli_hip.attn_decode_paged_fp8(q, p[2], p[3], table, lens, one, one, out=o,
                                                                        workspace=ws)
                         for p, o in zip(pools, outs["fp8"])]),
    }
    elems = 2 * B * S * HKV * D  # K and V of every valid key, once
    res = measure(a, legs, outs, {"bf16": 2 * elems, "fp8": elems})
    return dict(batch=B, keys=S, num_blocks=nb, sets=a.sets, **res)


def varlen_section(a) -> dict:
    q_lens, kv_lens = [256] * 4 + [1] * 60, [4096] * 64
    pools, table, lens, one, nb, mb = make_pools(kv_lens, 98, a.sets)
    T = sum(q_lens)
    cu_h = [0]
    for n in q_lens:
        cu_h.append(cu_h[-1] + n)
    cu = torch.tensor(cu_h, dtype=torch.int32, device=DEV)
    q = torch.randn(T, H, D, device=DEV).to(DT)
    outs = {leg: [torch.zeros(T, H, D, device=DEV, dtype=DT) for _ in range(a.sets)] for leg in ("bf16", "fp8")}
    legs = {
        "bf16": rotating([lambda p=p, o=o: pli_hip.attn_varlen_paged(q, p[0], p[1], table, lens, cu, out=o)
                          for p, o in zip(pools, outs["bf16"])]),
        "fp8": rotating([lambda p=p, o=o: pli_hip.attn_varlen_paged_fp8(q, p[2], p[3], table, lens, cu, one, one, out=o)
                         for p, o in zip(pools, outs["fp8"])]),
    }
    return dict(batch=len(q_lens), tokens=T, keys=kv_lens[0], num_blocks=nb, sets=a.sets, **measure(a, legs, outs))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sections", default="decode,varlen")
    ap.add_argument("--batch", type=int, default=8, help="decode section: sequences")
    ap.add_argument("--keys", type=int, default=32768, help="decode section: keys per sequence")
    ap.add_argument("--sets", type=int, default=2, help="pool copies a leg walks round-robin")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    ap.add_argument("--max-iters", type=int, default=2000, help="cap on calls per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per leg, alternating")
    ap.add_argument("--out", help="also append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("fp8_kv_bench: no ROCm device (there is no CPU path)", file=sys.stderr)
        return 1
    sections = {"decode": decode_section, "varlen": varlen_section}
    result = {"tool": "fp8_kv_bench", "device": torch.cuda.get_device_name(0), "q_dtype": "bf16", "heads": [H, HKV],
              "D": D, "block_size": BS, "repeats": a.repeats, "window_s": a.window,
              "sections": {s: sections[s](a) for s in a.sections.split(",")}}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
