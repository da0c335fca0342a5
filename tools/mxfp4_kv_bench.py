#!/usr/bin/env python3
"""The MXFP4 paged KV cache against the fp8 and the bf16 ones, in one process.

    python tools/mxfp4_kv_bench.py [--keys 32768] [--sets 2] [--out FILE]

Decode attention at B x keys (32 q / 8 kv heads, D 128, bf16 q, block size 16,
permuted tables), three legs over the same unit-normal K and V:
  bf16   pli_hip.attn_decode_paged on a bf16 pool
  fp8    pli_hip.attn_decode_paged_fp8 on its quantisation (unit scales)
  mxfp4  pli_hip.attn_decode_paged_mxfp4 on the code + scale pools
The quantised pools are made by the library's own appends.  The protocol is
tools/fp8_kv_bench.py's: every leg owns --sets copies of its pools and walks
them round-robin (choose --sets so that the smallest leg's copies together pass
the 256 MB Infinity Cache: 2 at 8 x 32k keys, 16 at 8 x 2k), legs are timed with
device events, warmed, alternating.

Prints ONE JSON line: per leg the median time per call, the spread over the
repeats ((max - min) / median), the K / V (and scale) bytes of the valid keys a
call reads over that time, the route; fp8 / mxfp4 and bf16 / mxfp4 time ratios
(> 1: the MXFP4 pool is faster) with whether the difference from fp8 exceeds both
legs' spreads; and max |o - o_bf16| of both formats.  No CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "physics-llm-inference_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import pli_hip  # noqa: E402
from fp8_kv_bench import BS, D, DEV, DT, H, HKV, rotating, timed  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--keys", type=int, default=32768, help="keys per sequence (a multiple of 16)")
    ap.add_argument("--sets", type=int, default=2, help="pool copies a leg walks round-robin")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    ap.add_argument("--max-iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per leg, alternating")
    ap.add_argument("--out", help="also append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("mxfp4_kv_bench: no ROCm device (there is no CPU path)", file=sys.stderr)
        return 1
    B, S = a.batch, a.keys
    assert S % BS == 0
    mb = S // BS
    nb = B * mb
    torch.manual_seed(16)
    table = torch.randperm(nb).to(torch.int32).reshape(B, mb).to(DEV)
    lens = torch.full((B,), S, dtype=torch.int32, device=DEV)
    zero, one = torch.zeros(B, dtype=torch.int32, device=DEV), torch.ones(HKV, device=DEV)
    pools = []
    for _ in range(a.sets):
        k16, v16 = (torch.empty(nb, BS, HKV, D, device=DEV, dtype=DT) for _ in range(2))
        k8, v8 = (torch.empty(nb, BS, HKV, D, device=DEV, dtype=torch.float8_e4m3fn) for _ in range(2))
        k4, v4 = (torch.empty(nb, BS, HKV, D // 2, device=DEV, dtype=torch.uint8) for _ in range(2))
        ke, ve = (torch.empty(nb, BS, HKV, D // 32, device=DEV, dtype=torch.uint8) for _ in range(2))
        kc, vc = (torch.randn(B, S, HKV, D, device=DEV).to(DT) for _ in range(2))
        pli_hip.kv_append_paged(kc, vc, k16, v16, table, zero)
        pli_hip.kv_append_paged_fp8(kc, vc, k8, v8, table, zero, one, one)
        pli_hip.kv_append_paged_mxfp4(kc, vc, k4, v4, ke, ve, table, zero)
        pools.append(dict(bf16=(k16, v16), fp8=(k8, v8), mxfp4=(k4, v4, ke, ve)))
        del kc, vc
    q = torch.randn(B, 1, H, D, device=DEV).to(DT)
    ws = torch.empty(max(pli_hip.attn_decode_paged_workspace_bytes(B, H, HKV, 1, S, D) // 4, 1), device=DEV)
    calls = {"bf16": lambda p, o: pli_hip.attn_decode_paged(q, *p, table, lens, out=o, workspace=ws),
             "fp8": lambda p, o: pli_hip.attn_decode_paged_fp8(q, *p, table, lens, one, one, out=o, workspace=ws),
             "mxfp4": lambda p, o: pli_hip.attn_decode_paged_mxfp4(q, *p, table, lens, out=o, workspace=ws)}
    outs = {leg: [torch.empty(B, 1, H, D, device=DEV, dtype=DT) for _ in range(a.sets)] for leg in calls}
    legs = {leg: rotating([lambda p=p[leg], o=o, f=f: f(p, o) for p, o in zip(pools, outs[leg])])
            for leg, f in calls.items()}
    elems = 2 * B * S * HKV * D  # K and V of every valid key, once
    nbytes = {"bf16": 2 * elems, "fp8": elems, "mxfp4": elems // 2 + elems // 32}
    routes, iters = {}, {}
    for leg, fn in legs.items():  # warm-up, and the size of a timed window
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
        res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4), "bytes_read": nbytes[leg],
                    "tbps": round(nbytes[leg] / med / 1e12, 4)}
    ratio = res["fp8"]["us"] / res["mxfp4"]["us"]
    margin = max(res["fp8"]["spread"], res["mxfp4"]["spread"])
    res["fp8_over_mxfp4"] = round(ratio, 4)
    res["bf16_over_mxfp4"] = round(res["bf16"]["us"] / res["mxfp4"]["us"], 4)
    res["verdict"] = ("mxfp4 faster than fp8" if ratio > 1 + margin else
                      "mxfp4 slower than fp8" if ratio < 1 - margin else "within the spread of fp8")
    for fn in legs.values():  # the outputs of set 0, for the accuracy figures
        for _ in range(a.sets):
            fn()
    ref = outs["bf16"][0].float()
    res["max_abs_diff_vs_bf16"] = {leg: float((outs[leg][0].float() - ref).abs().max()) for leg in ("fp8", "mxfp4")}
    res["max_abs_bf16_output"] = float(ref.abs().max())
    result = {"tool": "mxfp4_kv_bench", "device": torch.cuda.get_device_name(0), "q_dtype": "bf16", "heads": [H, HKV],
              "D": D, "block_size": BS, "batch": B, "keys": S, "sets": a.sets, "repeats": a.repeats,
              "window_s": a.window, **res}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
