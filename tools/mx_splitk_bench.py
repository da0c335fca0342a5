#!/usr/bin/env python3
"""The split-K block-scaled GEMM for 17 .. 256 rows (pli_hip.gemm_fp8 / gemm_mxfp4 with workspace=) against the plain
calls, the weight-only linears and the bf16 GEMM, in one process.

    python tools/mx_splitk_bench.py [--shapes 4096x4096,...] [--ms 32,64,...] [--out FILE]

C = x W^T at W [n, k] in 4096^2, 8192^2, 14336 x 4096 and 4096 x 14336, each at M in {32, 64, 128, 256} and at the
control M = 512, where the split route must not apply; rows quantised beforehand, N(0,1) weights; seven legs,
microseconds per call:
  w8a8_ws / w4a8_ws        gemm_fp8 / gemm_mxfp4 with the workspace, splits = 0 (the rule)
  w8a8_plain / w4a8_plain  the same operands without a workspace: what a caller gets without the new entry points
  w8a16 / w4a16            linear_fp8w / linear_mxfp4w on the bf16 rows with their workspaces
  bf16                     pli_hip.gemm NT on bf16 weights (with its workspace)

Protocol: tools/fp8w_linear_bench.py's (its helpers are imported): every leg owns enough copies of its weights that
one walk over them is past --footprint bytes, a leg is one captured graph that walks its copies once, graphs are
replayed back to back and timed with device events, the legs alternating, --repeats windows each.  Reported per case
and leg: median time per call, the spread ((max - min) / median), the route, the weight stream in TB/s (weight bytes
of the shape over the time); per format the ratio plain / ws (> 1: the split call is faster) with a verdict that needs
the difference to exceed both spreads, the ratio bf16 / ws, the S the rule chose, and the largest difference between
the split and the plain result relative to rms(C).  One JSON line per case; run it twice for two runs.  No CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "physics-llm-inference_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import fp8w_linear_bench as fb  # noqa: E402  (the protocol's helpers)
import pli_hip  # noqa: E402
from mxfp4a_gemm_bench import make_weights  # noqa: E402

DT, DEV = torch.bfloat16, "cuda"
SHAPES = "4096x4096,8192x8192,14336x4096,4096x14336"  # n x k
MS = "32,64,128,256,512"
WEIGHT_BYTES = {"w8a8": 1.0, "w4a8": 0.5 + 1 / 32, "w8a16": 1.0, "w4a16": 0.5 + 1 / 32, "bf16": 2.0}  # per element


def cases(a, emit):
    for n, k in (tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")):
        w16, w8, w4 = make_weights(n, k, a.footprint)
        for m in (int(v) for v in a.ms.split(",")):
            x = torch.randn(m, k, device=DEV).to(DT)
            x8, xs = pli_hip.quantize_rows_fp8(x)
            need = {"w8a8": pli_hip.gemm_fp8_workspace_bytes(m, n, k), "w4a8": pli_hip.gemm_mxfp4_workspace_bytes(m, n, k),
                    "w8a16": pli_hip.linear_fp8w_workspace_bytes(m, n, k, DT),
                    "w4a16": pli_hip.linear_mxfp4w_workspace_bytes(m, n, k, DT)}
            ws = {leg: torch.empty(max(b, 16), dtype=torch.uint8, device=DEV) for leg, b in need.items()}
            names = ("w8a8_ws", "w8a8_plain", "w4a8_ws", "w4a8_plain", "w8a16", "w4a16", "bf16")
            o = {leg: torch.empty(m, n, device=DEV, dtype=DT) for leg in names}
            legs = {
                "w8a8_ws": [lambda w=w: pli_hip.gemm_fp8(x8, xs, w[0], w[1], out_dtype=DT, out=o["w8a8_ws"],
                                                         workspace=ws["w8a8"]) for w in w8],
                "w8a8_plain": [lambda w=w: pli_hip.gemm_fp8(x8, xs, w[0], w[1], out_dtype=DT, out=o["w8a8_plain"])
                               for w in w8],
                "w4a8_ws": [lambda w=w: pli_hip.gemm_mxfp4(x8, xs, w[0], w[1], out_dtype=DT, out=o["w4a8_ws"],
                                                           workspace=ws["w4a8"]) for w in w4],
                "w4a8_plain": [lambda w=w: pli_hip.gemm_mxfp4(x8, xs, w[0], w[1], out_dtype=DT, out=o["w4a8_plain"])
                               for w in w4],
                "w8a16": [lambda w=w: pli_hip.linear_fp8w(x, w[0], w[1], out=o["w8a16"], workspace=ws["w8a16"])
                          for w in w8],
                "w4a16": [lambda w=w: pli_hip.linear_mxfp4w(x, w[0], w[1], out=o["w4a16"], workspace=ws["w4a16"])
                          for w in w4],
                "bf16": [lambda w=w: pli_hip.gemm(x, w, trans_b=True, out=o["bf16"]) for w in w16],
            }
            routes, times = fb.time_legs(a, legs)
            res = {}
            for leg, t in times.items():
                med = statistics.median(t)
                res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4),
                            "weight_tbps": round(n * k * WEIGHT_BYTES[leg.split("_")[0]] / med / 1e12, 3)}
            rec = {}
            for fmt in ("w8a8", "w4a8"):
                wsl, pl = fmt + "_ws", fmt + "_plain"
                ratio = res[pl]["us"] / res[wsl]["us"]
                rec[f"{pl}_over_ws"] = round(ratio, 3)
                rec[f"verdict_{fmt}"] = fb.verdict_of(ratio, max(res[pl]["spread"], res[wsl]["spread"]), "ws")
                rec[f"bf16_over_{wsl}"] = round(res["bf16"]["us"] / res[wsl]["us"], 3)
                rec[f"splits_{fmt}"] = need[fmt] // (m * n * 4)
                legs[wsl][0](), legs[pl][0]()  # copy 0 of both legs is the same weight
                d = (o[wsl].float() - o[pl].float()).abs().max() / o[pl].float().pow(2).mean().sqrt()
                rec[f"max_diff_over_rms_{fmt}"] = float(f"{d.item():.3e}")
            emit(dict(n=n, k=k, m=m, routes=routes, copies={leg: len(f) for leg, f in legs.items()}, **res, **rec))
        del w16, w8, w4
        torch.cuda.empty_cache()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x k")
    ap.add_argument("--ms", default=MS, help="comma-separated row counts")
    ap.add_argument("--footprint", type=int, default=512 << 20, help="bytes one walk over a leg's weight copies covers")
    ap.add_argument("--window", type=float, default=0.1, help="seconds of work per timed window")
    ap.add_argument("--max-replays", type=int, default=500, help="cap on graph replays per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per leg, alternating")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("mx_splitk_bench: no ROCm device (there is no CPU path)", file=sys.stderr)
        return 1
    torch.manual_seed(11)
    head = {"tool": "mx_splitk_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16",
            "footprint": a.footprint, "repeats": a.repeats, "window_s": a.window}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps({**head, **rec})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    cases(a, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
