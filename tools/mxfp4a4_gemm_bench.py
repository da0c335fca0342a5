#!/usr/bin/env python3
"""MXFP4 activations x MXFP4 weights (W4A4, pli_hip.linear_mxfp4a4) against W4A8, W8A8 and the bf16 GEMM, in one
process.

    python tools/mxfp4a4_gemm_bench.py [--shapes 4096x4096,...] [--ms 128,512,...] [--out FILE]

C = x W^T at W [n, k] in 4096^2, 8192^2, 14336 x 4096 and 4096 x 14336, each at M in {128, 512, 2048, 8192}; bf16
activations, N(0,1) weights; six legs, microseconds per call:
  w4a4         pli_hip.linear_mxfp4a4: quant_rows_mxfp4 + gemm_mxfp4_a4, two launches, the quantiser inside the leg
  w4a4_gemm    pli_hip.gemm_mxfp4_a4 alone on rows quantised beforehand, with its TFLOP/s
  w4a8         pli_hip.linear_mxfp4a: quant_rows_fp8 + gemm_mxfp4
  w4a8_gemm    pli_hip.gemm_mxfp4 alone: the comparison the W4A4 GEMM is held to
  w8a8_gemm    pli_hip.gemm_fp8 alone on fp8 weights of the same shape
  bf16         pli_hip.gemm NT on bf16 weights

Protocol: tools/mxfp4a_gemm_bench.py's, on the helpers of tools/fp8w_linear_bench.py: every leg owns enough copies of
its weights that one walk over them is past --footprint bytes (the Infinity Cache), a leg is one captured graph that
walks its copies once, graphs are replayed back to back and timed with device events, the legs alternating,
--repeats windows each.  Reported per case and leg: median time per call, the spread ((max - min) / median), TFLOP/s,
the route; the ratio of every other leg over w4a4 and over w4a4_gemm (> 1: the new call is faster) with a verdict that
needs the difference to exceed both spreads; and the error of the W4A4 and W4A8 results (rms and max, relative to
rms(y) of the bf16 linear over the same weights before quantisation).  One JSON line per case.  There is no CPU path.
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

DT, DEV = torch.bfloat16, "cuda"
SHAPES = "4096x4096,8192x8192,14336x4096,4096x14336"  # n x k
MS = "128,512,2048,8192"
LEGS = ("w4a4", "w4a4_gemm", "w4a8", "w4a8_gemm", "w8a8_gemm", "bf16")
NEW = ("w4a4", "w4a4_gemm")


def make_weights(n: int, k: int, footprint: int):
    """bf16, fp8 and MXFP4 copies of N(0,1) [n, k] weights, each set past the footprint; copy 0 of each is the same
    weight"""
    w0 = torch.randn(n, k, device=DEV)
    new = lambda i: w0 if i == 0 else torch.randn(n, k, device=DEV)  # noqa: E731
    w16 = [new(i).to(DT) for i in range(fb.copies(n * k * 2, footprint))]
    w8 = [pli_hip.quantize_weight_fp8(new(i)) for i in range(fb.copies(n * k, footprint))]
    w4 = [pli_hip.quantize_weight_mxfp4(new(i)) for i in range(fb.copies(n * k // 2 + n * k // 32, footprint))]
    return w16, w8, w4


def cases(a, emit):
    for n, k in (tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")):
        w16, w8, w4 = make_weights(n, k, a.footprint)
        for m in (int(v) for v in a.ms.split(",")):
            x = torch.randn(m, k, device=DEV).to(DT)
            x8, xs8 = pli_hip.quantize_rows_fp8(x)
            x4, xe, xs4 = pli_hip.quantize_rows_mxfp4(x)
            o = {leg: torch.empty(m, n, device=DEV, dtype=DT) for leg in LEGS}
            legs = {
                "w4a4": [lambda w=w: pli_hip.linear_mxfp4a4(x, w[0], w[1], out=o["w4a4"]) for w in w4],
                "w4a4_gemm": [lambda w=w: pli_hip.gemm_mxfp4_a4(x4, xe, xs4, w[0], w[1], out=o["w4a4_gemm"],
                                                                out_dtype=DT) for w in w4],
                "w4a8": [lambda w=w: pli_hip.linear_mxfp4a(x, w[0], w[1], out=o["w4a8"]) for w in w4],
                "w4a8_gemm": [lambda w=w: pli_hip.gemm_mxfp4(x8, xs8, w[0], w[1], out=o["w4a8_gemm"], out_dtype=DT)
                              for w in w4],
                "w8a8_gemm": [lambda w=w: pli_hip.gemm_fp8(x8, xs8, w[0], w[1], out_dtype=DT, out=o["w8a8_gemm"])
                              for w in w8],
                "bf16": [lambda w=w: pli_hip.gemm(x, w, trans_b=True, out=o["bf16"]) for w in w16],
            }
            routes, times = fb.time_legs(a, legs)
            routes["w4a4"] = "quant_rows_mxfp4+" + routes["w4a4"]  # the leg's two launches (last_route names the last)
            routes["w4a8"] = "quant_rows_fp8+" + routes["w4a8"]
            res = {}
            for leg, t in times.items():
                med = statistics.median(t)
                res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4),
                            "tflops": round(2.0 * m * n * k / med / 1e12, 1)}
            rec = {}
            for den in NEW:
                for num in LEGS:
                    if num in NEW:
                        continue
                    ratio = res[num]["us"] / res[den]["us"]
                    rec[f"{num}_over_{den}"] = round(ratio, 3)
                    rec[f"verdict_{den}_vs_{num}"] = fb.verdict_of(ratio, max(res[num]["spread"], res[den]["spread"]), den)
            for leg in legs:
                legs[leg][0]()  # copy 0 of every leg is the same weight: the format's cost against the bf16 linear
            emit(dict(n=n, k=k, m=m, routes=routes, copies={leg: len(f) for leg, f in legs.items()}, **res, **rec,
                      quant_error={leg: fb.quant_error(o[leg], o["bf16"]) for leg in ("w4a4", "w4a8")}))
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
        print("mxfp4a4_gemm_bench: no ROCm device (there is no CPU path)", file=sys.stderr)
        return 1
    torch.manual_seed(11)
    head = {"tool": "mxfp4a4_gemm_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16",
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
