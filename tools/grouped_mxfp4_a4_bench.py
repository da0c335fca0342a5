#!/usr/bin/env python3
"""MXFP4 activations in the MoE layer (pli_hip.gemm_grouped_mxfp4_a4, Mxfp4MoELayer(activations="mxfp4")) against the
fp8-activation path (pli_hip.gemm_grouped_mxfp4, the baseline) on the same routing, in one process.

    python tools/grouped_mxfp4_a4_bench.py [--tokens 512,2048,8192] [--out FILE]

MoEConfig defaults (H 4096, 8 experts x 14336, top-2), bf16, routed by the layer's own router on N(0,1) tokens.  Per
token count, legs (a8: fp8 rows, a4: MXFP4 rows):
  a8_w13_gemm / a4_w13_gemm, a8_w2_gemm / a4_w2_gemm   the grouped GEMM alone on rows quantised beforehand (fused
                                                       SwiGLU over W1 / W3 with gather; W2)
  a8_w13 / a4_w13, a8_w2 / a4_w2                       the row quantiser inside the timed leg
  a8_layer / a4_layer                                  the whole layers (router, route, both GEMMs, combine), eager
Protocol: tools/grouped_mxfp4_bench.py's (tools/fp8w_linear_bench.py's helpers): every weight leg walks --copies
separate copies of the layer's MXFP4 weights in turn, a leg is one captured graph over its copies, graphs are replayed
back to back and timed with device events after a warm-up, the legs alternating, --repeats windows each.  Reported per
leg: median time per call, spread ((max - min) / median) and, for the *_gemm legs, the TFLOP/s of 2 * rows * n * k (W1
and W3: twice); the ratios a8 / a4 (> 1: MXFP4 activations are faster) with a verdict that needs the difference to
exceed both spreads; and the format's error: rms and max of each quantised layer's y against the bf16 layer's,
relative to rms(y_bf16).  One JSON line per token count; run it twice for two runs.  There is no CPU path.
"""
from __future__ import annotations

import argparse
import copy
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
from ch09 import MoEConfig, MoELayer, Mxfp4MoELayer  # noqa: E402

DT, DEV = torch.bfloat16, "cuda"
LEGS = ("w13_gemm", "w2_gemm", "w13", "w2", "layer")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tokens", default="512,2048,8192")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--max-replays", type=int, default=200, help="cap on graph replays per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per leg, alternating")
    ap.add_argument("--layer-calls", type=int, default=10, help="eager layer calls per timed window")
    ap.add_argument("--copies", type=int, default=2, help="copies of the MXFP4 layer a leg walks in turn")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("grouped_mxfp4_a4_bench: no ROCm device (there is no CPU path)", file=sys.stderr)
        return 1
    torch.manual_seed(9)
    cfg = MoEConfig()
    H, I, k = cfg.hidden_dim, cfg.expert_dim, cfg.num_experts_per_tok
    with torch.device(DEV), torch.no_grad():
        layer = MoELayer(cfg).to(DT).eval()
        a8s = [Mxfp4MoELayer.from_layer(layer)]
        a8s += [copy.deepcopy(a8s[0]) for _ in range(a.copies - 1)]
        a4s = [copy.copy(m) for m in a8s]  # the same weights and tables, the other activation format
        for m in a4s:
            m.activations = "mxfp4"
    tabs = [m._weight_tables() for m in a8s]
    head = {"tool": "grouped_mxfp4_a4_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16", "hidden": H,
            "expert_dim": I, "experts": cfg.num_experts, "top_k": k, "repeats": a.repeats, "window_s": a.window,
            "copies": a.copies}
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "a")
    for T in (int(t) for t in a.tokens.split(",")):
        with torch.no_grad():
            x = torch.randn(1, T, H, device=DEV).to(DT)
            xf, rows = x.view(T, H), T * k
            _, _, _, gather, offsets = pli_hip.moe_route(layer.router._logits(xf), k, cfg.normalize_expert_weights)
            hm, ym = torch.empty(rows, I, device=DEV, dtype=DT), torch.empty(rows, H, device=DEV, dtype=DT)
            q8, q4 = pli_hip.quantize_rows_fp8, pli_hip.quantize_rows_mxfp4
            g8, g4 = pli_hip.gemm_grouped_mxfp4, pli_hip.gemm_grouped_mxfp4_a4
            w13 = lambda g, t, xq: g(*xq, gather, t[0], offsets, rows, I, H, up_tables=t[1], out=hm)  # noqa: E731
            w2 = lambda g, t, hq: g(*hq, None, t[2], offsets, rows, H, I, out=ym)  # noqa: E731
            x8, x4 = q8(xf), q4(xf)
            h = w13(g8, tabs[0], x8).clone()  # one h for both formats' W2 legs
            h8, h4 = q8(h), q4(h)
            legs = {}
            for tag, g, q, xq, hq in (("a8", g8, q8, x8, h8), ("a4", g4, q4, x4, h4)):
                legs[f"{tag}_w13_gemm"] = [lambda t=t, g=g, xq=xq: w13(g, t, xq) for t in tabs]
                legs[f"{tag}_w2_gemm"] = [lambda t=t, g=g, hq=hq: w2(g, t, hq) for t in tabs]
                legs[f"{tag}_w13"] = [lambda t=t, g=g, q=q: w13(g, t, q(xf)) for t in tabs]
                legs[f"{tag}_w2"] = [lambda t=t, g=g, q=q: w2(g, t, q(h)) for t in tabs]
            routes, times = fb.time_legs(a, legs)
            models = {"a8_layer": a8s, "a4_layer": a4s}  # eager: the router's launch stays out of captured graphs
            for leg, mdls in models.items():
                for mdl in mdls:
                    mdl(x)
                times[leg] = []
            for _ in range(a.repeats):
                for leg, mdls in models.items():
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    for i in range(a.layer_calls):
                        mdls[i % len(mdls)](x)
                    stop.record()
                    stop.synchronize()
                    times[leg].append(start.elapsed_time(stop) * 1e-3 / a.layer_calls)
            res = {}
            for leg, t in times.items():
                med = statistics.median(t)
                res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4)}
                if leg.endswith("_gemm"):
                    res[leg]["tflops"] = round((4 if "w13" in leg else 2) * rows * I * H / med / 1e12, 1)
            rec = {}
            for leg in LEGS:
                num, den = res[f"a8_{leg}"], res[f"a4_{leg}"]
                rec[f"a8_over_a4_{leg}"] = round(num["us"] / den["us"], 3)
                rec[f"verdict_{leg}"] = fb.verdict_of(num["us"] / den["us"], max(num["spread"], den["spread"]), "a4")
            y16 = layer(x)
            line = json.dumps({**head, "tokens": T, "rows": rows, "routes": routes, **res, **rec,
                               "format_error": {"a8": fb.quant_error(a8s[0](x), y16), "a4": fb.quant_error(a4s[0](x), y16)}})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
