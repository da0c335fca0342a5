#!/usr/bin/env python3
"""MXFP4 expert weights (pli_hip.gemm_grouped_mxfp4, ch09.Mxfp4MoELayer) against the bf16 grouped GEMM and
ch09.MoELayer, in one process.

    python tools/grouped_mxfp4_bench.py [--tokens 1,32,128,512,2048] [--out FILE]

MoEConfig defaults (H 4096, 8 experts x 14336, top-2), bf16, routed by the layer's own router on N(0,1) tokens.  Per
token count, legs:
  bf16_w13 / bf16_w2    pli_hip.gemm_grouped on the bf16 weights (fused SwiGLU over W1 / W3 with gather; W2)
  mx_w13 / mx_w2        quantize_rows_fp8 + gemm_grouped_mxfp4, the quantiser inside the timed leg
  mx_w13_gemm / mx_w2_gemm   gemm_grouped_mxfp4 alone on rows quantised beforehand
  quant_x / quant_h     quantize_rows_fp8 alone
  bf16_layer / mx_layer the whole layers (router, route, both grouped GEMMs, combine)
and, up to 32 sorted rows (16 tokens), the split-K decode route (pli_gemm_grouped_mxfp4_ws) beside the plain call:
  ws_w13 / ws_w2, ws_w13_gemm / ws_w2_gemm   the mx_* legs with a workspace (``--splits``: 0 lets the rule choose)
  ws_layer              Mxfp4MoELayer.from_layer(split_decode=True)
with the ratios mx / ws (> 1: the split route is faster than the plain call), bf16 / ws, and for the two ws_*_gemm
legs the GB/s of MXFP4 bytes of the experts that have rows (codes and scale bytes of W1 + W3, or of W2).

Protocol: tools/fp8w_linear_bench.py's (its helpers are imported).  At one token only two experts are read: 62 MB
(W2) / 125 MB (W1, W3) of MXFP4 and 235 / 470 MB of bf16, not all past the 256 MiB Infinity Cache.  So every weight
leg walks --mx-copies (4) / --bf16-copies (2) separate copies of the layer's weights in turn, 250 MB of MXFP4 or
470 MB of bf16 at the least between two reads of the same bytes.  A GEMM or quantiser leg is one captured graph over
its copies, graphs are replayed back to back and timed with device events, the legs alternating, --repeats windows
each; the two layer legs run eagerly over their copies in turn, --layer-calls calls per window (launch overhead
included on both sides).  Reported per
leg: median time per call and spread ((max - min) / median); the ratios bf16 / mx (> 1: MXFP4 is faster) with a
verdict that needs the difference to exceed both spreads; and the format's error, rms and max of the MXFP4 layer's y
against the bf16 layer's, relative to rms(y_bf16).  One JSON line per token count; run it twice for two runs.  There
is no CPU path.
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
PAIRS = (("bf16_w13", "mx_w13"), ("bf16_w13", "mx_w13_gemm"), ("bf16_w2", "mx_w2"), ("bf16_w2", "mx_w2_gemm"),
         ("bf16_layer", "mx_layer"))
WS_PAIRS = tuple((f"{side}_{leg}", f"ws_{leg}") for leg in ("w13", "w13_gemm", "w2", "w2_gemm", "layer")
                 for side in ("mx", "bf16") if not (side == "bf16" and leg.endswith("_gemm")))
WS_ROWS = Mxfp4MoELayer.SPLIT_ROWS


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tokens", default="1,32,128,512,2048")
    ap.add_argument("--window", type=float, default=0.1, help="seconds of work per timed window")
    ap.add_argument("--max-replays", type=int, default=200, help="cap on graph replays per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per leg, alternating")
    ap.add_argument("--layer-calls", type=int, default=20, help="eager layer calls per timed window")
    ap.add_argument("--bf16-copies", type=int, default=2, help="copies of the bf16 layer a leg walks in turn")
    ap.add_argument("--mx-copies", type=int, default=4, help="copies of the MXFP4 layer a leg walks in turn")
    ap.add_argument("--splits", type=int, default=0, help="S of the ws_* legs (0: the rule chooses)")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("grouped_mxfp4_bench: no ROCm device (there is no CPU path)", file=sys.stderr)
        return 1
    torch.manual_seed(9)
    cfg = MoEConfig()
    H, I, k = cfg.hidden_dim, cfg.expert_dim, cfg.num_experts_per_tok
    with torch.device(DEV), torch.no_grad():
        layer = MoELayer(cfg).to(DT).eval()
        layers = [layer] + [copy.deepcopy(layer) for _ in range(a.bf16_copies - 1)]
        mxs = [Mxfp4MoELayer.from_layer(layer)]
        mxs += [copy.deepcopy(mxs[0]) for _ in range(a.mx_copies - 1)]
        wss = [copy.copy(m) for m in mxs]  # the same weights and tables, the option on
        for m in wss:
            m.split_decode = True
    mx, bt, mt = mxs[0], [m._weight_tables() for m in layers], [m._weight_tables() for m in mxs]
    head = {"tool": "grouped_mxfp4_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16", "hidden": H,
            "expert_dim": I, "experts": cfg.num_experts, "top_k": k, "repeats": a.repeats, "window_s": a.window,
            "copies": {"bf16": a.bf16_copies, "mx": a.mx_copies}}
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "a")
    for T in (int(t) for t in a.tokens.split(",")):
        with torch.no_grad():
            x = torch.randn(1, T, H, device=DEV).to(DT)
            xf, rows = x.view(T, H), T * k
            _, _, _, gather, offsets = pli_hip.moe_route(layer.router._logits(xf), k, cfg.normalize_expert_weights)
            x8, xs = pli_hip.quantize_rows_fp8(xf)
            h16 = pli_hip.gemm_grouped(xf, gather, bt[0][0], offsets, rows, I, H, H, wu_table=bt[0][1])
            h8, hs = pli_hip.quantize_rows_fp8(h16)
            hm, ym = torch.empty_like(h16), torch.empty(max(rows, 1), H, device=DEV, dtype=DT)
            y16 = torch.empty_like(ym)
            q = lambda t: pli_hip.quantize_rows_fp8(t)  # noqa: E731
            g13 = lambda t, c8, s: pli_hip.gemm_grouped_mxfp4(c8, s, gather, t[0], offsets, rows, I, H, up_tables=t[1], out=hm)  # noqa: E731
            g2 = lambda t, c8, s: pli_hip.gemm_grouped_mxfp4(c8, s, None, t[2], offsets, rows, H, I, out=ym)  # noqa: E731
            b13 = lambda t: pli_hip.gemm_grouped(xf, gather, t[0], offsets, rows, I, H, H, wu_table=t[1], out=h16)  # noqa: E731
            b2 = lambda t: pli_hip.gemm_grouped(h16, None, t[2], offsets, rows, H, I, I, out=y16)  # noqa: E731
            legs = {
                "bf16_w13": [lambda t=t: b13(t) for t in bt], "bf16_w2": [lambda t=t: b2(t) for t in bt],
                "mx_w13": [lambda t=t: g13(t, *q(xf)) for t in mt], "mx_w13_gemm": [lambda t=t: g13(t, x8, xs) for t in mt],
                "mx_w2": [lambda t=t: g2(t, *q(h16)) for t in mt], "mx_w2_gemm": [lambda t=t: g2(t, h8, hs) for t in mt],
                "quant_x": [lambda: q(xf)], "quant_h": [lambda: q(h16)],
            }
            if rows <= WS_ROWS:
                need = max(pli_hip.gemm_grouped_mxfp4_workspace_bytes(cfg.num_experts, rows, I, H, True, a.splits),
                           pli_hip.gemm_grouped_mxfp4_workspace_bytes(cfg.num_experts, rows, H, I, False, a.splits))
                work = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
                w13 = lambda t, c8, s: pli_hip.gemm_grouped_mxfp4(c8, s, gather, t[0], offsets, rows, I, H, up_tables=t[1], out=hm,  # noqa: E731
                                                                  workspace=work, splits=a.splits)
                w2 = lambda t, c8, s: pli_hip.gemm_grouped_mxfp4(c8, s, None, t[2], offsets, rows, H, I, out=ym, workspace=work,  # noqa: E731
                                                                 splits=a.splits)
                legs.update({"ws_w13": [lambda t=t: w13(t, *q(xf)) for t in mt], "ws_w13_gemm": [lambda t=t: w13(t, x8, xs) for t in mt],
                             "ws_w2": [lambda t=t: w2(t, *q(h16)) for t in mt], "ws_w2_gemm": [lambda t=t: w2(t, h8, hs) for t in mt]})
            routes, times = fb.time_legs(a, legs)
            # the whole layers run eagerly (the router's launch clears its counters with a memset, which stays out of
            # captured graphs here): --layer-calls calls per window between two device events, alternating
            models = {"bf16_layer": layers, "mx_layer": mxs, **({"ws_layer": wss} if rows <= WS_ROWS else {})}
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
            rec = {}
            for num, den in PAIRS:
                ratio = res[num]["us"] / res[den]["us"]
                rec[f"{num}_over_{den}"] = round(ratio, 3)
                rec[f"verdict_{den}"] = fb.verdict_of(ratio, max(res[num]["spread"], res[den]["spread"]), den)
            if rows <= WS_ROWS:
                for num, den in WS_PAIRS:
                    ratio = res[num]["us"] / res[den]["us"]
                    rec[f"{num}_over_{den}"] = round(ratio, 3)
                    rec[f"verdict_{den}_vs_{num.split('_')[0]}"] = fb.verdict_of(ratio, max(res[num]["spread"], res[den]["spread"]), den)
                active = int((offsets[1:] != offsets[:-1]).sum())  # experts that have rows: the bytes a call must stream
                for leg, per_expert in (("ws_w13_gemm", 2 * I * (H // 2 + H // 32)), ("ws_w2_gemm", H * (I // 2 + I // 32))):
                    res[leg]["mxfp4_mb"] = round(active * per_expert / 1e6, 1)
                    res[leg]["mxfp4_gbps"] = round(active * per_expert / res[leg]["us"] / 1e3, 1)
            line = json.dumps({**head, "tokens": T, "rows": rows, "splits": a.splits, "routes": routes, **res, **rec,
                               "format_error": fb.quant_error(mx(x), layer(x))})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
