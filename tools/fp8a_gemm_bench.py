#!/usr/bin/env python3
"""fp8 activations (W8A8, pli_hip.linear_fp8a) against the bf16 GEMM and the W8A16 linear, in one process.

    python tools/fp8a_gemm_bench.py [--sections linear,prefill] [--out FILE]

Sections (bf16 activations, N(0,1) weights, one fp32 scale per row):
  linear   C = x W^T at W [n, k] in 4096^2, 8192^2, 14336 x 4096 and 4096 x
           14336, each at M in {64, 128, 512, 2048, 8192}; four legs:
             bf16       pli_hip.gemm NT on the bf16 weights (with its workspace)
             w8a16      pli_hip.linear_fp8w on the weights quantised, with the
                        workspace its widen + GEMM route wants
             w8a8       pli_hip.linear_fp8a: quant_rows_fp8 + gemm_fp8, two
                        launches, the quantiser inside the timed leg
             w8a8_gemm  pli_hip.gemm_fp8 alone on rows quantised beforehand
  prefill  the teacher-forced prefill of bench.py's 0.85B shape (32000 / 2048 /
           16 layers / 32-8 heads / 5632), batch 4 x 512 tokens, eager, over
           ch02.Fp8WeightModel with fp8_activations off and on; also the cost
           of quantising the activations: rel. L2 of the W8A8 prefill logits
           against the W8A16 model's, and of both against the bf16 model's

Protocol: tools/fp8w_linear_bench.py's (its helpers are imported): every leg
owns enough copies of its weights that one walk over them is past --footprint
bytes, a leg is one captured graph that walks its copies once, graphs are
replayed back to back and timed with device events, the legs alternating,
--repeats windows each.  Reported per case and leg: median time per call, the
spread ((max - min) / median), TFLOP/s, the route; the ratios bf16 / w8a8,
w8a16 / w8a8 and bf16 / w8a8_gemm (> 1: W8A8 is faster) with a verdict that
needs the difference to exceed both spreads; and the quantising error of each
fp8 leg relative to rms(y_bf16).  One JSON line per case; run it twice for two
runs.  There is no CPU path.
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
SHAPES = [(4096, 4096), (8192, 8192), (14336, 4096), (4096, 14336)]  # (n, k)
MS = [64, 128, 512, 2048, 8192]


def linear_cases(a, emit):
    for n, k in SHAPES:
        w16, w8 = fb.make_weights(n, k, a.footprint)
        for m in MS:
            x = torch.randn(m, k, device=DEV).to(DT)
            x8, xs = pli_hip.quantize_rows_fp8(x)
            o = {leg: torch.empty(m, n, device=DEV, dtype=DT) for leg in ("bf16", "w8a16", "w8a8", "w8a8_gemm")}
            nws = pli_hip.linear_fp8w_workspace_bytes(m, n, k, DT)
            ws = torch.empty(nws, dtype=torch.uint8, device=DEV) if nws else None
            legs = {
                "bf16": [lambda w=w: pli_hip.gemm(x, w[0], trans_b=True, out=o["bf16"]) for w in w16],
                "w8a16": [lambda w=w: pli_hip.linear_fp8w(x, w[0][0], w[0][1], out=o["w8a16"], workspace=ws) for w in w8],
                "w8a8": [lambda w=w: pli_hip.linear_fp8a(x, w[0][0], w[0][1], out=o["w8a8"]) for w in w8],
                "w8a8_gemm": [lambda w=w: pli_hip.gemm_fp8(x8, xs, w[0][0], w[0][1], out_dtype=DT, out=o["w8a8_gemm"])
                              for w in w8],
            }
            routes, times = fb.time_legs(a, legs)
            routes["w8a8"] = "quant_rows_fp8+" + routes["w8a8"]  # the leg's two launches (last_route names the last)
            res = {}
            for leg, t in times.items():
                med = statistics.median(t)
                res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4),
                            "tflops": round(2.0 * m * n * k / med / 1e12, 1)}
            rec = {}
            for num, den in (("bf16", "w8a8"), ("w8a16", "w8a8"), ("bf16", "w8a8_gemm")):
                ratio = res[num]["us"] / res[den]["us"]
                rec[f"{num}_over_{den}"] = round(ratio, 3)
                rec[f"verdict_{den}_vs_{num}"] = fb.verdict_of(ratio, max(res[num]["spread"], res[den]["spread"]), den)
            for leg in legs:
                legs[leg][0]()
            emit(dict(section="linear", m=m, n=n, k=k, routes=routes, copies={leg: len(f) for leg, f in legs.items()},
                      **res, **rec, quant_error={leg: fb.quant_error(o[leg], o["bf16"]) for leg in ("w8a16", "w8a8")}))
        del w16, w8
        torch.cuda.empty_cache()


def prefill_cases(a, emit):
    from ch02 import CachedTransformerModel, Fp8WeightModel
    cfg, B, S = (32000, 2048, 16, 32, 8, 5632), 4, 512
    with torch.device(DEV):
        model = CachedTransformerModel(*cfg).to(DT).eval()
    models = {"w8a16": Fp8WeightModel.from_model(model), "w8a8": Fp8WeightModel.from_model(model).with_fp8_activations()}
    ids = torch.randint(0, cfg[0], (B, S), device=DEV)
    rel = lambda x, y: float((x.float() - y.float()).norm() / y.float().norm())  # noqa: E731
    with torch.no_grad():
        logits = {"bf16": model(ids)}
        for leg, mdl in models.items():
            logits[leg] = mdl(ids)  # also grows the W8A16 workspace, outside the timed windows
        torch.cuda.synchronize()
        times = {leg: [] for leg in models}
        for _ in range(a.repeats):
            for leg, mdl in models.items():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(a.prefills):
                    mdl(ids)
                stop.record()
                stop.synchronize()
                times[leg].append(start.elapsed_time(stop) * 1e-3 / a.prefills)
    res = {}
    for leg, t in times.items():
        med = statistics.median(t)
        res[leg] = {"ms": round(med * 1e3, 3), "spread": round((max(t) - min(t)) / med, 4),
                    "tokens_per_s": round(B * S / med)}
    ratio = res["w8a16"]["ms"] / res["w8a8"]["ms"]
    emit(dict(section="prefill", model="0.85B: 32000 / 2048 / 16 layers / 32-8 heads / 5632", batch=B, tokens=S, **res,
              w8a16_over_w8a8=round(ratio, 3),
              verdict=fb.verdict_of(ratio, max(res["w8a16"]["spread"], res["w8a8"]["spread"]), "w8a8"),
              logits_rel_l2={"w8a8_vs_w8a16": round(rel(logits["w8a8"], logits["w8a16"]), 5),
                             "w8a8_vs_bf16": round(rel(logits["w8a8"], logits["bf16"]), 5),
                             "w8a16_vs_bf16": round(rel(logits["w8a16"], logits["bf16"]), 5)}))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sections", default="linear,prefill")
    ap.add_argument("--footprint", type=int, default=512 << 20, help="bytes one walk over a leg's weight copies covers")
    ap.add_argument("--window", type=float, default=0.1, help="seconds of work per timed window")
    ap.add_argument("--max-replays", type=int, default=500, help="cap on graph replays per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per leg, alternating")
    ap.add_argument("--prefills", type=int, default=3, help="prefills per timed window of the prefill section")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("fp8a_gemm_bench: no ROCm device (there is no CPU path)", file=sys.stderr)
        return 1
    torch.manual_seed(9)
    head = {"tool": "fp8a_gemm_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16",
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

    sections = {"linear": linear_cases, "prefill": prefill_cases}
    for s in a.sections.split(","):
        sections[s](a, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
