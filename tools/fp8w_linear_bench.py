#!/usr/bin/env python3
"""Weight-only fp8 linear (W8A16) against the bf16 calls, in one process.

    python tools/fp8w_linear_bench.py [--sections linear,swiglu,step] [--out FILE]
    python tools/fp8w_linear_bench.py --sections fused [--out FILE]

Sections (bf16 activations, N(0,1) weights, one fp32 scale per output row):
  linear  C = x W^T at W [n, k] in 4096^2, 8192^2, 14336 x 4096, 4096 x 14336
          and 32000 x 2048, each at M in {1, 4, 16, 64, 128}: pli_hip.gemv
          (M = 1) / pli_hip.gemm NT on bf16 weights against pli_hip.gemv_fp8w /
          pli_hip.linear_fp8w on the same weights quantised
  swiglu  14336 x 4096 at M in {1, 16}: pli_hip.gemm_swiglu against
          pli_hip.linear_swiglu_fp8w
  step    one decode step as one graph launch (ch08.DecodeStepGraph, prompt
          128) over the bf16 ch02.CachedTransformerModel and over
          ch02.Fp8WeightModel, batch 1 and 32: bench.py's 0.85B shape and four
          layers of a 4096-hidden / 32-8 heads / 14336 / 32000 shape (both past
          the Infinity Cache without copies); the error figure is the relative
          L2 distance of the prefill logits
  fused   (not in the default list) the fused norm + fp8 projection,
          pli_hip.rms_*_fp8w.  Kernel legs: pli_hip.rmsnorm (+ residual) then
          pli_hip.linear_fp8w / linear_swiglu_fp8w -- two launches per call in
          the leg's graph -- against the one fused launch, at 2048 -> 2048 +
          512 + 512 (q / k / v, the fused leg into a cache), 2048 -> 5632
          SwiGLU, 2048 -> 32000 and 4096 -> 14336 SwiGLU, M 1 and 4; the record
          says whether the two outputs are equal bit for bit (they are where
          the unfused projection takes linear_fp8w_vec).  Step legs: the step
          section's two models at batch 1 and 4, three graphs alternating: the
          bf16 model (fused step), Fp8WeightModel, and
          Fp8WeightModel(fused_decode=True)

Protocol (the one of tools/fp8_kv_bench.py): every leg owns enough copies of
its weights that one walk over them is past --footprint bytes (default 512
MiB, twice the 256 MiB Infinity Cache), so no call finds its weights cached.
A leg is ONE captured graph that walks its copies once; graphs are replayed
back to back and timed with device events, the two legs alternating, --repeats
windows each.  Reported per case: median time per call and the spread
((max - min) / median) of each leg, the weight bytes per second, the routes,
bf16 / fp8 (> 1: fp8 weights are faster) with whether the difference exceeds
both spreads, and the cost of quantising at this shape: max and rms of
|y_fp8 - y_bf16| relative to rms(y_bf16) (the format's error on N(0,1) data,
not the kernels').  One JSON line per case; there is no CPU path.
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

DT, DEV = torch.bfloat16, "cuda"
SHAPES = [(4096, 4096), (8192, 8192), (14336, 4096), (4096, 14336), (32000, 2048)]  # (n, k)
MS = [1, 4, 16, 64, 128]


def replay_time(graph, calls: int, replays: int) -> float:
    """seconds per call over `replays` back-to-back replays of a graph of `calls` calls"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(replays):
        graph.replay()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / (replays * calls)


def capture(fns):
    """one graph that runs every fn once, in order"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fns[0]()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for fn in fns:
            fn()
    return g


def copies(bytes_per_copy: int, footprint: int) -> int:
    return max(2, -(-footprint // bytes_per_copy))


def verdict_of(ratio: float, margin: float, name: str) -> str:
    return f"{name} faster" if ratio > 1 + margin else f"{name} slower" if ratio < 1 - margin else "within the spread"


def time_legs(a, legs: dict):
    """measure()'s protocol for any leg names: (routes, per-leg list of seconds per call, one per window)"""
    graphs, routes, replays = {}, {}, {}
    for leg, fns in legs.items():
        fns[0]()
        routes[leg] = pli_hip.last_route()
        graphs[leg] = capture(fns)
        est = replay_time(graphs[leg], len(fns), 2)
        replays[leg] = max(2, min(a.max_replays, int(a.window / max(est * len(fns), 1e-7))))
        replay_time(graphs[leg], len(fns), max(1, replays[leg] // 4))
    times = {leg: [] for leg in legs}
    for _ in range(a.repeats):
        for leg, fns in legs.items():
            times[leg].append(replay_time(graphs[leg], len(fns), replays[leg]))
    return routes, times


def measure(a, legs: dict, nbytes: dict) -> dict:
    """legs: name -> list of calls (one per weight copy)"""
    graphs, routes, replays = {}, {}, {}
    for leg, fns in legs.items():
        fns[0]()
        routes[leg] = pli_hip.last_route()
        graphs[leg] = capture(fns)
        est = replay_time(graphs[leg], len(fns), 2)
        replays[leg] = max(2, min(a.max_replays, int(a.window / max(est * len(fns), 1e-7))))
        replay_time(graphs[leg], len(fns), max(1, replays[leg] // 4))
    times = {leg: [] for leg in legs}
    for _ in range(a.repeats):
        for leg, fns in legs.items():
            times[leg].append(replay_time(graphs[leg], len(fns), replays[leg]))
    res = {"routes": routes, "copies": {leg: len(f) for leg, f in legs.items()}}
    for leg, t in times.items():
        med = statistics.median(t)
        res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4),
                    "weight_tbps": round(nbytes[leg] / med / 1e12, 3)}
    ratio = res["bf16"]["us"] / res["fp8"]["us"]
    margin = max(res["bf16"]["spread"], res["fp8"]["spread"])
    res["bf16_over_fp8"] = round(ratio, 3)
    res["verdict"] = "fp8 faster" if ratio > 1 + margin else "fp8 slower" if ratio < 1 - margin else "within the spread"
    return res


def quant_error(y8: torch.Tensor, y16: torch.Tensor) -> dict:
    d, r = (y8.float() - y16.float()), y16.float()
    rms = float(r.pow(2).mean().sqrt())
    return {"max_rel": round(float(d.abs().max()) / rms, 5), "rms_rel": round(float(d.pow(2).mean().sqrt()) / rms, 5)}


def make_weights(n: int, k: int, footprint: int, parts: int = 1):
    """bf16 copies and fp8 copies (codes, scale) of `parts` N(0,1) [n, k] weights each; fp8 copy 0 is bf16 copy 0
    quantised"""
    w16 = [[torch.randn(n, k, device=DEV).to(DT) for _ in range(parts)] for _ in range(copies(parts * n * k * 2, footprint))]
    w8 = []
    for i in range(copies(parts * n * k, footprint)):
        src = w16[0] if i == 0 else [torch.randn(n, k, device=DEV) for _ in range(parts)]
        w8.append([pli_hip.quantize_weight_fp8(w) for w in src])
    return w16, w8


def linear_cases(a, emit):
    for n, k in SHAPES:
        w16, w8 = make_weights(n, k, a.footprint)
        for m in MS:
            x = torch.randn(m, k, device=DEV).to(DT)
            o16, o8 = torch.empty(m, n, device=DEV, dtype=DT), torch.empty(m, n, device=DEV, dtype=DT)
            if m == 1:
                legs = {"bf16": [lambda w=w: pli_hip.gemv(w[0], x[0], out=o16[0]) for w in w16],
                        "fp8": [lambda w=w: pli_hip.gemv_fp8w(w[0][0], w[0][1], x[0], out=o8[0]) for w in w8]}
            else:
                legs = {"bf16": [lambda w=w: pli_hip.gemm(x, w[0], trans_b=True, out=o16) for w in w16],
                        "fp8": [lambda w=w: pli_hip.linear_fp8w(x, w[0][0], w[0][1], out=o8) for w in w8]}
            res = measure(a, legs, {"bf16": n * k * 2, "fp8": n * k + 4 * n})
            legs["bf16"][0]()
            legs["fp8"][0]()
            emit(dict(section="linear", m=m, n=n, k=k, quant_error=quant_error(o8, o16), **res))
        del w16, w8
        torch.cuda.empty_cache()


def swiglu_cases(a, emit):
    n, k = 14336, 4096
    w16, w8 = make_weights(n, k, a.footprint, parts=2)
    for m in (1, 16):
        x = torch.randn(m, k, device=DEV).to(DT)
        o16, o8 = torch.empty(m, n, device=DEV, dtype=DT), torch.empty(m, n, device=DEV, dtype=DT)
        legs = {"bf16": [lambda w=w: pli_hip.gemm_swiglu(x, w[0], w[1], out=o16) for w in w16],
                "fp8": [lambda w=w: pli_hip.linear_swiglu_fp8w(x, w[0][0], w[0][1], w[1][0], w[1][1], out=o8) for w in w8]}
        res = measure(a, legs, {"bf16": 2 * n * k * 2, "fp8": 2 * (n * k + 4 * n)})
        legs["bf16"][0]()
        legs["fp8"][0]()
        emit(dict(section="swiglu", m=m, n=n, k=k, quant_error=quant_error(o8, o16), **res))


def step_cases(a, emit):
    """ch08.DecodeStepGraph (one graph launch per token) over the bf16 model and over ch02.Fp8WeightModel"""
    from ch02 import CachedTransformerModel, Fp8WeightModel
    from ch08 import DecodeStepGraph
    prompt, steps = 128, 32
    for name, cfg in (("0.85B: 32000 / 2048 / 16 layers / 32-8 heads / 5632", (32000, 2048, 16, 32, 8, 5632)),
                      ("4 layers of 32000 / 4096 / 32-8 heads / 14336", (32000, 4096, 4, 32, 8, 14336))):
        with torch.device(DEV):
            model = CachedTransformerModel(*cfg).to(DT).eval()
        fq = Fp8WeightModel.from_model(model)
        for B in (1, 32):
            ids = torch.randint(0, cfg[0], (B, prompt), device=DEV)
            tok = torch.randint(0, cfg[0], (B, 1), device=DEV)
            graphs, logits = {}, {}
            with torch.no_grad():
                for leg, mdl in (("bf16", model), ("fp8", fq)):
                    g = DecodeStepGraph(mdl, B, prompt + steps * (a.repeats + 2) + 8, DT)
                    logits[leg] = g.prefill(ids).float()
                    g.step(tok)
                    graphs[leg] = g
                times = {leg: [] for leg in graphs}
                for _ in range(a.repeats):
                    for leg, g in graphs.items():
                        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        start.record()
                        for _ in range(steps):
                            g.step(tok)
                        stop.record()
                        stop.synchronize()
                        times[leg].append(start.elapsed_time(stop) * 1e-3 / steps)
            res = {}
            for leg, t in times.items():
                med = statistics.median(t)
                res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4)}
            ratio = res["bf16"]["us"] / res["fp8"]["us"]
            margin = max(res["bf16"]["spread"], res["fp8"]["spread"])
            verdict = "fp8 faster" if ratio > 1 + margin else "fp8 slower" if ratio < 1 - margin else "within the spread"
            rel = float((logits["fp8"] - logits["bf16"]).norm() / logits["bf16"].norm())
            emit(dict(section="step", model=name, batch=B, prompt=prompt, steps_per_window=steps, **res,
                      bf16_over_fp8=round(ratio, 3), verdict=verdict, prefill_logits_rel_l2=round(rel, 5),
                      weight_bytes={"bf16": sum(p.numel() * 2 for n, p in model.named_parameters() if "embed" not in n
                                                and "norm" not in n), "fp8": fq.quantized_bytes()}))
            del graphs
        del model, fq
        torch.cuda.empty_cache()


FUSED_KERNEL_SHAPES = [("qkv", 2048, (2048, 512, 512)), ("swiglu", 2048, (5632,)), ("linear", 2048, (32000,)),
                       ("swiglu", 4096, (14336,))]


def fused_kernel_cases(a, emit):
    """rmsnorm + linear_fp8w (two launches in one graph) against the one fused launch, M 1 and 4.  The qkv shape's
    unfused leg is the norm and the packed projection only (the model's third launch there, the cache append, is
    left out), its fused leg writes k / v into a cache at a device position."""
    eps, s_max, hd = 1e-6, 64, 64
    for kind, k, widths in FUSED_KERNEL_SHAPES:
        n = sum(widths)
        parts = 2 if kind == "swiglu" else 1
        w8 = [[pli_hip.quantize_weight_fp8(torch.randn(n, k, device=DEV)) for _ in range(parts)]
              for _ in range(copies(parts * n * k, a.footprint))]
        g = (1 + 0.1 * torch.randn(k, device=DEV)).to(DT)
        for m in (1, 4):
            x, r = torch.randn(m, k, device=DEV).to(DT), torch.randn(m, k, device=DEV).to(DT)
            h = torch.empty(m, k, device=DEV, dtype=DT)
            o_u, o_f = torch.empty(m, n, device=DEV, dtype=DT), torch.empty(m, n, device=DEV, dtype=DT)

            def unfused(w):
                _, y = pli_hip.rmsnorm(x, g, eps, residual=r)
                if kind == "swiglu":
                    pli_hip.linear_swiglu_fp8w(y, w[0][0], w[0][1], w[1][0], w[1][1], out=o_u)
                else:
                    pli_hip.linear_fp8w(y, w[0][0], w[0][1], out=o_u)

            if kind == "qkv":
                nq, nk = widths[0], widths[1]
                q = torch.empty(m, 1, nq, device=DEV, dtype=DT)
                kc, vc = (torch.zeros(m, s_max, nk // hd, hd, device=DEV, dtype=DT) for _ in range(2))
                pos = torch.full((1,), 5, dtype=torch.int32, device=DEV)

                def fused(w):
                    c, s = w[0]
                    pli_hip.rms_qkv_into_cache_fp8w(x.view(m, 1, k), g, eps, (c[:nq], s[:nq]),
                                                    (c[nq:nq + nk], s[nq:nq + nk]), (c[nq + nk:], s[nq + nk:]), q, kc,
                                                    vc, pos, residual=r.view(m, 1, k), h_out=h)
            elif kind == "swiglu":
                def fused(w):
                    pli_hip.rms_swiglu_fp8w(x, g, eps, w[0][0], w[0][1], w[1][0], w[1][1], residual=r, h_out=h, out=o_f)
            else:
                def fused(w):
                    pli_hip.rms_linear_fp8w(x, g, eps, w[0][0], w[0][1], residual=r, h_out=h, out=o_f)

            legs = {"unfused": [lambda w=w: unfused(w) for w in w8], "fused": [lambda w=w: fused(w) for w in w8]}
            routes, times = time_legs(a, legs)
            routes["unfused"] = "rmsnorm_vec+" + routes["unfused"]  # the leg's two launches (last_route names the last)
            res = {}
            for leg, t in times.items():
                med = statistics.median(t)
                res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4),
                            "weight_tbps": round(parts * (n * k + 4 * n) / med / 1e12, 3)}
            ratio = res["unfused"]["us"] / res["fused"]["us"]
            legs["unfused"][0]()
            legs["fused"][0]()
            if kind == "qkv":
                same = torch.equal(o_u[:, :nq], q[:, 0]) and torch.equal(o_u[:, nq:nq + nk], kc[:, 5].flatten(1))
            else:
                same = torch.equal(o_u, o_f)
            emit(dict(section="fused", leg_kind="kernel", kind=kind, m=m, k=k, widths=list(widths), routes=routes,
                      copies=len(w8), **res, unfused_over_fused=round(ratio, 3),
                      verdict=verdict_of(ratio, max(res["unfused"]["spread"], res["fused"]["spread"]), "fused"),
                      bitwise_equal=bool(same)))
        del w8
        torch.cuda.empty_cache()


def fused_step_cases(a, emit):
    """one decode step as one graph launch: the bf16 model (its own fused step), Fp8WeightModel unfused and
    Fp8WeightModel(fused_decode=True), alternating, batch 1 and 4"""
    from ch02 import CachedTransformerModel, Fp8WeightModel
    from ch08 import DecodeStepGraph
    prompt, steps = 128, 32
    for name, cfg in (("0.85B: 32000 / 2048 / 16 layers / 32-8 heads / 5632", (32000, 2048, 16, 32, 8, 5632)),
                      ("4 layers of 32000 / 4096 / 32-8 heads / 14336", (32000, 4096, 4, 32, 8, 14336))):
        with torch.device(DEV):
            model = CachedTransformerModel(*cfg).to(DT).eval()
        models = {"bf16_fused": model, "fp8_unfused": Fp8WeightModel.from_model(model),
                  "fp8_fused": Fp8WeightModel.from_model(model, fused_decode=True)}
        for B in (1, 4):
            ids = torch.randint(0, cfg[0], (B, prompt), device=DEV)
            tok = torch.randint(0, cfg[0], (B, 1), device=DEV)
            graphs, logits = {}, {}
            with torch.no_grad():
                for leg, mdl in models.items():
                    g = DecodeStepGraph(mdl, B, prompt + steps * (a.repeats + 2) + 8, DT)
                    g.prefill(ids)
                    logits[leg] = g.step(tok).float().clone()
                    graphs[leg] = g
                times = {leg: [] for leg in graphs}
                for _ in range(a.repeats):
                    for leg, g in graphs.items():
                        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        start.record()
                        for _ in range(steps):
                            g.step(tok)
                        stop.record()
                        stop.synchronize()
                        times[leg].append(start.elapsed_time(stop) * 1e-3 / steps)
            res = {}
            for leg, t in times.items():
                med = statistics.median(t)
                res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4)}
            sp = {leg: res[leg]["spread"] for leg in res}
            r_uf = res["fp8_unfused"]["us"] / res["fp8_fused"]["us"]
            r_bf = res["bf16_fused"]["us"] / res["fp8_fused"]["us"]
            emit(dict(section="fused", leg_kind="step", model=name, batch=B, prompt=prompt, steps_per_window=steps, **res,
                      fp8_unfused_over_fp8_fused=round(r_uf, 3),
                      verdict_vs_fp8_unfused=verdict_of(r_uf, max(sp["fp8_unfused"], sp["fp8_fused"]), "fp8 fused"),
                      bf16_fused_over_fp8_fused=round(r_bf, 3),
                      verdict_vs_bf16_fused=verdict_of(r_bf, max(sp["bf16_fused"], sp["fp8_fused"]), "fp8 fused"),
                      first_step_logits_equal_unfused=bool(torch.equal(logits["fp8_fused"], logits["fp8_unfused"])),
                      first_step_logits_rel_l2_vs_bf16=round(float((logits["fp8_fused"] - logits["bf16_fused"]).norm()
                                                                   / logits["bf16_fused"].norm()), 5)))
            del graphs
        del model, models
        torch.cuda.empty_cache()


def fused_cases(a, emit):
    fused_kernel_cases(a, emit)
    fused_step_cases(a, emit)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sections", default="linear,swiglu,step")
    ap.add_argument("--footprint", type=int, default=512 << 20, help="bytes one walk over a leg's weight copies covers")
    ap.add_argument("--window", type=float, default=0.1, help="seconds of work per timed window")
    ap.add_argument("--max-replays", type=int, default=500, help="cap on graph replays per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per leg, alternating")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("fp8w_linear_bench: no ROCm device (there is no CPU path)", file=sys.stderr)
        return 1
    torch.manual_seed(8)
    head = {"tool": "fp8w_linear_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16",
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

    sections = {"linear": linear_cases, "swiglu": swiglu_cases, "step": step_cases, "fused": fused_cases}
    for s in a.sections.split(","):
        sections[s](a, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
