#!/usr/bin/env python3
"""Token choice on the device (pli_sample) against torch's eager sampling chains,
in one process.

    python tools/sample_bench.py [--sections launch,step] [--out FILE]

Sections (bf16 logits):
  launch  the sampler alone on fixed logits [B, vocab], B in {1, 32}, vocab in
          {32000, 128256}.  Legs per sampling rule:
            torch        the reference's chain, eager, as today's loops run it --
                         topk: ch02/generation.py:23-31 (divide, topk, full_like
                         + scatter_, softmax, multinomial); topp: ch10/engine.py:
                         105-115 batched (softmax, sort, cumsum, mask, renorm,
                         scatter_, multinomial); greedy: argmax
            pli          pli_hip.sample with the same parameters, eager (one
                         launch from Python)
            pli_graph    the same call captured, `--calls` per graph: its device
                         time without the Python launch
  step    per-token time of a decode loop on bench.py's 0.85B shape (vocab
          32000) and the same model with vocab 128256, batch 1 and 32, prompt 128:
            torch_topk / torch_topp   today's loop: DecodeStepGraph.step() (one
                         graph launch, plus the copy of the ids into the static
                         buffer) followed by the eager chain
            sampled_topk / sampled_topp   DecodeStepGraph(sampler=...).
                         step_sampled(): one graph launch and nothing else

Protocol: every leg is warmed up, legs alternate within each of --repeats
windows, a window is timed with device events around back-to-back work that
ends in a synchronise.  Reported per leg: the median microseconds per call /
per token and the spread ((max - min) / median); per comparison torch / pli
(> 1: pli is faster) with whether the difference exceeds both spreads.  One
JSON line per case; there is no CPU path and no threshold.
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
import torch.nn.functional as F  # noqa: E402

import pli_hip  # noqa: E402

DT, DEV = torch.bfloat16, "cuda"
T, TOP_K, TOP_P = 0.8, 50, 0.9


def chain_topk(logits: torch.Tensor) -> torch.Tensor:
    """ch02/generation.py:23-31"""
    nl = logits / T
    values, indices = torch.topk(nl, TOP_K)
    nl = torch.full_like(nl, float("-inf")).scatter_(1, indices, values)
    return torch.multinomial(F.softmax(nl, dim=-1), num_samples=1)


def chain_topp(logits: torch.Tensor) -> torch.Tensor:
    """ch10/engine.py:105-115 over a batch"""
    probs = torch.softmax(logits / T, dim=-1)
    sp, si = torch.sort(probs, descending=True)
    cs = torch.cumsum(sp, dim=-1)
    sp[cs - sp > TOP_P] = 0.0
    sp = sp / sp.sum(-1, keepdim=True)
    probs = torch.zeros_like(probs).scatter_(1, si, sp)
    return torch.multinomial(probs, 1)


def chain_greedy(logits: torch.Tensor) -> torch.Tensor:
    return logits.argmax(-1, keepdim=True)


RULES = {
    "topk": (chain_topk, dict(temperature=T, top_k=TOP_K, top_p=1.0)),
    "topp": (chain_topp, dict(temperature=T, top_k=None, top_p=TOP_P)),
    "greedy": (chain_greedy, dict(temperature=0.0, top_k=None, top_p=1.0)),
}


def window(fn, calls: int) -> float:
    """seconds per call of `calls` back-to-back calls"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / calls


def alternate(a, legs: dict, calls: dict) -> dict:
    for leg, fn in legs.items():
        window(fn, max(2, calls[leg] // 4))
    times = {leg: [] for leg in legs}
    for _ in range(a.repeats):
        for leg, fn in legs.items():
            times[leg].append(window(fn, calls[leg]))
    res = {}
    for leg, t in times.items():
        med = statistics.median(t)
        res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4)}
    return res


def compare(res: dict, base: str, new: str) -> dict:
    ratio = res[base]["us"] / res[new]["us"]
    margin = max(res[base]["spread"], res[new]["spread"])
    verdict = f"{new} faster" if ratio > 1 + margin else f"{new} slower" if ratio < 1 - margin else "within the spread"
    return {f"{base}_over_{new}": round(ratio, 3), f"verdict_{new}_vs_{base}": verdict}


def launch_cases(a, emit):
    for vocab in (32000, 128256):
        for B in (1, 32):
            logits = (torch.randn(B, vocab, device=DEV) * 2).to(DT)
            out = torch.empty(B, dtype=torch.int64, device=DEV)
            pos = torch.zeros(1, dtype=torch.int32, device=DEV)
            for rule, (chain, kw) in RULES.items():
                def pli_call():
                    pli_hip.sample(logits, kw["temperature"], kw["top_k"], kw["top_p"], seed=7, offset=pos, out=out)

                pli_call()
                route = pli_hip.last_route()
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    pli_call()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    for _ in range(a.calls):
                        pli_call()
                        pos.add_(1)
                legs = {"torch": lambda: chain(logits), "pli": pli_call, "pli_graph": graph.replay}
                res = alternate(a, legs, {"torch": a.calls, "pli": a.calls, "pli_graph": 8})
                # (a replay is a.calls sampler launches and as many one-element adds of the offset)
                res["pli_graph"]["us"] = round(res["pli_graph"]["us"] / a.calls, 2)
                res["pli_graph"]["note"] = "per call, the offset's add_ included"
                emit(dict(section="launch", rule=rule, batch=B, vocab=vocab, route=route, **res,
                          **compare(res, "torch", "pli"), **compare(res, "torch", "pli_graph")))


def step_cases(a, emit):
    from ch02 import CachedTransformerModel, Sampler
    from ch08 import DecodeStepGraph
    prompt, steps = 128, a.steps
    for vocab in (32000, 128256):
        with torch.device(DEV):
            model = CachedTransformerModel(vocab, 2048, 16, 32, 8, 5632).to(DT).eval()
        for B in (1, 32):
            ids = torch.randint(0, vocab, (B, prompt), device=DEV)
            room = prompt + steps * (a.repeats + 2) + 8
            legs = {}
            with torch.no_grad():
                for rule in ("topk", "topp"):
                    chain, kw = RULES[rule]
                    g = DecodeStepGraph(model, B, room, DT)
                    state = {"tok": chain(g.prefill(ids)[:, -1])}

                    def today(g=g, chain=chain, state=state):
                        state["tok"] = chain(g.step(state["tok"])[:, -1])

                    gs = DecodeStepGraph(model, B, room, DT, sampler=Sampler(kw["temperature"], kw["top_k"], kw["top_p"], seed=7))
                    gs.prefill(ids, sample=True)
                    legs[f"torch_{rule}"] = today
                    legs[f"sampled_{rule}"] = gs.step_sampled
                res = alternate(a, legs, {leg: steps for leg in legs})
            emit(dict(section="step", model=f"{vocab} / 2048 / 16 layers / 32-8 heads / 5632", batch=B, prompt=prompt,
                      tokens_per_window=steps, **res, **compare(res, "torch_topk", "sampled_topk"),
                      **compare(res, "torch_topp", "sampled_topp")))
            del legs
        del model
        torch.cuda.empty_cache()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sections", default="launch,step")
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window of the launch section")
    ap.add_argument("--steps", type=int, default=32, help="tokens per timed window of the step section")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per leg, alternating")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("sample_bench: no ROCm device (there is no CPU path)", file=sys.stderr)
        return 1
    torch.manual_seed(8)
    head = {"tool": "sample_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16", "repeats": a.repeats,
            "temperature": T, "top_k": TOP_K, "top_p": TOP_P}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps({**head, **rec})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    sections = {"launch": launch_cases, "step": step_cases}
    for s in a.sections.split(","):
        sections[s](a, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
