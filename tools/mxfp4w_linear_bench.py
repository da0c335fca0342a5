#!/usr/bin/env python3
"""Weight-only MXFP4 linear (W4A16) against the fp8 (W8A16) and bf16 calls, in one process.

    python tools/mxfp4w_linear_bench.py [--sections gemv,linear,swiglu] [--out FILE]

Sections (bf16 activations, N(0,1) weights):
  gemv    M = 1 at 4096^2, 8192^2 and 16384^2: pli_hip.gemv (bf16), pli_hip.gemv_fp8w and pli_hip.gemv_mxfp4w
  linear  8192 x 8192 and 28672 x 8192 at M in {2, 4, 8, 16, 32, 64, 128}: pli_hip.linear_fp8w against
          pli_hip.linear_mxfp4w
  swiglu  14336 x 4096 at the same M: pli_hip.linear_swiglu_fp8w against pli_hip.linear_swiglu_mxfp4w
  routes  (not in the default list) mxfp4w_vec against mxfp4w_smallm on the same weights at M in {2, 4, 8, 16}, the
          rows both kernels take: the data behind the crossover in csrc/mxfp4w_plan.h

Protocol (the one of tools/fp8w_linear_bench.py): after a clock ramp, every leg owns enough copies of its weights
that one walk over them is past --footprint bytes (default 512 MiB, twice the 256 MiB Infinity Cache), so no call
finds its weights cached.  A leg is ONE captured graph that walks its copies once; graphs are replayed back to back
and timed with device events, the legs alternating, --repeats windows each.  Reported per case and leg: median time
per call, the A/A spread ((max - min) / median over the leg's windows), the bytes the call must move, bytes per
second and their fraction of the 6.5 TB/s streaming figure of DESIGN.md section 3, the route; and fp8 / mxfp4 (> 1:
MXFP4 weights are faster; the byte ratio bounds it at 1.88) with whether the difference exceeds both spreads.  One
JSON line per case; there is no CPU path.
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

import pli_hip  # noqa: E402
from fp8w_linear_bench import DEV, DT, copies, time_legs, verdict_of  # noqa: E402

STREAM_TBPS = 6.5
MS = [2, 4, 8, 16, 32, 64, 128]


def moved_bytes(kind: str, m: int, n: int, k: int, parts: int = 1) -> int:
    """compulsory bytes of one call: the weights (with their scales), x and the output"""
    w = {"bf16": n * k * 2, "fp8": n * k + 4 * n, "mxfp4": n * k // 2 + n * k // 32}[kind]
    return parts * w + 2 * m * (k + n)


def weights(kind: str, n: int, k: int, footprint: int, parts: int = 1):
    count = copies(moved_bytes(kind, 0, n, k, parts), footprint)
    make = {"bf16": lambda w: (w.to(DT),), "fp8": pli_hip.quantize_weight_fp8,
            "mxfp4": lambda w: pli_hip.quantize_weight_mxfp4(w, DT)}[kind]
    return [[make(torch.randn(n, k, device=DEV)) for _ in range(parts)] for _ in range(count)]


def report(a, section, m, n, k, legs, parts, emit):
    routes, times = time_legs(a, legs)
    res = {}
    for leg, t in times.items():
        med, nbytes = statistics.median(t), moved_bytes(leg, m, n, k, parts)
        res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4), "bytes": nbytes,
                    "tbps": round(nbytes / med / 1e12, 3), "of_stream": round(nbytes / med / 1e12 / STREAM_TBPS, 3),
                    "route": routes[leg]}
    ratio = res["fp8"]["us"] / res["mxfp4"]["us"]
    emit(dict(section=section, m=m, n=n, k=k, copies={leg: len(f) for leg, f in legs.items()}, **res,
              fp8_over_mxfp4=round(ratio, 3),
              verdict=verdict_of(ratio, max(res["fp8"]["spread"], res["mxfp4"]["spread"]), "mxfp4")))


def gemv_cases(a, emit):
    for n in (4096, 8192, 16384):
        w = {kind: weights(kind, n, n, a.footprint) for kind in ("bf16", "fp8", "mxfp4")}
        x, y = torch.randn(n, device=DEV).to(DT), torch.empty(n, device=DEV, dtype=DT)
        legs = {"bf16": [lambda c=c: pli_hip.gemv(c[0][0], x, out=y) for c in w["bf16"]],
                "fp8": [lambda c=c: pli_hip.gemv_fp8w(*c[0], x, out=y) for c in w["fp8"]],
                "mxfp4": [lambda c=c: pli_hip.gemv_mxfp4w(*c[0], x, out=y) for c in w["mxfp4"]]}
        report(a, "gemv", 1, n, n, legs, 1, emit)
        del w, legs
        torch.cuda.empty_cache()


def linear_cases(a, emit, shapes=((8192, 8192), (28672, 8192)), swiglu=False):
    parts = 2 if swiglu else 1
    for n, k in shapes:
        w = {kind: weights(kind, n, k, a.footprint, parts) for kind in ("fp8", "mxfp4")}
        for m in MS:
            x, o = torch.randn(m, k, device=DEV).to(DT), torch.empty(m, n, device=DEV, dtype=DT)
            if swiglu:
                legs = {"fp8": [lambda c=c: pli_hip.linear_swiglu_fp8w(x, *c[0], *c[1], out=o) for c in w["fp8"]],
                        "mxfp4": [lambda c=c: pli_hip.linear_swiglu_mxfp4w(x, *c[0], *c[1], out=o) for c in w["mxfp4"]]}
            else:
                legs = {"fp8": [lambda c=c: pli_hip.linear_fp8w(x, *c[0], out=o) for c in w["fp8"]],
                        "mxfp4": [lambda c=c: pli_hip.linear_mxfp4w(x, *c[0], out=o) for c in w["mxfp4"]]}
            report(a, "swiglu" if swiglu else "linear", m, n, k, legs, parts, emit)
        del w, legs
        torch.cuda.empty_cache()


def offset_out(m: int, n: int) -> torch.Tensor:
    """an [m, n] output 8 bytes off 16-byte alignment: the route rule then takes mxfp4w_vec where mxfp4w_smallm
    would run (the VALU kernel puts no condition on C)"""
    return torch.empty(m * n + 8, device=DEV, dtype=DT)[4:4 + m * n].view(m, n)


def route_cases(a, emit, shapes=((8192, 8192), (28672, 8192))):
    """mxfp4w_vec against mxfp4w_smallm on the same weights at the M both take"""
    for n, k in shapes:
        w = weights("mxfp4", n, k, a.footprint)
        for m in (2, 4, 8, 16):
            x, o, ov = torch.randn(m, k, device=DEV).to(DT), torch.empty(m, n, device=DEV, dtype=DT), offset_out(m, n)
            legs = {"smallm": [lambda c=c: pli_hip.linear_mxfp4w(x, *c[0], out=o) for c in w],
                    "vec": [lambda c=c: pli_hip.linear_mxfp4w(x, *c[0], out=ov) for c in w]}
            routes, times = time_legs(a, legs)
            res = {}
            for leg, t in times.items():
                med = statistics.median(t)
                res[leg] = {"us": round(med * 1e6, 2), "spread": round((max(t) - min(t)) / med, 4), "route": routes[leg]}
            ratio = res["smallm"]["us"] / res["vec"]["us"]
            emit(dict(section="routes", m=m, n=n, k=k, **res, smallm_over_vec=round(ratio, 3),
                      verdict=verdict_of(ratio, max(res["smallm"]["spread"], res["vec"]["spread"]), "vec")))
        del w, legs
        torch.cuda.empty_cache()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sections", default="gemv,linear,swiglu")
    ap.add_argument("--footprint", type=int, default=512 << 20, help="bytes one walk over a leg's weight copies covers")
    ap.add_argument("--window", type=float, default=0.1, help="seconds of work per timed window")
    ap.add_argument("--max-replays", type=int, default=500, help="cap on graph replays per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per leg, alternating")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("mxfp4w_linear_bench: no ROCm device (there is no CPU path)", file=sys.stderr)
        return 1
    torch.manual_seed(8)
    ramp = torch.randn(4096, 4096, device=DEV).to(DT)  # clock ramp: about a second of GEMMs before anything is timed
    for _ in range(300):
        pli_hip.gemm(ramp, ramp)
    torch.cuda.synchronize()
    head = {"tool": "mxfp4w_linear_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16",
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

    sections = {"gemv": gemv_cases, "linear": linear_cases, "routes": route_cases,
                "swiglu": lambda a, emit: linear_cases(a, emit, ((14336, 4096),), swiglu=True)}
    for s in a.sections.split(","):
        sections[s](a, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
