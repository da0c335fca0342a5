"""Inputs, float64 references, the CPU emulation and the case list shared by the
tests of the fused RMSNorm + fp8-weight projection, pli_rms_gemm_nt_fp8w
(tests/test_gpu_decode_step_fp8w.py on the GPU,
tests/test_decode_step_fp8w_emulation_cpu.py on the CPU).  Guarded outputs,
padded row views, the bound and the norm's emulation are
tests/decode_step_cases.py's.

Activations and the norm weight are drawn as there.  Projection weights are
drawn N(0,1) * k**-0.5 in fp32 and quantised with pli_hip.quantize_weight_fp8:
absmax / 448 row scales, or (every other case) the smallest power of two above
them.  What the kernel sees is (codes, scale); the float64 reference is
oracle.linear.rms_linear / rms_swiglu over decode(code) * scale on the stored
h = a (+ residual), so the quantisation error is on neither side of the
comparison.  On request the codes are a uint8 view (ldw = k + 16) inside a
buffer of NaN codes (0x7F): one row above and below, 16 bytes in front of each
row -- the 16 bytes after a row are the next row's front padding.

`emulate` restates the documented semantics on the CPU: dc.emulate_norm's y
(h rounded, fp32 statistics, y rounded to the storage type), the fp32 dot over
the widened codes, the scale after the sum, SwiGLU in fp32, one rounding.

No case had to be replaced: the emulation alone stays at or below 0.5 of the
bound on every case, SwiGLU at K = 16 included (0.25 bf16 at M 2, at most 0.41
over M 1..4 and both widths; the 16-bit list's K = 8 SwiGLU sat at 0.61 and
was replaced there).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

import decode_step_cases as dc
import pli_hip
from decode_step_cases import (LIN_TOL, POS, S_MAX, Guarded, assert_untouched, emulate_norm, lin_ratio,  # noqa: F401
                               row_view, stored_h)
from oracle import linear as olin
from oracle.numerics import round_to_dtype, seeded_normal

TDT, DTYPES, EPS, TOKEN_SPLITS = dc.TDT, dc.DTYPES, dc.EPS, dc.TOKEN_SPLITS
NAN_CODE = 0x7F

# q: one (codes float8_e4m3fn [n, k], scale fp32 [n]) per width; qu: the up weights with swiglu
Fp8Operands = namedtuple("Fp8Operands", "a residual g q qu")


def pow2_scale(w: torch.Tensor) -> torch.Tensor:
    """the smallest power of two >= absmax / 448 per row (1 for a zero row)"""
    amax = w.float().abs().amax(dim=1)
    return torch.where(amax > 0, torch.exp2(torch.ceil(torch.log2(amax.clamp_min(1e-30) / 448.0))), torch.ones_like(amax))


def quantized(n: int, k: int, seed: int, pow2: bool, coarse: float = 1.0):
    """coarse > 1: scales that many times the usual ones, so the codes are that much smaller (for runs that ignore
    the scales and must keep silu(g) * u inside fp16)"""
    w = torch.from_numpy(seeded_normal((n, k), seed) * np.float32(k ** -0.5))
    if coarse != 1.0:
        return pli_hip.quantize_weight_fp8(w, scale=pow2_scale(w) * coarse)
    return pli_hip.quantize_weight_fp8(w, scale=pow2_scale(w) if pow2 else None)


def operands(k: int, m: int, widths, dt: str, seed: int, residual: bool = True, swiglu: bool = False,
             scale: float = 1.0, pow2: bool = False, coarse: float = 1.0) -> Fp8Operands:
    def act(s):
        return round_to_dtype(seeded_normal((m, k), s) * np.float32(scale), dt)

    g = round_to_dtype(1 + np.float32(0.1) * seeded_normal((k,), seed + 2), dt)
    return Fp8Operands(act(seed), act(seed + 1) if residual else None, g,
                       [quantized(n, k, seed + 3 + i, pow2, coarse) for i, n in enumerate(widths)],
                       [quantized(n, k, seed + 13 + i, pow2, coarse) for i, n in enumerate(widths)] if swiglu else None)


def dequantized(q) -> np.ndarray:
    """float64 decode(code) * scale (both exact in float64)"""
    codes, scale = q
    return codes.view(torch.float8_e4m3fn).double().numpy() * scale.double().numpy()[:, None]


def codes_view(q, device, padded: bool):
    """(codes, scale) on the device.  padded: uint8 columns 16 .. 16 + k of rows 1 .. n of an [n + 2, k + 16] buffer
    of NaN codes (ldw = k + 16, rows still 16-byte aligned); else the contiguous float8_e4m3fn tensor"""
    codes, scale = q
    scale = scale.to(device)
    if not padded:
        return codes.to(device), scale
    n, k = codes.shape
    buf = torch.full((n + 2, k + 16), NAN_CODE, dtype=torch.uint8, device=device)
    buf[1:n + 1, 16:] = codes.view(torch.uint8).to(device)
    return buf[1:n + 1, 16:], scale


# -------------------------------------------------------------- references
def reference(op: Fp8Operands, dt: str, eps: float, swiglu: bool):
    """float64 outputs [m, n_g] per group, on the stored h, over the dequantised weights"""
    h = dc.f64(stored_h(op, dt))
    if swiglu:
        return [olin.rms_swiglu(h, op.g, eps, dequantized(q), dequantized(qu)) for q, qu in zip(op.q, op.qu)]
    return [olin.rms_linear(h, op.g, eps, dequantized(q)) for q in op.q]


def emulate(op: Fp8Operands, dt: str, eps: float, swiglu: bool):
    """the kernel's semantics on the CPU -> float64 outputs per group"""
    y = emulate_norm(op, dt, eps).float()

    def dot(q):
        return (y @ q[0].float().t()) * q[1][None, :]

    outs = []
    for i, q in enumerate(op.q):
        r = dot(q)
        if swiglu:
            r = r / (1 + torch.exp(-r)) * dot(op.qu[i])
        outs.append(dc.f64(r.to(TDT[dt])))
    return outs


# ---------------------------------------------------------------- case list
# as dc.FusedCase, plus pow2: power-of-two scales
Fp8Case = namedtuple("Fp8Case", "kind K M B S widths padded res pos pow2")
# 16 one chunk; 2048 the last RPT 1 / short-row (ROWS, CPL) shape, one full trip; 2064 the first RPT 2 / long-row
# shape; 4096 the last RPT 2, one full long trip; 4112 the first RPT 4, a second trip of one chunk; 6160 1.5 trips;
# 8176 two trips less a chunk; 8192 two full trips and the largest row
KS = (16, 2048, 2064, 4096, 4112, 6160, 8176, 8192)
MS = (1, 2, 3, 4)


def _cases():
    main, lds = [], []
    kinds, res, pos = ("linear", "swiglu", "qkv"), ("res+h", "none", "res", "h"), ("mid", "zero", "last", "full")
    for ki, K in enumerate(KS):
        for M in MS:
            i = 4 * ki + M - 1
            kind = kinds[i % 3]
            if kind == "qkv":
                B, S = {1: (1, 1), 2: (2, 1), 3: (1, 3), 4: ((4, 1), (2, 2), (1, 4))[ki % 3]}[M]
                widths = (5, 3, 2)
            else:
                B, S = M, 1
                widths = (10,) if (i // 3) % 2 == 0 else (1,)
            c = Fp8Case(kind, K, M, B, S, widths, bool((i // 2) % 2), res[(i + ki) % 4],
                        pos[(ki + M) % 4] if kind == "qkv" else None, bool(i % 2))
            (lds if (K, M) == (8192, 4) else main).append(c)
    main += [
        Fp8Case("qkv", 2064, 4, 2, 2, (5, 3, 2), True, "res+h", "last", False),   # second token of each batch dropped
        Fp8Case("qkv", 4112, 4, 4, 1, (5, 3, 2), False, "none", "full", True),    # caches untouched, q written
        Fp8Case("qkv", 16, 4, 1, 4, (5, 3, 2), True, "res", "mid", False),
        Fp8Case("qkv", 6160, 3, 1, 3, (5, 3, 2), False, "res+h", "last", True),
        Fp8Case("qkv", 2048, 2, 2, 1, (5, 3, 2), True, "h", "zero", False),
        Fp8Case("qkv", 8176, 1, 1, 1, (5, 3, 2), False, "res+h", "full", True),
        Fp8Case("qkv", 2048, 4, 2, 2, (5, 3, 2), False, "res", "mid", True),      # the (2, 2) token split, short rows
        Fp8Case("linear", 4112, 2, 2, 1, (1,), True, "res+h", None, False),       # h_out at ntot 1: one workgroup
        Fp8Case("swiglu", 6160, 3, 3, 1, (1,), False, "res+h", None, True),
        # the SwiGLU instances the rotation above misses
        Fp8Case("swiglu", 2048, 1, 1, 1, (10,), True, "h", None, False),          # NB 1 x RPT 1
        Fp8Case("swiglu", 2048, 2, 2, 1, (10,), False, "none", None, True),       # NB 2 x RPT 1
        Fp8Case("swiglu", 2048, 4, 4, 1, (10,), True, "res", None, False),        # NB 4 x RPT 1
        Fp8Case("swiglu", 4096, 1, 1, 1, (10,), True, "h", None, True),           # NB 1 x RPT 2
        Fp8Case("swiglu", 2064, 2, 2, 1, (10,), False, "res+h", None, False),     # NB 2 x RPT 2
        Fp8Case("swiglu", 4096, 3, 3, 1, (1,), True, "res", None, True),          # NB 4 x RPT 2
        Fp8Case("swiglu", 8176, 1, 1, 1, (10,), False, "none", None, False),      # NB 1 x RPT 4
        Fp8Case("swiglu", 4112, 2, 2, 1, (10,), True, "res+h", None, True),       # NB 2 x RPT 4
    ]
    # m = 4, k = 8192: 65536 bytes of dynamic LDS + the 16 static; tests of their own
    lds += [Fp8Case("swiglu", 8192, 4, 4, 1, (10,), True, "res+h", None, False),
            Fp8Case("qkv", 8192, 4, 2, 2, (5, 3, 2), False, "res", "mid", True)]
    return main, lds


FP8W_CASES, FP8W_LDS_CASES = _cases()


def instance(c) -> tuple:
    """(SW, NB, ROWS, CPL, RPT) of the rms_gemm_fp8w instance pli_rms_gemm_nt_fp8w launches for the case"""
    sw = c.kind == "swiglu"
    short = c.K <= 2048
    rows, cpl = ((2, 2) if short else (1, 4)) if sw else ((4, 2) if short else (2, 4))
    return sw, 1 if c.M <= 1 else 2 if c.M <= 2 else 4, rows, cpl, 1 if short else 2 if c.K <= 4096 else 4


def all_instances() -> set:
    """every instance the library holds per storage type: SW x NB x the three (ROWS, CPL, RPT) forms"""
    out = set()
    for sw in (False, True):
        for nb in (1, 2, 4):
            out |= {(sw, nb, 2 if sw else 4, 2, 1), (sw, nb, 1 if sw else 2, 4, 2), (sw, nb, 1 if sw else 2, 4, 4)}
    return out


def self_test() -> None:
    """the list reaches every kernel instantiation, every (K, M) pair, every rotated property, and only token splits
    of dc.TOKEN_SPLITS"""
    cases = FP8W_CASES + FP8W_LDS_CASES
    missing = all_instances() - {instance(c) for c in cases}
    assert not missing, sorted(missing)
    assert {(c.K, c.M) for c in cases} == {(k, m) for k in KS for m in MS}
    for kind in ("linear", "swiglu", "qkv"):
        mine = [c for c in cases if c.kind == kind]
        assert {c.padded for c in mine} == {False, True} and {c.pow2 for c in mine} == {False, True}, kind
        assert {c.res for c in mine} == {"res+h", "none", "res", "h"}, kind
    assert {c.widths for c in cases} == {(10,), (1,), (5, 3, 2)}
    qkv = [c for c in cases if c.kind == "qkv"]
    assert {c.pos for c in qkv} == set(POS)
    assert {(c.B, c.S) for c in qkv} == set(TOKEN_SPLITS)
    assert all(c.B * c.S == c.M and c.K % 16 == 0 for c in cases)
    assert all((c.K, c.M) == (8192, 4) for c in FP8W_LDS_CASES) and not any((c.K, c.M) == (8192, 4) for c in FP8W_CASES)


self_test()


def case_id(c) -> str:
    return dc.case_id(c) + ("_pow2" if c.pow2 else "")


def case_seed(c, dt: str) -> int:
    return 2000 + 37 * c.K + 101 * c.M + 7 * len(c.widths) + 3 * c.S + (500 if dt == "fp16" else 0)


def case_operands(c, dt: str, scale: float = 1.0) -> Fp8Operands:
    return operands(c.K, c.M, c.widths, dt, case_seed(c, dt), residual=c.res.startswith("res"),
                    swiglu=c.kind == "swiglu", scale=scale, pow2=c.pow2)
