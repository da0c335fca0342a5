"""Route replay, case list, operands, float64 reference and the two per-element
bounds shared by the plain GEMM / GEMV tests (tests/test_gpu_gemm.py on the GPU,
tests/test_gemm_emulation_cpu.py and tests/test_gemm_capi.py on the CPU).  The
guarded outputs and the project's linear bound come from
tests/decode_step_cases.py; the form follows tests/swiglu_cases.py.

Route replay: `gemm_route` restates gemm_dispatch, splitk_slices /
splitk_target / splitk_variant, pli_gemm_workspace_size, launch_skinny /
_smallm / _midm / _splitk / _256 (csrc/gemm.hip), gemm_w5_ok and the persistent
rule of launch_gemm_w5 (gemm_w5.hip), gemm_w4v_ok (gemm_w4v.hip),
gemm_f32_mfma_ok and the NW rule of launch_gemm_f32_mfma (gemm_f32.hip);
`f32out_route` restates pli_gemm_f32out and `gemv_route` pli_gemv[_variant]
(gemv.hip).  Each returns Route(kernel, inst): the kernel as pli_last_route
reports it ("a+b" for two launches) and the template instance.  Every case names
the kernel and instance it is meant to reach and is asserted against the replay
when this module is imported (256 CUs); the GPU test asserts the name against
pli_hip.last_route().  Cases whose instance depends on the CU count (the
persistent gemm_w5 walk, gemm_f32_mfma's four-wave form) are built by
`device_cases(cus)` from the device's count.

Operands: a [m, k] = N(0,1) * 0.5, b [n, k] (NT) or [k, n] (NN) = N(0,1) *
k^-0.5, bias [n] = N(0,1), seeded per case and type and rounded to the storage
type.  Kind "large" (once per route): a and b unscaled N(0,1), so |ref| ~ sqrt(k)
and the output rounding dominates.

Padded family: a is a view with lda = k + 8, b one with ldb = k + 16 (NT) or
n + 16 (NN), NaN in all row padding and in three spare rows after each; the
bias sits 8 elements into a NaN-filled buffer; the output is a Guarded
[m + 3, n] with ldc = n + 8.  Modes that leave the vector class: "ld2" (lda =
k + 2), "offa" (a starts one element into its storage), "bias2" (the bias
pointer 2 bytes past a 16-byte boundary); "bias8" (8 bytes past it) stays in
it.  The contiguous family has ld == k (ldc == n).

Bounds, per element, both asserted:

(a) the project's bound |err| <= LIN_TOL * (|ref| + 1), bf16 1e-2, fp16 4e-3;
    fp32 outputs 1e-4 * (|ref| + 1), gemm_f32_mfma 4e-6 * k + 1e-5 absolute;
(b) |err| <= NORM_SLACK * u * |ref| + (K + 2) * 2^-23 * mag + MIN_NORMAL,
    u the unit roundoff of the output type (2^-8 / 2^-11 / 2^-24) and mag =
    |a| |b|^T + |bias| in float64: one output rounding plus twice the
    first-order error of a length-K fp32 dot in any order and one fp32 bias
    add.  Any summation tree over K products is within K * 2^-24 * sum
    |products| to first order, so the split-K planes and the four-wave LDS sums
    are covered.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np
import torch

from decode_step_cases import HALF_ULP, LIN_TOL, MIN_NORMAL, NORM_SLACK, TDT, Guarded, f64  # noqa: F401
from oracle.numerics import round_to_dtype, seeded_normal

TDT3 = dict(TDT, fp32=torch.float32)
TOL_A = dict(LIN_TOL, fp32=1e-4)
ROUND = dict(HALF_ULP, fp32=2.0 ** -24)            # the unit roundoff of the output type
FLOOR = dict(MIN_NORMAL, fp32=2.0 ** -126)
DTYPE_CODE = {"fp32": 0, "fp16": 1, "bf16": 2}
BITS = {"fp32": torch.int32, "fp16": torch.int16, "bf16": torch.int16}
B16 = ("bf16", "fp16")

SKINNY, SMALLM, MIDM, MFMA, G256, W5, W4V, F32MFMA, GENERIC = (
    "gemm_skinny_nt", "gemm_smallm_nt", "gemm_midm_nt", "gemm_mfma", "gemm_256", "gemm_w5", "gemm_w4v",
    "gemm_f32_mfma", "gemm_generic")
SPLIT_D, SPLIT_L, REDUCE = "gemm_splitk_nt", "gemm_splitk_lds_nt", "gemm_splitk_reduce"
F32OUT_GENERIC = "gemm_f32out_generic"
GEMV_VEC, GEMV_SCALAR = "gemv_vec", "gemv_scalar"

Route = namedtuple("Route", "kernel inst")


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ------------------------------------------------------------- route replay
def splitk_slices(m: int, n: int, k: int, target: int, max_m: int = 256) -> int:
    """pli::splitk_slices: the largest power of two with tiles * ks <= target, slices >= 256 and % 64 == 0"""
    if m <= 16 or m > max_m or n % 32 != 0 or k % 64 != 0 or k < 64:
        return 0
    tiles = cdiv(n, 128) * cdiv(m, 128)
    ks = 1
    while tiles * ks * 2 <= target and k % (ks * 2 * 64) == 0 and k // (ks * 2) >= 256:
        ks *= 2
    return ks


def splitk_target(v: int) -> int:
    return 512 if v in (0, 22, 26, 28) else 128 if v in (24, 27, 29) else 256


def splitk_variant(v: int) -> bool:
    return v in (0, 22, 24) or 25 <= v <= 29


def workspace_size(m: int, n: int, k: int, trans_b, dt: str) -> int:
    """pli_gemm_workspace_size: ks planes of m * n fp32 for the most slices any variant uses; 0 where ks <= 1"""
    if not trans_b or dt == "fp32" or m <= 0 or n <= 0 or k <= 0:
        return 0
    ks = splitk_slices(m, n, k, splitk_target(22), 2048)
    return ks * m * n * 4 if ks > 1 else 0


def w5_ok(n: int, k: int, lda: int, ldb: int, trans_b) -> bool:
    return (k >= 64 and k % 64 == 0 and n % 8 == 0 and n >= 8 and lda * 512 < 2 ** 31
            and ldb * 2 * (256 if trans_b else 64) < 2 ** 31)


def w4v_ok(n: int, k: int, lda: int, ldb: int, trans_b) -> bool:
    return (k >= 32 and k % 32 == 0 and n % 8 == 0 and n >= 8 and lda * 512 < 2 ** 31
            and ldb * 2 * (256 if trans_b else 32) < 2 ** 31)


def _w5_inst(m: int, n: int, k: int, persistent: bool, cus: int, f32: bool = False) -> str:
    """launch_gemm_w5: the persistent instance needs k >= 128; it walks only with more tiles than cus / 8 * 8"""
    nb, g = cdiv(m, 256) * cdiv(n, 256), cus // 8 * 8
    form = "tile" if not persistent or k < 128 else "persistent" if g >= 8 and nb > g else "persistent1"
    return ("w5 f32 " if f32 else "w5 ") + form


SKINNY_CPL = ((128, 2), (256, 4), (512, 8), (768, 12), (1024, 16))


def _skinny_inst(m: int, k: int) -> str:
    nb = 1 if m <= 1 else 2 if m <= 2 else 4 if m <= 4 else 8 if m <= 8 else 16
    cpl = 8 if nb > 4 else next((c for lim, c in SKINNY_CPL if k // 8 <= lim), 8)
    return f"NB{nb},CPL{cpl}"


def _mc(m: int) -> int:
    return cdiv(min(m, 128), 32)


def _tb(trans_b) -> str:
    return "NT" if trans_b else "NN"


GEMV_VARIANTS = {  # rows per wave, chunks per lane, non-temporal, waves per block
    0: (2, 8, True, 4), 1: (4, 8, True, 4), 2: (1, 8, True, 4), 3: (2, 8, False, 4), 4: (4, 4, True, 4),
    5: (8, 4, True, 4), 6: (2, 8, True, 1), 7: (2, 8, True, 8), 8: (1, 8, True, 2), 9: (1, 4, True, 2),
    10: (2, 4, True, 4), 11: (1, 4, True, 4), 12: (1, 8, True, 1), 13: (1, 8, True, 4), 14: (1, 8, False, 2),
    15: (1, 2, True, 2), 16: (2, 2, True, 4)}


def gemv_route(m: int, k: int, dt: str, ldw=None, aligned: bool = True, variant=None) -> Route:
    """The launch of pli_gemv[_variant] for m, k > 0 (variant None = the default rule 16 / 9 / 8); aligned: w and
    x 16-byte aligned."""
    epc = 4 if dt == "fp32" else 8
    ldw = k if ldw is None else ldw
    if k % epc or ldw % epc or not aligned:
        return Route(GEMV_SCALAR, "")
    nch = k // epc
    if variant is None or variant < 0:
        variant = 16 if nch <= 128 else 9 if m >= 16384 and nch <= 256 else 8
    rows, cpl, ntl, wpb = GEMV_VARIANTS[variant]
    return Route(GEMV_VEC, "R{},CPL{},{},WPB{},{}".format(rows, cpl, "nt" if ntl else "plain", wpb,
                                                          "exact" if nch % (64 * cpl) == 0 else "clamped"))


def gemm_route(m: int, n: int, k: int, dt: str, trans_b, bias, variant, workspace, lds=None, aligned: bool = True,
               bias_aligned: bool = True, cus: int = 256) -> Route:
    """The launch of pli_gemm[_variant | _ws | _ws_variant] for m, n > 0.  variant None = 0; workspace: the bytes
    the call passes with a non-null pointer (0 / None: no workspace; True: any size); lds = (lda, ldb, ldc), default
    contiguous; aligned: a, b and c 16-byte aligned; bias_aligned: the bias pointer 8-byte aligned."""
    v = variant or 0
    lda, ldb, ldc = lds or (k, k if trans_b else n, n)
    gen = Route(GENERIC, ("f32," if dt == "fp32" else "16,") + _tb(trans_b))
    if k == 0:
        return gen
    vec = (dt != "fp32" and k % 8 == 0 and n % 8 == 0 and lda % 8 == 0 and ldb % 8 == 0 and ldc % 8 == 0 and aligned
           and (not bias or bias_aligned))
    if vec and trans_b and m == 1:
        return Route(SKINNY, _skinny_inst(m, k)) if bias else gemv_route(n, k, dt, ldb)
    have = float("inf") if workspace is True else int(workspace or 0)
    short_k = k <= 2048 and m <= 128 and n < 16384 and (m <= 32 or n // 128 >= 64)
    few_tiles = 256 < m <= 2048 and cdiv(m, 256) * cdiv(n, 256) < 128
    if (vec and trans_b and splitk_variant(v) and have > 0 and not (v == 0 and short_k)
            and (v != 0 or m <= 256 or few_tiles)):
        target = 128 if v == 0 and m > 256 and k < 4096 else splitk_target(v)
        ks = splitk_slices(m, n, k, target, 2048 if v == 0 or v >= 25 else 256)
        if ks >= 1 and (ks == 1 or have >= ks * m * n * 4):
            lds_k = v == 0 or v >= 25
            inst = "MC{},ks{},{},{},{}".format(_mc(m), ks, "lds" if lds_k else "direct", "NB3" if v in (28, 29) else "NB2",
                                               "partial" if ks > 1 else "direct-store")
            return Route((SPLIT_L if lds_k else SPLIT_D) + ("+" + REDUCE if ks > 1 else ""), inst)
    if vec and trans_b and k % 256 == 0 and ((v == 20 and m <= 256) or (v == 0 and 32 < m <= 128)):
        return Route(MIDM, f"MC{_mc(m)}")
    if vec and trans_b and m <= 128 and k % 128 == 0 and n % 16 == 0:
        return Route(SMALLM, "NBG{}".format(1 if m <= 16 else 2 if m <= 32 else 4 if m <= 64 else 8))
    if vec and trans_b and m <= 16:
        return Route(SKINNY, _skinny_inst(m, k))
    if v == 40 and vec and w4v_ok(n, k, lda, ldb, trans_b):
        return Route(W4V, "")
    if v == 41 and vec and w5_ok(n, k, lda, ldb, trans_b):
        return Route(W5, _w5_inst(m, n, k, False, cus))
    if v == 43 and vec and m % 256 == 0 and n % 256 == 0 and w5_ok(n, k, lda, ldb, trans_b):
        return Route(W5, _w5_inst(m, n, k, True, cus))
    big = (vec and k % 64 == 0 and m >= 512 and n >= 512 and v != 1
           and (v != 0 or cdiv(m, 256) * cdiv(n, 256) >= 128))
    if v == 0 and big and w5_ok(n, k, lda, ldb, trans_b):
        return Route(W5, _w5_inst(m, n, k, m % 256 == 0 and n % 256 == 0 and k >= 128, cus))
    if big or (vec and v >= 2 and k % 64 == 0 and n >= 8):
        phased = 0 if v == 3 else 2 * (v - 5) + 1 if 5 <= v <= 8 else -1
        group_m = 0
        if v == 0:
            phased, group_m = (-1 if trans_b and k <= 4096 else 7), 4
        if 9 <= v <= 11:
            group_m = 4 << (v - 9)
        if 12 <= v <= 15:
            phased, group_m = 7, {12: 8, 13: 4, 14: 2, 15: 16}[v]
        if phased >= 0:
            return Route(G256, f"256p SCHED{phased} g{group_m}")
        return Route(G256, f"256 g{group_m}" + (" prio" if v == 4 else ""))
    if vec:
        return Route(MFMA, "")
    if dt == "fp32" and aligned and k % 4 == 0 and lda % 4 == 0 and ldb % 4 == 0 and (trans_b or n % 4 == 0):
        return Route(F32MFMA, "f32 NW8" if cdiv(n, 128) * cdiv(m, 128) < 2 * cus else "f32 NW4")
    return gen


def f32out_route(m: int, n: int, k: int, dt: str, lds=None, aligned: bool = True, cus: int = 256) -> Route:
    """The launch of pli_gemm_f32out for m, n > 0; lds = (lda, ldb); aligned: a, b and c 16-byte aligned."""
    lda, ldb = lds or (k, k)
    lds_ok = k % 64 == 0 and k > 0 and n % 32 == 0 and lda % 8 == 0 and ldb % 8 == 0 and aligned
    if lds_ok and m >= 512 and n >= 512 and cdiv(m, 256) * cdiv(n, 256) >= 128 and w5_ok(n, k, lda, ldb, True):
        return Route(W5, _w5_inst(m, n, k, m % 256 == 0 and n % 256 == 0 and k >= 128, cus, f32=True))
    if lds_ok:
        return Route(SPLIT_L, f"MC{_mc(m)},f32")
    return Route(F32OUT_GENERIC, "")


# ---------------------------------------------------------------- case list
# api: "gemm" | "f32out" | "gemv" (gemv: m rows of W, n unused = 0, trans_b / bias unused)
# ws: "auto" = what pli_hip.gemm passes (pli_gemm_workspace_size bytes for the split-K variants), 0 = none and
#     "min" = 16 bytes (the one-slice routes need a non-null workspace), both through the C ABI
# mode: "pad" | "ld2" | "offa" | "bias2" | "bias8" | "offc" (pli_gemm_f32out into a C 4 bytes past a 16-byte boundary)
GemmCase = namedtuple("GemmCase", "api kernel inst m n k trans_b bias variant ws kind mode dts")
SPLIT_VARIANTS = (None, 0, 22, 24, 25, 26, 27, 28, 29)


def _case(kernel, inst, mnk, tb=True, bias=False, variant=None, ws="auto", kind="default", mode="pad", dts=B16,
          api="gemm"):
    return GemmCase(api, kernel, inst, *mnk, bool(tb), bool(bias), variant, ws, kind, mode, dts)


def _gemv_inst(variant: int, k: int, dt: str) -> str:
    rows, cpl, ntl, wpb = GEMV_VARIANTS[variant]
    exact = (k // (4 if dt == "fp32" else 8)) % (64 * cpl) == 0
    return "R{},CPL{},{},WPB{},{}".format(rows, cpl, "nt" if ntl else "plain", wpb, "exact" if exact else "clamped")


SKINNY_KS = (8, 1024, 1032, 2048, 2056, 4096, 4104, 6144, 6152, 8192, 8200)
SKINNY_K_CPL = {8: 2, 1024: 2, 1032: 4, 2048: 4, 2056: 8, 4096: 8, 4104: 12, 6144: 12, 6152: 16, 8192: 16, 8200: 8}
SKINNY_NS = (8, 24, 40)          # odd multiples of 8: the last workgroup of the cdiv(N, 2) grid is half used


def _gemm_cases():
    cs = []
    # gemm_skinny_nt<NB, CPL>: NB 1 / 2 / 4 pick CPL by K (each side of every boundary), NB 8 / 16 keep CPL 8.
    # M = 1 reaches it with a bias only (without one it is gemv_vec, below)
    for i, k in enumerate(SKINNY_KS):
        n = SKINNY_NS[i % 3]
        cs.append(_case(SKINNY, f"NB1,CPL{SKINNY_K_CPL[k]}", (1, n, k), bias=True))
        for bias in (False, True):
            cs.append(_case(SKINNY, f"NB2,CPL{SKINNY_K_CPL[k]}", (2, n, k), bias=bias))
            cs.append(_case(SKINNY, f"NB4,CPL{SKINNY_K_CPL[k]}", (3 + (i + bias) % 2, n, k), bias=bias))
        # gemv_vec through pli_gemm (M = 1, no bias): N rows of K; <= 128 chunks variant 16, else 8
        cs.append(_case(GEMV_VEC, _gemv_inst(16 if k <= 1024 else 8, k, "bf16"), (1, n, k)))
    for i, k in enumerate((8, 2048, 2056, 4104)):
        for bias in (False, True):
            cs.append(_case(SKINNY, "NB8,CPL8", ((5, 8)[(i + bias) % 2], SKINNY_NS[i % 3], k), bias=bias))
            cs.append(_case(SKINNY, "NB16,CPL8", ((9, 16)[(i + bias) % 2], SKINNY_NS[(i + 1) % 3], k), bias=bias))
    # gemm_smallm_nt<NBG, BIAS>: kw = K / 4 per wave, one body step is K = 512.  K 128 remainder only, 512 one
    # body step, 640 / 1152 body + remainder, 1024 two steps.  Variant 21 where the default is the mid-M kernel
    # (32 < M <= 128 with K % 256 == 0)
    for j, (nbg, m) in enumerate(((1, 2), (1, 16), (2, 17), (2, 32), (4, 33), (4, 64), (8, 65), (8, 128))):
        for i, k in enumerate((128, 512, 640, 1152, 1024)):
            cs.append(_case(SMALLM, f"NBG{nbg}", (m, (16, 48)[(i + j) % 2], k), bias=(i + j // 2) % 2,
                            variant=21 if m > 32 and k % 256 == 0 else None))
    # gemm_midm_nt<MC, BIAS> through variant 20 (M <= 256, K % 256 == 0): K 256 one step per wave, 512 one pass of
    # the two-step loop, 768 loop + tail; N 40: a column group cut by n >= N; M 129 / 256: second slabs of 1 / 128 rows
    for j, m in enumerate((17, 33, 65, 97, 128, 129, 256)):
        for i, k in enumerate((256, 512, 768)):
            cs.append(_case(MIDM, f"MC{_mc(m)}", (m, (32, 40)[(i + j) % 2], k), bias=(i + j) % 2 == 0, variant=20))
    cs += [_case(MIDM, "MC3", (65, 8200, 256), bias=True, variant=20), _case(MIDM, "MC1", (30, 8200, 256), variant=20),
           _case(MIDM, "MC2", (64, 8192, 256)),                       # the default: short K and N / 128 >= 64
           _case(MIDM, "MC2", (64, 32, 4096), bias=True, ws=0)]       # the default without a workspace
    # the split-K kernels: gemm_splitk_nt<MC, PARTIAL, BIAS> (22 / 24) and gemm_splitk_lds_nt<MC, PARTIAL, BIAS, NB>
    # (default, 25 - 27 NB 2, 28 / 29 NB 3) + gemm_splitk_reduce<BIAS>.  One slice (direct store) needs a non-null
    # workspace of any size: the C ABI.  Slices of 64 / 128 / 192 / 256 = 1 - 4 steps.
    for v, kern, form in ((22, SPLIT_D, "direct,NB2"), (24, SPLIT_D, "direct,NB2"), (25, SPLIT_L, "lds,NB2"),
                          (26, SPLIT_L, "lds,NB2"), (28, SPLIT_L, "lds,NB3"), (29, SPLIT_L, "lds,NB3")):
        for j, m in enumerate((17, 33, 65, 97)):
            for bias in (False, True):
                k = (64, 128, 192, 256)[(j + bias + v) % 4]
                cs.append(_case(kern, f"MC{j + 1},ks1,{form},direct-store", (m, (32, 160)[(j + bias) % 2], k), bias=bias,
                                variant=v, ws="min"))
            ks = (2, 4, 8, 2)[(j + v) % 4]
            cs.append(_case(kern + "+" + REDUCE, f"MC{j + 1},ks{ks},{form},partial", (m, (32, 160, 288)[(j + v) % 3], 256 * ks),
                            bias=(j + v) % 2, variant=v))
    for v, kern, form in ((22, SPLIT_D, "direct,NB2"), (27, SPLIT_L, "lds,NB2"), (28, SPLIT_L, "lds,NB3")):
        # NB 3 ring at 1, 2 and 3 steps per slice on every variant family; second slabs of 1, 2 and 128 rows
        for k in (64, 128, 192):
            cs.append(_case(kern, f"MC4,ks1,{form},direct-store", (128, 32, k), bias=k == 128, variant=v, ws="min"))
        for m, n, k, ks in ((129, 32, 512, 2), (130, 160, 1024, 4), (256, 288, 512, 2)):
            cs.append(_case(kern + "+" + REDUCE, f"MC4,ks{ks},{form},partial", (m, n, k), bias=m == 130, variant=v))
    # the default: M <= 256 past short K, and the few-tile route 256 < M <= 2048 (target 128 below K 4096, else 512)
    cs += [_case(SPLIT_L + "+" + REDUCE, "MC1,ks16,lds,NB2,partial", (17, 32, 4096)),
           _case(SPLIT_L + "+" + REDUCE, "MC3,ks2,lds,NB2,partial", (65, 160, 512), bias=True),
           _case(SPLIT_L + "+" + REDUCE, "MC4,ks4,lds,NB2,partial", (129, 32, 1024)),
           _case(SPLIT_L + "+" + REDUCE, "MC4,ks2,lds,NB2,partial", (257, 32, 512), bias=True),
           _case(SPLIT_L + "+" + REDUCE, "MC4,ks2,lds,NB2,partial", (520, 160, 512)),
           _case(SPLIT_L + "+" + REDUCE, "MC4,ks16,lds,NB2,partial", (257, 32, 4096)),
           _case(SPLIT_L + "+" + REDUCE, "MC4,ks16,lds,NB2,partial", (520, 160, 4096), bias=True),
           _case(SPLIT_L, "MC4,ks1,lds,NB2,direct-store", (257, 32, 192), ws="min"),
           _case(SPLIT_L, "MC2,ks1,lds,NB2,direct-store", (64, 32, 4160), bias=True, ws="min")]   # 65 steps: no doubling
    # gemm_mfma<T, TB, BIAS>: 128 x 128 outputs per workgroup, K tiles of 64 (K 72: a tail of 8); M 129: a one-row
    # second tile
    for i, k in enumerate((8, 64, 72, 192)):
        for tb in (True, False):
            for bias in (False, True):
                cs.append(_case(MFMA, "", (129, (8, 72, 136)[(i + tb + bias) % 3], k), tb=tb, bias=bias))
    cs += [_case(MFMA, "", (17, 8, 8)), _case(MFMA, "", (130, 136, 72), bias=True, mode="bias8"),
           _case(MFMA, "", (130, 136, 72), tb=False, bias=True, mode="bias8")]
    # gemm_256<T, TB, BIAS, PRIO> (variants 2, 4; 9 - 11 group_m 4 / 8 / 16) and gemm_256p<T, TB, BIAS, SCHED>
    # (3, 5 - 8 SCHED 0 / 1 / 3 / 5 / 7; 12 - 15 SCHED 7 with group_m 8 / 4 / 2 / 16), forced at the small shapes
    # the rule variant >= 2 && k % 64 == 0 && n >= 8 admits.  The default reaches them only where gemm_w5_ok
    # refuses a >= 128-tile shape, i.e. from a leading dimension of 2^22 on: no small allocation does, so the forced
    # variants are the coverage
    shapes = ((257, 264), (300, 520), (512, 768))
    i = 0
    for v, inst in ((2, "256 g0"), (4, "256 g0 prio"), (3, "256p SCHED0 g0"), (5, "256p SCHED1 g0"), (6, "256p SCHED3 g0"),
                    (7, "256p SCHED5 g0"), (8, "256p SCHED7 g0")):
        for tb in (True, False):
            for bias in (False, True):
                cs.append(_case(G256, inst, (*shapes[i % 3], (64, 128, 192)[(i // 3 + i) % 3]), tb=tb, bias=bias, variant=v))
                i += 1
    for v, inst, g in ((9, "256 g4", 4), (10, "256 g8", 8), (11, "256 g16", 16), (12, "256p SCHED7 g8", 8),
                       (13, "256p SCHED7 g4", 4), (14, "256p SCHED7 g2", 2), (15, "256p SCHED7 g16", 16)):
        # more row tiles than the group and a last group that is not full: g + 2 row tiles, 2 column tiles
        cs.append(_case(G256, inst, (256 * (g + 1) + 1, 264, 64), tb=v % 2, bias=v % 3 == 0, variant=v))
    # gemm_w5 (41; 43 with M, N % 256 == 0: the one-tile form below K 128, else the persistent instance with one
    # tile per workgroup) and gemm_w4v (40, K tiles of 32)
    for tb in (True, False):
        for bias in (False, True):
            cs += [_case(W5, "w5 tile", (256, 256, 64), tb=tb, bias=bias, variant=41),
                   _case(W5, "w5 tile", (300, 520, 192), tb=tb, bias=not bias, variant=41),
                   _case(W4V, "", (256, 256, 64), tb=tb, bias=bias, variant=40),
                   _case(W4V, "", (300, 520, 192), tb=tb, bias=not bias, variant=40),
                   _case(W4V, "", (257, 264, 32), tb=tb, bias=bias, variant=40),
                   _case(W4V, "", (257, 264, 96), tb=tb, bias=not bias, variant=40),
                   _case(W5, "w5 tile", (256, 256, 64), tb=tb, bias=bias, variant=43),
                   _case(W5, "w5 persistent1", (256, 512, 128 + 64 * bias), tb=tb, bias=bias, variant=43)]
    # gemm_f32_mfma<TB, NW 8> (fewer than 2 * CUs tiles of 128^2; NW 4 in device_cases)
    for tb in (True, False):
        for bias in (False, True):
            cs.append(_case(F32MFMA, "f32 NW8", (129, 136, 36), tb=tb, bias=bias, dts=("fp32",)))
    # gemm_generic<T, TB>: fp32 outside the MFMA class (NN with n % 4, k % 4, ld % 4) and 16-bit outside the vector
    # class (n % 8, k % 8, lda % 8, a pointer 2 bytes off, a bias pointer 2 bytes off)
    cs += [_case(GENERIC, "f32,NT", (1, 1, 1), dts=("fp32",)),
           _case(GENERIC, "f32,NN", (1, 1, 1), tb=False, bias=True, dts=("fp32",)),
           _case(GENERIC, "f32,NT", (65, 33, 17), bias=True, dts=("fp32",)),
           _case(GENERIC, "f32,NN", (65, 33, 17), tb=False, dts=("fp32",)),
           _case(GENERIC, "f32,NN", (65, 34, 36), tb=False, bias=True, dts=("fp32",)),       # NN with n % 4 != 0
           _case(GENERIC, "f32,NT", (33, 136, 36), mode="ld2", dts=("fp32",)),               # lda % 4 != 0
           _case(GENERIC, "16,NT", (65, 33, 17), bias=True), _case(GENERIC, "16,NN", (65, 33, 17), tb=False),
           _case(GENERIC, "16,NT", (33, 100, 72)), _case(GENERIC, "16,NN", (33, 100, 72), tb=False, bias=True),
           _case(GENERIC, "16,NT", (5, 8, 12), bias=True), _case(GENERIC, "16,NN", (5, 8, 12), tb=False),
           _case(GENERIC, "16,NT", (33, 64, 72), mode="ld2"), _case(GENERIC, "16,NN", (33, 64, 72), tb=False, mode="ld2"),
           _case(GENERIC, "16,NT", (33, 64, 72), mode="offa"), _case(GENERIC, "16,NT", (1, 1, 1)),
           _case(GENERIC, "16,NT", (130, 136, 72), bias=True, mode="bias2")]
    return cs


def _f32out_cases():
    cs = []
    f = lambda kernel, inst, mnk, mode="pad": _case(kernel, inst, mnk, api="f32out", mode=mode)  # noqa: E731
    # gemm_splitk_lds_nt<MC, partial> writing C directly; M <= 16 and M > 2048 never come here from pli_gemm
    for m, n, k in ((5, 32, 64), (17, 160, 128), (33, 32, 192), (64, 288, 256), (65, 32, 64), (96, 160, 320),
                    (97, 32, 128), (130, 160, 192), (256, 32, 64), (2049, 32, 64)):
        cs.append(f(SPLIT_L, f"MC{_mc(m)},f32", (m, n, k)))
    cs += [f(F32OUT_GENERIC, "", (33, 64, 72)), f(F32OUT_GENERIC, "", (33, 40, 64)), f(F32OUT_GENERIC, "", (1, 1, 1)),
           f(F32OUT_GENERIC, "", (33, 64, 64), "ld2"), f(F32OUT_GENERIC, "", (33, 64, 64), "offc")]
    return cs


def _gemv_cases():
    cs = []
    for dts in (B16, ("fp32",)):
        epc = 4 if dts[0] == "fp32" else 8
        for v, (rows, cpl, ntl, wpb) in GEMV_VARIANTS.items():
            kx = 64 * cpl * epc              # one exact pass of the chunk loop
            form = "R{},CPL{},{},WPB{},".format(rows, cpl, "nt" if ntl else "plain", wpb)
            # M: a last wave and a last workgroup that are partly filled
            cs += [_case(GEMV_VEC, form + "exact", (rows * wpb + 1, 0, kx), variant=v, dts=dts, api="gemv"),
                   _case(GEMV_VEC, form + "clamped", (max(1, rows * wpb - 1), 0, kx + 8), variant=v, dts=dts, api="gemv"),
                   _case(GEMV_VEC, form + "clamped", (1, 0, kx - 8), variant=v, dts=dts, api="gemv")]
    # the default rule: <= 128 chunks variant 16; M >= 16384 with <= 256 chunks variant 9; else 8
    cs += [_case(GEMV_VEC, "R2,CPL2,nt,WPB4,exact", (5, 0, 1024), api="gemv"),
           _case(GEMV_VEC, "R1,CPL8,nt,WPB2,clamped", (5, 0, 1032), api="gemv"),
           _case(GEMV_VEC, "R1,CPL4,nt,WPB2,exact", (16384, 0, 2048), api="gemv"),
           _case(GEMV_VEC, "R1,CPL8,nt,WPB2,clamped", (16383, 0, 2048), api="gemv"),
           _case(GEMV_VEC, "R2,CPL2,nt,WPB4,exact", (5, 0, 512), dts=("fp32",), api="gemv"),
           _case(GEMV_SCALAR, "", (5, 0, 13), dts=B16 + ("fp32",), api="gemv"), _case(GEMV_SCALAR, "", (1, 0, 1), api="gemv"),
           _case(GEMV_SCALAR, "", (6, 0, 130), dts=("fp32",), api="gemv"),
           _case(GEMV_SCALAR, "", (9, 0, 136), mode="ld2", dts=B16 + ("fp32",), api="gemv"),
           _case(GEMV_SCALAR, "", (9, 0, 136), mode="offa", dts=B16 + ("fp32",), api="gemv")]
    return cs


def _with_large(cases):
    """the "large" kind once per route (kernel and api), at the route's last default case in the padded mode"""
    out = list(cases)
    for key in dict.fromkeys((c.api, c.kernel) for c in cases):
        out.append([c for c in cases if (c.api, c.kernel) == key and c.mode == "pad"][-1]._replace(kind="large"))
    return out


GEMM_CASES = _with_large(_gemm_cases())
F32OUT_CASES = _with_large(_f32out_cases())
GEMV_CASES = _with_large(_gemv_cases())
ALL_CASES = GEMM_CASES + F32OUT_CASES + GEMV_CASES


def device_cases(cus: int):
    """The cases whose instance depends on the CU count: the persistent gemm_w5 walk at the smallest grid of
    256 x 256 tiles above cus / 8 * 8 (16 column tiles; K 128 and 192 walk, K 64 is the one-tile form), pli_gemm
    and pli_gemm_f32out, and gemm_f32_mfma's four-wave form at the smallest grid of >= 2 * cus tiles of 128^2."""
    cs = []
    g = cus // 8 * 8
    m, n = 256 * max(g // 16 + 1, 8), 256 * 16      # (and at least the 128 tiles of the default route)
    assert cdiv(m, 256) * cdiv(n, 256) > g and cdiv(m, 256) * cdiv(n, 256) >= 128
    for k, form in ((128, "persistent"), (192, "persistent"), (64, "tile")):
        for tb in (True, False):
            cs.append(_case(W5, "w5 " + form, (m, n, k), tb=tb, bias=True, dts=("bf16",) if tb else ("fp16",)))
    cs += [_case(W5, "w5 f32 persistent", (m, n, 128), api="f32out"),
           _case(W5, "w5 f32 tile", (m, n, 64), api="f32out", dts=("fp16",)),
           _case(W5, "w5 f32 tile", (m + 1, n, 128), api="f32out", dts=("bf16",))]
    fm, fn = 128 * cdiv(2 * cus, 32), 128 * 32
    for k, tb, bias in ((4, True, False), (36, False, True), (36, True, True), (4, False, False)):
        cs.append(_case(F32MFMA, "f32 NW4", (fm, fn, k), tb=tb, bias=bias, dts=("fp32",)))
    return cs


def case_id(c: GemmCase) -> str:
    shape = f"m{c.m}k{c.k}" if c.api == "gemv" else f"m{c.m}n{c.n}k{c.k}-{_tb(c.trans_b)}"
    return "{}{}{}-{}{}{}{}{}{}".format("" if c.api == "gemm" else c.api + "-", c.kernel.split("+")[0],
                                        "-" + c.inst.replace(" ", "_") if c.inst else "", shape, "-bias" if c.bias else "",
                                        "" if c.variant is None else f"-v{c.variant}", "" if c.ws == "auto" else f"-ws{c.ws}",
                                        "" if c.kind == "default" else "-" + c.kind, "" if c.mode == "pad" else "-" + c.mode)


def leading_dims(c: GemmCase, padded: bool = True):
    """(lda, ldb, ldc) as the call passes them (gemv: (-, ldw, -)); pli_hip.gemm passes the contiguous stride for an
    operand of one row"""
    k, n = c.k, c.n
    if c.api == "gemv":
        return 0, (k + (2 if c.mode == "ld2" else 8) if padded else k), 0
    cols_b = k if c.trans_b else n
    rows_b = n if c.trans_b else k
    if not padded:
        return k, cols_b, n
    lda = k + (2 if c.mode == "ld2" else 8)
    ldb = cols_b + 16
    if c.ws == "auto" and c.api == "gemm":                     # through the wrapper
        lda, ldb = (lda if c.m > 1 else k), (ldb if rows_b > 1 else cols_b)
    return lda, ldb, (n if c.api == "f32out" else n + 8)


def case_ws_bytes(c: GemmCase, dt: str) -> int:
    """the workspace bytes the case's call passes (with a non-null pointer iff > 0)"""
    if c.ws == "auto":
        return workspace_size(c.m, c.n, c.k, c.trans_b, dt) if c.variant in SPLIT_VARIANTS else 0
    return 16 if c.ws == "min" else int(c.ws)


def case_route(c: GemmCase, dt: str, padded: bool = True, cus: int = 256, workspace=None) -> Route:
    lda, ldb, _ = lds = leading_dims(c, padded)
    aligned = not (padded and c.mode in ("offa", "offc"))
    if c.api == "gemv":
        return gemv_route(c.m, c.k, dt, ldb, aligned, c.variant)
    if c.api == "f32out":
        return f32out_route(c.m, c.n, c.k, dt, (lda, ldb), aligned, cus)
    ws = case_ws_bytes(c, dt) if workspace is None else workspace
    return gemm_route(c.m, c.n, c.k, dt, c.trans_b, c.bias, c.variant, ws, lds, aligned,
                      not (padded and c.mode == "bias2"), cus)


def _contig(cases):
    """one default-kind case per (api, kernel, inst, trans_b, bias, dts) that stays on its route with ld == k"""
    pick = {}
    for c in cases:
        if c.kind == "default" and c.mode in ("pad", "bias8"):
            pick.setdefault((c.api, c.kernel, c.inst.replace("clamped", "").replace("exact", ""), c.trans_b, c.bias, c.dts), c)
    return list(pick.values())


CONTIG_CASES = _contig(ALL_CASES)


# -------------------------------------- the instances the launchers can make
def template_key(c: GemmCase, dt: str):
    """the template instance a case launches, as (kernel, parameters...) without run-time parameters (ks, group_m)"""
    i = c.inst
    if c.api == "gemv":
        return (c.kernel, dt, i)
    if c.api == "f32out":
        return ("f32out:" + c.kernel, dt, i)
    if c.kernel in (SKINNY, GEMV_VEC):
        return (c.kernel, dt, i)
    if c.kernel == GENERIC:
        return (c.kernel, dt, i)
    if c.kernel == F32MFMA:
        return (c.kernel, dt, i, c.trans_b)
    if c.kernel.startswith("gemm_splitk"):
        mc, ks, load, nb, store = i.split(",")
        return (c.kernel, dt, mc, load, nb, store) + ((c.bias,) if ks == "ks1" else ())   # (the reduce: covered_instances)
    if c.kernel == G256:
        return (c.kernel, dt, i.split(" g")[0] + (" prio" if i.endswith("prio") else ""), c.trans_b, c.bias)
    if c.kernel in (SMALLM, MIDM):
        return (c.kernel, dt, i, c.bias)
    return (c.kernel, dt, i, c.trans_b, c.bias)      # gemm_mfma, gemm_w5, gemm_w4v


def launchable_instances():
    """every template instance launch_skinny / _smallm / _midm / _splitk / _mfma / _256 / _generic, launch_gemm_w5 /
    _w4v / _f32_mfma, pli_gemm_f32out and gemv's launch can instantiate, as template_key writes them"""
    s = set()
    tf = (True, False)
    for dt in B16:
        s |= {(SKINNY, dt, f"NB{nb},CPL{cpl}") for nb in (1, 2, 4) for cpl in (2, 4, 8, 12, 16)}
        s |= {(SKINNY, dt, f"NB{nb},CPL8") for nb in (8, 16)}
        s |= {(SMALLM, dt, f"NBG{g}", b) for g in (1, 2, 4, 8) for b in tf}
        s |= {(MIDM, dt, f"MC{mc}", b) for mc in (1, 2, 3, 4) for b in tf}
        for mc in (1, 2, 3, 4):
            for kern, load, nb in ((SPLIT_D, "direct", "NB2"), (SPLIT_L, "lds", "NB2"), (SPLIT_L, "lds", "NB3")):
                s |= {(kern, dt, f"MC{mc}", load, nb, "direct-store", b) for b in tf}
                s.add((kern + "+" + REDUCE, dt, f"MC{mc}", load, nb, "partial"))
            s.add(("f32out:" + SPLIT_L, dt, f"MC{mc},f32"))
        s |= {(REDUCE, dt, b) for b in tf}
        s |= {(MFMA, dt, "", tb, b) for tb in tf for b in tf}
        s |= {(G256, dt, i, tb, b) for i in ("256", "256 prio", "256p SCHED0", "256p SCHED1", "256p SCHED3",
                                             "256p SCHED5", "256p SCHED7") for tb in tf for b in tf}
        s |= {(W5, dt, i, tb, b) for i in ("w5 tile", "w5 persistent") for tb in tf for b in tf}
        s |= {(W4V, dt, "", tb, b) for tb in tf for b in tf}
        s |= {("f32out:" + W5, dt, i) for i in ("w5 f32 tile", "w5 f32 persistent")}
        s.add(("f32out:" + F32OUT_GENERIC, dt, ""))
    for dt in B16 + ("fp32",):
        s |= {(GENERIC, dt, ("f32," if dt == "fp32" else "16,") + t) for t in ("NT", "NN")}
        s |= {(GEMV_VEC, dt, _gemv_inst(v, 0, dt).replace("exact", e)) for v in GEMV_VARIANTS for e in ("exact", "clamped")}
        s.add((GEMV_SCALAR, dt, ""))
    s |= {(F32MFMA, "fp32", f"f32 NW{nw}", tb) for nw in (4, 8) for tb in tf}
    return s


def covered_instances(cus: int = 256):
    out = set()
    for c in ALL_CASES + device_cases(cus):
        for dt in c.dts:
            key = template_key(c, dt)
            if c.kernel == W5 and "persistent1" in c.inst:      # the persistent instance, one tile per workgroup
                key = key[:2] + (c.inst.replace("persistent1", "persistent"),) + key[3:]
            out.add(key)
            if c.kernel.endswith("+" + REDUCE):
                out.add((REDUCE, dt, c.bias))
    return out


# ----------------------------------------------------------------- operands
def case_seed(c: GemmCase, dt: str) -> int:
    return (9000 + 3 * c.m + 7 * c.n + 11 * c.k + {"fp32": 0, "bf16": 100, "fp16": 600}[dt] + (50 if c.kind == "large" else 0)
            + (1000 if c.api != "gemm" else 0) + (13 if not c.trans_b else 0))


Operands = namedtuple("Operands", "a b bias")


def operands(c: GemmCase, dt: str) -> Operands:
    """float32 arrays holding values of dt: a [m, k], b [n, k] (NT) or [k, n] (NN), bias [n] or None.  gemv: a is
    W [m, k], b is x as [1, k]"""
    seed = case_seed(c, dt)
    sa, sb = (1.0, 1.0) if c.kind == "large" else (0.5, max(c.k, 1) ** -0.5)
    n = 1 if c.api == "gemv" else c.n
    a = round_to_dtype(seeded_normal((c.m, c.k), seed) * np.float32(sa), dt)
    b = round_to_dtype(seeded_normal((n, c.k) if c.trans_b else (c.k, n), seed + 1) * np.float32(sb), dt)
    bias = round_to_dtype(seeded_normal((n,), seed + 2), dt) if c.bias else None
    return Operands(a, b, bias)


# ------------------------------------------------------ reference and bounds
Reference = namedtuple("Reference", "c bracket k")


def reference(op: Operands, trans_b: bool = True) -> Reference:
    """float64: C = A B^T (or A B) + bias, and the bracket (K + 2) * 2^-23 * (|A| |B|^T + |bias|) of bound (b)"""
    a = np.asarray(op.a, np.float64)
    b = np.asarray(op.b, np.float64)
    bt = b.T if trans_b else b
    K = a.shape[1]
    c, mag = a @ bt, np.abs(a) @ np.abs(bt)
    if op.bias is not None:
        c, mag = c + np.asarray(op.bias, np.float64), mag + np.abs(np.asarray(op.bias, np.float64))
    return Reference(c, (K + 2) * 2.0 ** -23 * mag, K)


@functools.lru_cache(maxsize=8)
def case_reference(c: GemmCase, dt: str):
    """(operands, reference) of a case, computed once and shared (read-only) by the tests that need it"""
    op = operands(c, dt)
    ref = reference(op, c.trans_b)
    for x in tuple(op) + (ref.c, ref.bracket):
        if x is not None:
            x.setflags(write=False)
    return op, ref


def out_dtype(c: GemmCase, dt: str) -> str:
    return "fp32" if c.api == "f32out" else dt


def bound_a(c: GemmCase, ref: Reference, dt: str) -> np.ndarray:
    if c.kernel == F32MFMA:
        return np.full(ref.c.shape, 4e-6 * ref.k + 1e-5)
    return TOL_A[out_dtype(c, dt)] * (np.abs(ref.c) + 1)


def bound_b(c: GemmCase, ref: Reference, dt: str) -> np.ndarray:
    o = out_dtype(c, dt)
    return NORM_SLACK * ROUND[o] * np.abs(ref.c) + ref.bracket + FLOOR[o]


def ratios(got, c: GemmCase, ref: Reference, dt: str):
    """(max |err| / bound (a), max |err| / bound (b)) over the elements; inf for a non-finite output"""
    got = np.asarray(got, np.float64).reshape(ref.c.shape)
    if got.size == 0:
        return 0.0, 0.0
    if not np.isfinite(got).all():
        return float("inf"), float("inf")
    err = np.abs(got - ref.c)
    return float((err / bound_a(c, ref, dt)).max()), float((err / bound_b(c, ref, dt)).max())


def worst(got, c: GemmCase, ref: Reference, dt: str) -> str:
    got = np.asarray(got, np.float64).reshape(ref.c.shape)
    err = np.abs(got - ref.c)
    bb = bound_b(c, ref, dt)
    i = np.unravel_index(np.nanargmax(err / bb), err.shape)
    return ("element {}: got {:.9g} ref {:.9g} err {:.3e}; rounding term {:.3e}, bracket {:.3e}, (a) {:.3e}; {} elements "
            "over (b)").format(i, got[i], ref.c[i], err[i], NORM_SLACK * ROUND[out_dtype(c, dt)] * abs(ref.c[i]),
                               ref.bracket[i], bound_a(c, ref, dt)[i], int((err > bb).sum()))


# ---------------------------------------------------------------- emulation
def split_ks(c: GemmCase) -> int:
    return int(c.inst.split("ks")[1].split(",")[0]) if "ks" in c.inst else 1


def emulate_f32(op: Operands, trans_b: bool = True, ks: int = 1, rows=None) -> np.ndarray:
    """the semantics on the CPU before the output rounding, float32: fp32 products and sums of the rounded inputs
    (ks > 1: the split route's ks fp32 partials over K / ks each, summed in plane order), the bias added in fp32"""
    a = torch.from_numpy(np.array(op.a if rows is None else op.a[rows], dtype=np.float32))
    b = torch.from_numpy(np.array(op.b, dtype=np.float32))
    bt = b.t() if trans_b else b
    kslice = a.shape[1] // ks
    acc = torch.zeros(a.shape[0], bt.shape[1])
    for s in range(ks):
        sl = slice(s * kslice, (s + 1) * kslice if s + 1 < ks else None)
        acc = acc + a[:, sl] @ bt[sl]
    if op.bias is not None:
        acc = acc + torch.from_numpy(np.array(op.bias, dtype=np.float32))
    return acc.numpy()


def emulate(op: Operands, out_dt: str, trans_b: bool = True, ks: int = 1, rows=None) -> np.ndarray:
    """emulate_f32 with the one rounding to the output type, as float64"""
    return f64(torch.from_numpy(emulate_f32(op, trans_b, ks, rows)).to(TDT3[out_dt]))


def chain_ratio(c32, ref: Reference, rows=None) -> float:
    """max over elements of |c32 - ref| / the bracket of (b) (0 / 0 counts as 0)"""
    rc, rb = (ref.c, ref.bracket) if rows is None else (ref.c[rows], ref.bracket[rows])
    err = np.abs(np.asarray(c32, np.float64) - rc)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / rb)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------ device inputs
def _padded(a: np.ndarray, ld: int, dt: str, device, offset: int = 0) -> torch.Tensor:
    """[r, k] values as a view with row stride ld inside a NaN-filled buffer of r + 3 rows, `offset` elements in"""
    r, k = a.shape
    buf = torch.full(((r + 3) * ld + offset,), float("nan"), dtype=TDT3[dt], device=device)
    view = buf.as_strided((r, k), (ld, 1), offset)
    view.copy_(torch.from_numpy(np.array(a, dtype=np.float32)).to(TDT3[dt]))
    return view


def _dev(a: np.ndarray, dt: str, device) -> torch.Tensor:
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(TDT3[dt]).to(device)


def device_operands(c: GemmCase, op: Operands, dt: str, device, padded: bool = True):
    """a, b, bias on the device (see the module docstring; strides independent of the one-row rule of
    leading_dims) and the Guarded output: pli_gemm [m + 3, n] with row stride n + 8 (n without padding);
    pli_gemm_f32out a flat m * n (+ 4, the view one element in, for "offc"); pli_gemv [m + 3]"""
    k = c.k
    epc = 4 if dt == "fp32" else 8
    if padded:
        lda = k + (2 if c.mode == "ld2" else 8)
        if c.api == "gemv":
            a = _padded(op.a, lda, dt, device)
            b = _padded(op.b, k + epc, dt, device, epc + (1 if c.mode == "offa" else 0))[0]
        else:
            a = _padded(op.a, lda, dt, device, 1 if c.mode == "offa" else 0)
            b = _padded(op.b, op.b.shape[1] + 16, dt, device)
    else:
        a, b = _dev(op.a, dt, device), _dev(op.b, dt, device)
        if c.api == "gemv":
            b = b[0]
    bias = None
    if op.bias is not None:
        off = {"bias2": 1, "bias8": 4}.get(c.mode, 8) if padded else 0
        buf = torch.full((c.n + 16,), float("nan"), dtype=TDT3[dt], device=device)
        bias = buf[off:off + c.n]
        bias.copy_(_dev(op.bias, dt, device))
    if c.api == "gemv":
        out = Guarded((c.m + 3,), dt, device)
    elif c.api == "f32out":
        out = Guarded((c.m * c.n + 4,), "fp32", device)
    else:
        out = Guarded((c.m + 3, c.n), dt, device, strides=((c.n + 8) if padded else c.n, 1))
    return a, b, bias, out


def addressed(c: GemmCase, padded: bool = True):
    """view -> the part of the Guarded output the call may write"""
    if c.api == "f32out":
        off = 1 if padded and c.mode == "offc" else 0
        return lambda v: v[off:off + c.m * c.n]
    return lambda v: v[:c.m]


# ------------------------------------------------------- import-time checks
for _family, _pad in ((ALL_CASES + device_cases(256), True), (CONTIG_CASES, False)):
    for _c in _family:
        for _dt in _c.dts:
            _r = case_route(_c, _dt, _pad)
            assert (_r.kernel, _r.inst) == (_c.kernel, _c.inst), (case_id(_c), _dt, _pad, _r)
assert len({case_id(c) for c in ALL_CASES}) == len(ALL_CASES)
assert all(c.k <= 8200 and (c.m * max(c.n, 1) <= 1 << 20 or c.k <= 192) for c in ALL_CASES + device_cases(256))
