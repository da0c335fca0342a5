"""Route replay, case list, operands, float64 reference and the two per-element bounds shared by the fp8-activation
(W8A8) tests: tests/test_gpu_fp8a.py on the GPU, tests/test_fp8a_emulation_cpu.py, tests/test_fp8a_plan.py and
tests/test_fp8a_capi.py on the CPU.

Route replay: `route` restates fp8a_route of csrc/fp8a_plan.h; the constants it uses are read back from the header
when this module is imported, every case is asserted against the replay, and the kernel names the cases expect are
asserted against the names the launchers of csrc/gemm_fp8.hip report (its launch_status strings), both ways: no case
names a kernel that cannot be launched, and no GEMM kernel is without a case.  gemm_fp8_mx has one template shape
(128 x 128, two stages); its BIAS instance is selected by the bias pointer, and both are in the list.

Operands: x [m, k] = N(0,1) * 0.5 and w [n, k] = N(0,1) * k^-0.5 rounded to the storage type, each quantised per
row by the rule of pli_hip.quantize_weight_fp8 (on the CPU); bias [n] = N(0,1).  An operand whose scale pointer a
case leaves NULL holds the codes of 4 * its values at scale one.  The oracle is float64 over the dequantised operands
decode(code) * scale.

Bounds, per element, both asserted:
(a) the project's |err| <= LIN_TOL * (|ref| + 1), bf16 1e-2, fp16 4e-3;
(b) tests/gemm_cases.py's derived form with its constant: NORM_SLACK * u * |ref| + (K + 2) * 2^-23 * mag +
    MIN_NORMAL, mag = (x_scale |X8|) (w_scale |W8|)^T + |bias| in float64.  The K term is twice the first-order
    error of a length-K fp32 sum in any order (the products are exact); the + 2 covers the three fp32 roundings
    after the sum (x_scale * w_scale, the product with the sum, the bias add: 1.5 * 2^-23 to first order).
"""
from __future__ import annotations

import functools
import os
import re
from collections import namedtuple

import numpy as np
import torch

from conftest import PKG
from decode_step_cases import HALF_ULP, LIN_TOL, MIN_NORMAL, NORM_SLACK, TDT
from oracle.numerics import round_to_dtype, seeded_normal

MX, GENERIC, QUANT = "gemm_fp8_mx", "gemm_fp8_generic", "quant_rows_fp8"
EMPTY_R, MX_R, GENERIC_R = 0, 1, 2
DTYPES = ("bf16", "fp16")
# every e4m3fn code's value (exact in fp32); NaN at 0x7F / 0xFF
DECODE = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)

_PLAN = open(os.path.join(PKG, "csrc", "fp8a_plan.h")).read()
_SRC = open(os.path.join(PKG, "csrc", "gemm_fp8.hip")).read()


def _const(name: str) -> int:
    m = re.search(r"constexpr int " + name + r" = (\d+);", _PLAN)
    assert m, f"{name} is not a plain constant of fp8a_plan.h"
    return int(m.group(1))


TM, TN, KSTEP, STAGES = _const("kFp8aTM"), _const("kFp8aTN"), _const("kFp8aKStep"), _const("kFp8aStages")
MIN_M, STORE_N, GROUP_M = _const("kFp8aMinM"), _const("kFp8aStoreN"), _const("kFp8aGroupM")
QUANT_THREADS, QUANT_HELD = _const("kFp8aQuantThreads"), _const("kFp8aQuantHeld")
QUANT_REG_K = 8 * QUANT_THREADS * QUANT_HELD


def route(m, n, k, ldx8=None, ldw=None, ldc=None, x8=4096, w8=8192, c=12288) -> int:
    """fp8a_route: addresses as integers, leading dimensions default to the widths"""
    ldx8, ldw, ldc = (k if ldx8 is None else ldx8), (k if ldw is None else ldw), (n if ldc is None else ldc)
    if m <= 0 or n <= 0 or k <= 0:
        return EMPTY_R
    if (m >= MIN_M and k % KSTEP == 0 and (x8 | w8) % 16 == 0 and ldx8 % 16 == 0 and ldw % 16 == 0 and
            n % STORE_N == 0 and ldc % STORE_N == 0 and c % 8 == 0):
        return MX_R
    return GENERIC_R


def kernel_of(m, n, k, **kw) -> str:
    """what pli_last_route reports for a non-empty call (k == 0 runs the generic kernel: bias or 0)"""
    return MX if route(m, n, k, **kw) == MX_R else GENERIC


# scales: "both", "none" (both pointers NULL), "x" / "w" (only that one given)
# mode: "" contiguous; "pad": ldx8 = k + 16, ldw = k + 48 (the codes a column slice of a wider matrix of NaN codes),
#       ldc = n + 8, guards around C; "off1": the w8 view starts one byte into its buffer (generic)
Case = namedtuple("Case", "m n k kernel bias scales mode")


def _c(m, n, k, kernel=MX, bias=False, scales="both", mode=""):
    return Case(m, n, k, kernel, bias, scales, mode)


S = STAGES
GEMM_CASES = [
    # m edges x n edges x ring wraps (k = 128 one step, 256 = S steps, 384 = S + 1, 4096 = 32 steps)
    _c(MIN_M, STORE_N, KSTEP),
    _c(MIN_M, TN, KSTEP * S),
    _c(MIN_M, TN + STORE_N, 4096),
    _c(TM - 1, TN - STORE_N, KSTEP),
    _c(TM - 1, TN + STORE_N, KSTEP * (S + 1)),
    _c(TM - 1, TN, 4096),
    _c(TM, TN, KSTEP),
    _c(TM, TN, KSTEP * S),
    _c(TM, STORE_N, KSTEP * (S + 1)),
    _c(TM, TN - STORE_N, KSTEP * S),
    _c(TM + 1, TN, KSTEP),
    _c(TM + 1, TN + STORE_N, KSTEP * S),
    _c(TM + 1, TN - STORE_N, 4096),
    _c(2 * TM + 3, TN + STORE_N, KSTEP * (S + 1)),
    _c(2 * TM + 3, TN, KSTEP),
    _c(2 * TM + 3, STORE_N, KSTEP * S),
    _c(2 * TM + 3, 3 * TN + STORE_N, KSTEP * S),          # several n tiles: m fastest inside a band
    _c((GROUP_M + 1) * TM + 5, TN + STORE_N, KSTEP),      # more m-tiles than a band: a full band and a short one
    # the BIAS instance, NULL scales, padded leading dimensions with NaN codes in the padding
    _c(TM + 1, TN + STORE_N, KSTEP * (S + 1), bias=True, mode="pad"),
    _c(MIN_M, TN - STORE_N, KSTEP * S, bias=True, scales="none"),
    _c(2 * TM + 3, TN, KSTEP, scales="none", mode="pad"),
    _c(TM - 1, TN, KSTEP * S, scales="x", mode="pad"),
    _c(TM, TN + STORE_N, KSTEP, bias=True, scales="w"),
    # generic: k = 40 with n = 24, an unaligned view, n no multiple of 4, fewer rows than the threshold
    _c(MIN_M, 24, 40, GENERIC, bias=True),
    _c(MIN_M, 24, 40, GENERIC, scales="none", mode="pad"),
    _c(MIN_M, TN, KSTEP, GENERIC, mode="off1"),
    _c(MIN_M + 2, 6, KSTEP, GENERIC, bias=True),
    _c(MIN_M - 1, TN, KSTEP, GENERIC),
]


def leading_dims(c: Case):
    return (c.k + 16, c.k + 48, c.n + 8) if c.mode == "pad" else (c.k, c.k, c.n)


def case_id(c: Case) -> str:
    return "m{}n{}k{}{}{}{}".format(c.m, c.n, c.k, "b" if c.bias else "", "" if c.scales == "both" else "-s" + c.scales,
                                    "-" + c.mode if c.mode else "")


def launchable_kernels() -> set:
    """the names the launchers of gemm_fp8.hip can report"""
    return set(re.findall(r'launch_status\("([a-z0-9_]+)"\)', _SRC))


def _check_cases():
    names = launchable_kernels()
    assert names == {MX, GENERIC, QUANT}, names
    assert len({case_id(c) for c in GEMM_CASES}) == len(GEMM_CASES)
    for c in GEMM_CASES:
        ldx8, ldw, ldc = leading_dims(c)
        got = kernel_of(c.m, c.n, c.k, ldx8=ldx8, ldw=ldw, ldc=ldc, w8=8192 + (1 if c.mode == "off1" else 0))
        assert got == c.kernel and got in names, (c, got)
    assert {c.kernel for c in GEMM_CASES} == names - {QUANT}
    for kernel in (MX, GENERIC):  # each GEMM kernel with and without a bias (the BIAS template instance)
        assert {c.bias for c in GEMM_CASES if c.kernel == kernel} == {False, True}


_check_cases()

# quantiser: m x k; the last two k are the register-resident limit and the first vector-class k past it
QUANT_MS = (1, 3, 17)
QUANT_KS = (1, 16, 130, 2048, QUANT_REG_K, QUANT_REG_K + 8)


# ---------------------------------------------------------------- operands
def quantize_rows_np(a32: np.ndarray, unit: bool = False):
    """(codes uint8, scale fp32) of a finite fp32 array by quantize_weight_fp8's rule (torch on the CPU); unit: the
    codes of 4 * a32 at scale 1 and no scale (None)"""
    import pli_hip
    a = torch.from_numpy(np.ascontiguousarray(a32, dtype=np.float32))
    if unit:
        codes, _ = pli_hip.quantize_weight_fp8(a * 4.0, scale=torch.ones(a.shape[0]))
        return codes.view(torch.uint8).numpy().copy(), None
    codes, scale = pli_hip.quantize_weight_fp8(a)
    return codes.view(torch.uint8).numpy().copy(), scale.numpy().copy()


Operands = namedtuple("Operands", "x8 xs w8 ws bias")
Reference = namedtuple("Reference", "c bracket k")


def case_seed(c: Case, dt: str) -> int:
    return 31000 + 7 * c.m + 13 * c.n + c.k + (500 if dt == "fp16" else 0) + (len(c.mode) + len(c.scales)) * 1000


def operands(c: Case, dt: str) -> Operands:
    seed = case_seed(c, dt)
    x = round_to_dtype(seeded_normal((c.m, c.k), seed) * np.float32(0.5), dt)
    w = round_to_dtype(seeded_normal((c.n, c.k), seed + 1) * np.float32(c.k ** -0.5), dt)
    # an operand without a scale (NULL: ones) holds the codes of 4 * its values, so the results stay in fp16's range
    x8, xs = quantize_rows_np(x, unit=c.scales in ("none", "w"))
    w8, ws = quantize_rows_np(w, unit=c.scales in ("none", "x"))
    bias = round_to_dtype(seeded_normal((c.n,), seed + 2), dt) if c.bias else None
    return Operands(x8, xs, w8, ws, bias)


def reference(op: Operands) -> Reference:
    """float64 over the dequantised operands, and the bracket (K + 2) * 2^-23 * mag of bound (b)"""
    xd = DECODE[op.x8] * (1.0 if op.xs is None else op.xs.astype(np.float64)[:, None])
    wd = DECODE[op.w8] * (1.0 if op.ws is None else op.ws.astype(np.float64)[:, None])
    K = xd.shape[1]
    c, mag = xd @ wd.T, np.abs(xd) @ np.abs(wd).T
    if op.bias is not None:
        c, mag = c + op.bias.astype(np.float64), mag + np.abs(op.bias.astype(np.float64))
    return Reference(c, (K + 2) * 2.0 ** -23 * mag, K)


@functools.lru_cache(maxsize=None)
def case_reference(c: Case, dt: str):
    """(operands, reference) of a case, computed once and shared read-only by the tests that need it"""
    op = operands(c, dt)
    ref = reference(op)
    for a in tuple(op) + (ref.c, ref.bracket):
        if a is not None:
            a.setflags(write=False)
    return op, ref


def bound_a(ref: Reference, dt: str) -> np.ndarray:
    return LIN_TOL[dt] * (np.abs(ref.c) + 1)


def bound_b(ref: Reference, dt: str) -> np.ndarray:
    return NORM_SLACK * HALF_ULP[dt] * np.abs(ref.c) + ref.bracket + MIN_NORMAL[dt]


def ratios(got, ref: Reference, dt: str):
    """(max |err| / (a), max |err| / (b)); inf for a non-finite output"""
    got = np.asarray(got, np.float64).reshape(ref.c.shape)
    if not np.isfinite(got).all():
        return float("inf"), float("inf")
    err = np.abs(got - ref.c)
    return float((err / bound_a(ref, dt)).max()), float((err / bound_b(ref, dt)).max())


def emulate_f32(op: Operands) -> np.ndarray:
    """the semantics before the output rounding, in float32: fp32 sum of the exact products, sum * (xs * ws), + bias"""
    acc = torch.from_numpy(DECODE[op.x8].astype(np.float32)) @ torch.from_numpy(DECODE[op.w8].astype(np.float32)).t()
    xs = torch.ones(op.x8.shape[0]) if op.xs is None else torch.from_numpy(np.array(op.xs))
    ws = torch.ones(op.w8.shape[0]) if op.ws is None else torch.from_numpy(np.array(op.ws))
    v = acc * (xs[:, None] * ws[None, :])
    if op.bias is not None:
        v = v + torch.from_numpy(np.array(op.bias, dtype=np.float32))
    return v.numpy()


def emulate(op: Operands, dt: str) -> np.ndarray:
    return torch.from_numpy(emulate_f32(op)).to(TDT[dt]).double().numpy()


# ---------------------------------------------------------------- exact patterns (lane map)
def const_rows_codes(k: int):
    """x8 row r = code r in every column, w8 row j = code j: all 256 x 256 code pairs"""
    a = np.repeat(np.arange(256, dtype=np.uint8)[:, None], k, axis=1)
    return a, a.copy()


def small_int_code(v: np.ndarray) -> np.ndarray:
    """e4m3fn codes of the integers -8 .. 8 (exact)"""
    return torch.from_numpy(v.astype(np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def asymmetric_codes(m: int, n: int, k: int):
    """distinct small-integer patterns for the two operands, depending on (row, k) and (col, k): integer sums below
    2^24, so every partial sum is exact in any order, and a row <-> column swap or a k permutation applied to one
    operand only changes the result"""
    r, j, i = np.arange(m)[:, None], np.arange(n)[:, None], np.arange(k)[None, :]
    xv = ((3 * r + 5 * i + (r * i) // 7) % 9) - 4
    wv = ((7 * j + 2 * i + (j * i) // 5 + 1) % 13) - 6
    return small_int_code(xv), small_int_code(wv), xv.astype(np.float64), wv.astype(np.float64)
