"""Inputs, guarded outputs, float64 references and the case lists shared by the
decode-step tests (tests/test_gpu_decode_step.py on the GPU,
tests/test_decode_step_emulation_cpu.py on the CPU).

Operands are drawn with oracle.numerics.seeded_normal and rounded to the
storage type: activations N(0,1) (times an optional power-of-two scale), norm
weight 1 + 0.1 N(0,1), projection weights N(0,1) * k**-0.5.  On request the
inputs are views of wider buffers with NaN around them, and every output is a
view inside a buffer pre-filled with a sentinel that both 16-bit types hold
exactly (-1024.0), with guard rows before and after it: `assert_untouched`
checks, bit for bit, that nothing outside the addressed elements was written.

The reference of the fused calls is float64 on the stored h = a (+ residual)
(h itself is held bitwise to the torch CPU add): oracle.linear.rms_norm,
rms_linear, rms_swiglu.  `emulate_fused` restates the kernel's documented
semantics on the CPU (h rounded, fp32 statistics, y rounded to the storage
type, fp32 dot, SwiGLU in fp32, one output rounding); the CPU test holds it to
half the GPU bound over the same case list.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np
import torch

from oracle import linear as olin
from oracle.numerics import round_to_dtype, seeded_normal

TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
DTYPES = ("bf16", "fp16")
# the project's linear bound (test_gpu_fp8w.py, test_gpu_swiglu.py): |err| <= LIN_TOL * (|ref| + 1) per element
LIN_TOL = {"bf16": 1e-2, "fp16": 4e-3}
# exact rounding of the storage type: half an ulp, relative; and the smallest normal (absolute floor)
HALF_ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
MIN_NORMAL = {"bf16": 2.0 ** -126, "fp16": 2.0 ** -14}
NORM_SLACK = 1.05  # over half an ulp, for the fp32 statistics
SENTINEL = -1024.0
EPS = 1e-6
S_MAX = 8  # cache capacity of every qkv case


# ---------------------------------------------------------------- operands
def t16(a, dt: str, device="cpu") -> torch.Tensor:
    """float32 values already rounded to `dt` -> a storage-type tensor (exact)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TDT[dt]).to(device)


def f64(t: torch.Tensor) -> np.ndarray:
    return t.detach().double().cpu().numpy()


Operands = namedtuple("Operands", "a residual g w wu")


def operands(k: int, m: int, widths, dt: str, seed: int, residual: bool = True, swiglu: bool = False,
             scale: float = 1.0) -> Operands:
    """float32 arrays rounded to dt: a / residual [m, k], norm weight [k], one [n, k] weight per width (and an up
    weight each with swiglu)"""
    def act(s):
        return round_to_dtype(seeded_normal((m, k), s) * np.float32(scale), dt)

    def wgt(n, s):
        return round_to_dtype(seeded_normal((n, k), s) * np.float32(k ** -0.5), dt)

    g = round_to_dtype(1 + np.float32(0.1) * seeded_normal((k,), seed + 2), dt)
    return Operands(act(seed), act(seed + 1) if residual else None, g,
                    [wgt(n, seed + 3 + i) for i, n in enumerate(widths)],
                    [wgt(n, seed + 13 + i) for i, n in enumerate(widths)] if swiglu else None)


def row_view(a: np.ndarray, dt: str, device, pad: int = 0) -> torch.Tensor:
    """[m, k] rows as a view with row stride k + pad, NaN in the padding"""
    m, k = a.shape
    buf = torch.full((m, k + pad), float("nan"), dtype=TDT[dt], device=device)
    buf[:, :k] = t16(a, dt, device)
    return buf[:, :k]


def weight_view(w: np.ndarray, dt: str, device, padded: bool) -> torch.Tensor:
    """[n, k] weights; padded: columns 8 .. 8 + k of rows 1 .. n of an [n + 2, k + 16] matrix of NaN
    (ldw = k + 16, rows still 16-byte aligned)"""
    if not padded:
        return t16(w, dt, device)
    n, k = w.shape
    buf = torch.full((n + 2, k + 16), float("nan"), dtype=TDT[dt], device=device)
    buf[1:n + 1, 8:8 + k] = t16(w, dt, device)
    return buf[1:n + 1, 8:8 + k]


# ---------------------------------------------------------- guarded outputs
GUARDED_DT = dict(TDT, fp32=torch.float32)  # what a Guarded may hold (the MoE router's weights are fp32)
_BITS = {2: torch.int16, 4: torch.int32}


def sentinel_bits(dt: str) -> int:
    t = torch.tensor([SENTINEL], dtype=GUARDED_DT[dt])
    return int(t.view(_BITS[t.element_size()]).item())


class Guarded:
    """An output of `shape` / `strides` (elements) inside a flat buffer filled with the sentinel, with at least two
    of its largest strides (and 64 elements) of guard before and after; the view stays 16-byte aligned."""

    def __init__(self, shape, dt: str, device, strides=None, guard: int | None = None):
        self.shape = tuple(int(s) for s in shape)
        if strides is None:
            strides, acc = [], 1
            for s in reversed(self.shape):
                strides.insert(0, acc)
                acc *= s
        self.strides = tuple(int(s) for s in strides)
        span = 1 + sum((n - 1) * s for n, s in zip(self.shape, self.strides)) if all(self.shape) else 0
        if guard is None:
            guard = max(64, 2 * max(self.strides))
        self.guard = -(-guard // 8) * 8
        self.dt = dt
        self.buf = torch.full((2 * self.guard + span,), SENTINEL, dtype=GUARDED_DT[dt], device=device)
        self.view = self.buf.as_strided(self.shape, self.strides, self.guard)

    def stray_writes(self, *regions) -> torch.Tensor:
        """flat indices of elements outside `regions` (functions view -> the addressed sub-view) that no longer
        hold the sentinel's bits"""
        mask = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        mv = mask.as_strided(self.shape, self.strides, self.guard)
        for sel in regions:
            sel(mv).fill_(True)
        bad = (self.buf.view(_BITS[self.buf.element_size()]) != sentinel_bits(self.dt)) & ~mask
        return bad.nonzero().flatten()


def assert_untouched(g: Guarded, *regions, what: str = "output") -> None:
    bad = g.stray_writes(*regions)
    assert bad.numel() == 0, (f"{what}: {bad.numel()} elements outside the addressed region were written, first at flat "
                              f"offsets {(bad[:8] - g.guard).tolist()} from the view")


def group_outputs(B: int, S: int, widths, s_max: int, dt: str, device, padded: bool):
    """group 0 q-like [B, S, n0]; the others cache-like [B, s_max, max(widths[1:])] (k and v of one shape, a
    narrower group leaves the upper columns alone).  padded: token stride width + 4 and one spare row per batch,
    so the strides stay multiples of 4 (the small-M kernel's 8-byte stores) but not of the width."""
    outs = []
    for gi, n in enumerate(widths):
        rows = S if gi == 0 else s_max
        wa = n if gi == 0 else max(widths[1:])
        st = wa + (4 if padded else 0)
        sb = (rows + (1 if padded else 0)) * st
        outs.append(Guarded((B, rows, wa), dt, device, strides=(sb, st, 1)))
    return outs


def written_rows(gi: int, S: int, pos: int, s_max: int):
    """(first row, rows written) of group gi's [B, rows, n] output: q rows 0 .. S-1, cache rows pos .. clamped"""
    if gi == 0:
        return 0, S
    return pos, max(0, min(S, s_max - pos))


# ------------------------------------------------------------------- bounds
def lin_ratio(got, ref, dt: str) -> float:
    """max over elements of |got - ref| / (LIN_TOL * (|ref| + 1)); inf for a non-finite output"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / (LIN_TOL[dt] * (np.abs(ref) + 1))).max())


def norm_ratio(got, ref, dt: str) -> float:
    """max of |got - ref| / (1.05 * half an ulp * |ref| + the smallest normal)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / (NORM_SLACK * HALF_ULP[dt] * np.abs(ref) + MIN_NORMAL[dt])).max())


# -------------------------------------------------------------- references
def stored_h(op: Operands, dt: str) -> torch.Tensor:
    """h = a (+ residual) as the torch CPU add stores it in the storage type (fp32 sum, one rounding)"""
    a = t16(op.a, dt)
    return a if op.residual is None else a + t16(op.residual, dt)


def reference_fused(op: Operands, dt: str, eps: float, swiglu: bool):
    """float64 outputs [m, n_g] per group, on the stored h"""
    h = f64(stored_h(op, dt))
    if swiglu:
        return [olin.rms_swiglu(h, op.g, eps, w, wu) for w, wu in zip(op.w, op.wu)]
    return [olin.rms_linear(h, op.g, eps, w) for w in op.w]


def emulate_norm(op: Operands, dt: str, eps: float) -> torch.Tensor:
    """y in the storage type: fp32 sum of squares of the stored h, h * (1 / sqrt(mean + eps)) * g, one rounding"""
    hf = stored_h(op, dt).float()
    k = hf.shape[-1]
    inv = 1.0 / torch.sqrt((hf * hf).sum(-1, keepdim=True) / k + torch.tensor(eps, dtype=torch.float32))
    return (hf * inv * t16(op.g, dt).float()).to(TDT[dt])


def emulate_fused(op: Operands, dt: str, eps: float, swiglu: bool):
    """the fused kernel's semantics on the CPU -> float64 outputs per group"""
    y = emulate_norm(op, dt, eps).float()
    outs = []
    for i, w in enumerate(op.w):
        r = y @ t16(w, dt).float().t()
        if swiglu:
            r = r / (1 + torch.exp(-r)) * (y @ t16(op.wu[i], dt).float().t())
        outs.append(f64(r.to(TDT[dt])))
    return outs


# ---------------------------------------------------------------- case list
# kind: rms_linear / rms_swiglu / rms_qkv_into_cache; res: "res+h" residual and h_out, "res" residual only (h_out
# NULL), "none" neither, "h" h_out without a residual; pos (qkv): 0, mid-cache, S_MAX - 1, S_MAX (all dropped)
FusedCase = namedtuple("FusedCase", "kind K M B S widths padded res pos")
KS = (8, 2048, 2056, 4096, 4104, 6144, 6152, 8184, 8192)
MS = (1, 2, 3, 4)
POS = {"zero": 0, "mid": 3, "last": S_MAX - 1, "full": S_MAX}
TOKEN_SPLITS = ((1, 1), (2, 1), (4, 1), (2, 2), (1, 4), (1, 3))


def _fused_cases():
    main, lds = [], []
    kinds, res, pos = ("linear", "swiglu", "qkv"), ("res+h", "none", "res", "h"), ("mid", "zero", "last", "full")
    for ki, K in enumerate(KS):
        for M in MS:
            i = 4 * ki + M - 1
            kind = kinds[i % 3]
            if (K, kind) == (8, "swiglu"):
                # replaced, not widened: with 8 terms the rounding of y does not average out and the emulated
                # SwiGLU sits at 0.61 of the bound (bf16); K = 8 keeps the linear and qkv forms
                kind = "linear"
            if kind == "qkv":
                B, S = {1: (1, 1), 2: (2, 1), 3: (1, 3), 4: ((4, 1), (2, 2), (1, 4))[ki % 3]}[M]
                widths = (5, 3, 2)
            else:
                B, S = M, 1
                widths = (10,) if (i // 3) % 2 == 0 else (1,)
            c = FusedCase(kind, K, M, B, S, widths, bool((i // 2) % 2), res[(i + ki) % 4],
                          pos[(ki + M) % 4] if kind == "qkv" else None)
            (lds if (K, M) == (8192, 4) else main).append(c)
    main += [
        FusedCase("qkv", 2056, 4, 2, 2, (5, 3, 2), True, "res+h", "last"),   # second token of each batch dropped
        FusedCase("qkv", 4104, 4, 4, 1, (5, 3, 2), False, "none", "full"),   # caches untouched, q written
        FusedCase("qkv", 8, 4, 1, 4, (5, 3, 2), True, "res", "mid"),
        FusedCase("qkv", 6152, 3, 1, 3, (5, 3, 2), False, "res+h", "last"),
        FusedCase("qkv", 2048, 2, 2, 1, (5, 3, 2), True, "h", "zero"),
        FusedCase("qkv", 8184, 1, 1, 1, (5, 3, 2), False, "res+h", "full"),
        FusedCase("linear", 4104, 2, 2, 1, (1,), True, "res+h", None),        # h_out at ntot 1: one workgroup
        FusedCase("swiglu", 6152, 3, 3, 1, (1,), False, "res+h", None),
        FusedCase("swiglu", 2048, 4, 4, 1, (10,), True, "res", None),
        FusedCase("swiglu", 4096, 1, 1, 1, (10,), True, "h", None),          # the SwiGLU instances the rotation
        FusedCase("swiglu", 2048, 2, 2, 1, (10,), False, "none", None),      # above misses: NB 1 x RPT 2, NB 2 x RPT 1
    ]
    # m = 4, k = 8192: 65536 bytes of dynamic LDS + the 16 static; tests of their own
    lds += [FusedCase("linear", 8192, 4, 4, 1, (10,), True, "res+h", None),
            FusedCase("qkv", 8192, 4, 2, 2, (5, 3, 2), False, "res", "mid")]
    return main, lds


FUSED_CASES, LDS_CASES = _fused_cases()


def fused_instance(c: FusedCase):
    """(SW, NB, RPT) of the rms_gemm_skinny instance pli_rms_gemm_nt launches for the case"""
    return c.kind == "swiglu", 1 if c.M <= 1 else 2 if c.M <= 2 else 4, 1 if c.K <= 2048 else 2 if c.K <= 4096 else 4


def case_id(c) -> str:
    return "{}_k{}_m{}_b{}s{}_n{}{}_{}{}".format(c.kind, c.K, c.M, c.B, c.S, "-".join(map(str, c.widths)),
                                                 "_pad" if c.padded else "", c.res.replace("+", ""),
                                                 "_" + c.pos if c.pos else "")


def case_seed(c, dt: str) -> int:
    return 1000 + 37 * c.K + 101 * c.M + 7 * len(c.widths) + 3 * c.S + (500 if dt == "fp16" else 0)


def case_operands(c: FusedCase, dt: str, scale: float = 1.0) -> Operands:
    return operands(c.K, c.M, c.widths, dt, case_seed(c, dt), residual=c.res.startswith("res"),
                    swiglu=c.kind == "swiglu", scale=scale)


# pli_gemm_multi_nt (unfused q/k/v): K, B, S, widths, padded, pos
MultiCase = namedtuple("MultiCase", "K B S widths padded pos")
SKINNY_MULTI_CASES = [  # gemm_skinny_multi<NB, CPL>: CPL 2 (K <= 1024), 4 (<= 2048), 8; NB 1 / 8 / 16
    MultiCase(8, 1, 1, (6, 3, 1), False, 3),
    MultiCase(1024, 5, 1, (6, 3, 1), True, 0),
    MultiCase(1032, 2, 4, (6, 3, 1), False, S_MAX - 2),
    MultiCase(2048, 3, 3, (6, 3, 1), True, 3),
    MultiCase(2056, 16, 1, (6, 3, 1), False, S_MAX),
    MultiCase(4104, 1, 5, (6, 3, 1), True, S_MAX - 2),
    MultiCase(4104, 4, 4, (6, 3, 1), False, 3),
    MultiCase(2056, 1, 1, (6, 3, 1), True, 0),
    MultiCase(4104, 1, 8, (6, 3, 1), False, S_MAX - 2),
    MultiCase(1024, 9, 1, (6, 3, 1), False, 3),
    MultiCase(8, 8, 2, (6, 3, 1), True, S_MAX - 1),
]
SMALLM_MULTI_CASES = [  # gemm_smallm_nt<NBG, MULTI>: NBG 2 (m <= 32), 4 (<= 64), 8; kw = K / 4 per wave
    MultiCase(128, 17, 1, (32, 16, 16), False, 3),          # remainder loop only
    MultiCase(1024, 8, 4, (32, 16, 16), True, S_MAX - 2),   # one unrolled body step
    MultiCase(1152, 33, 1, (32, 16, 16), False, 0),         # body + remainder
    MultiCase(2176, 16, 4, (32, 16, 16), True, S_MAX - 2),  # two body steps + remainder
    MultiCase(1152, 13, 5, (16, 16), False, S_MAX - 2),     # two groups, 65 rows
    MultiCase(128, 2, 64, (32, 16, 16), True, S_MAX - 2),   # 128 rows, 62 tokens per batch dropped
    MultiCase(2176, 17, 1, (16, 16), True, S_MAX),          # all cache rows dropped
    MultiCase(1024, 32, 2, (32, 16, 16), False, 3),
]


def multi_id(c) -> str:
    return "k{}_b{}s{}_n{}{}_p{}".format(c.K, c.B, c.S, "-".join(map(str, c.widths)), "_pad" if c.padded else "", c.pos)


# ------------------------------------------------------ direct C ABI calls
def dtype_code(dt: str) -> int:
    return {"fp16": 1, "bf16": 2}[dt]


def call_multi(L, x2: torch.Tensor, S: int, weights, outs, pos: torch.Tensor, s_max: int, dt: str) -> int:
    """pli_gemm_multi_nt on x2 [m, k] (a view): group g = weights[g] -> outs[g] (Guarded, group 0 q-like with no
    row offset and capacity S, the others at *pos with capacity s_max).  Returns the status."""
    ng = len(weights)
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    w = (P * ng)(*(t.data_ptr() for t in weights))
    c = (P * ng)(*(o.view.data_ptr() for o in outs))
    n = (ctypes.c_int * ng)(*(t.shape[0] for t in weights))
    ldw = (I64 * ng)(*(t.stride(0) for t in weights))
    sb = (I64 * ng)(*(o.strides[0] for o in outs))
    st = (I64 * ng)(*(o.strides[1] for o in outs))
    ro = (P * ng)(*([None] + [pos.data_ptr()] * (ng - 1)))
    cap = (ctypes.c_int * ng)(*([S] + [s_max] * (ng - 1)))
    return L.pli_gemm_multi_nt(x2.data_ptr(), x2.stride(0), x2.shape[0], x2.shape[1], S, w, c, n, ldw, sb, st, ro, cap,
                               ng, dtype_code(dt), torch.cuda.current_stream().cuda_stream)


def call_rmsnorm(L, x, r, w, y, h, eps: float, dt: str) -> int:
    """pli_rmsnorm on 2-D views with their own row strides (r / h may be None)"""
    rows, n = x.shape
    return L.pli_rmsnorm(x.data_ptr(), r.data_ptr() if r is not None else None, w.data_ptr(), y.data_ptr(),
                         h.data_ptr() if h is not None else None, rows, n, x.stride(0),
                         r.stride(0) if r is not None else n, y.stride(0), h.stride(0) if h is not None else n,
                         float(eps), dtype_code(dt), torch.cuda.current_stream().cuda_stream)
