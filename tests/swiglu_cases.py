"""Route replay, case list, operands, float64 reference and the two per-element
bounds shared by the dense fused SwiGLU tests (tests/test_gpu_swiglu.py on the
GPU, tests/test_swiglu_emulation_cpu.py and tests/test_swiglu_capi.py on the
CPU).  The guarded outputs and the project's linear bound come from
tests/decode_step_cases.py.

Route replay: `swiglu_route` restates swiglu_dispatch, swiglu_slices,
splitk_slices and launch_swiglu (csrc/gemm.hip) and returns the kernel as
pli_last_route reports it with the template instance (NB / NBG / MC and ks).
Every case names the instance it is meant to reach and is asserted against the
replay when this module is imported; the GPU test asserts the name against
pli_hip.last_route().

Operands: x [m, k] = N(0,1) * sx, gate and up weights [n, k] = N(0,1) * sw *
k^-0.5, seeded per case and type and rounded to the storage type.  Kind
"default": sx 0.5, sw 1.  Kind "sat": sx 4, sw 4, so the gates have a standard
deviation of 16 and reach |g| ~ 60; the import asserts 20 <= max |g| <= 80 for
them (the sigmoid is saturated on both sides, fp32 exp(-g) stays finite and a
bf16 result stays a normal number).

Padded family (`device_operands(..., padded=True)`): x is a view with ldx =
k + 8, the gate weight one with ldwg = k + 16 and the up weight one with ldwu =
k + 8 -- deliberately another stride than the gate's, each of the seven kernels
carries the pair separately -- with NaN in all row padding and in three spare
rows after each operand.  xmode "ld4" gives ldx = k + 4 and "off1" starts x one
element into its storage: the two ways besides n % 8 and k % 8 in which a
16-bit call leaves the vector class.  The contiguous family has ld == k.

Bounds, per element, both asserted:

(a) the project's linear bound |err| <= LIN_TOL * (|ref| + 1), bf16 1e-2, fp16
    4e-3, fp32 1e-4;
(b) for h = silu(g) * u with g = x wg^T, u = x wu^T:

    |err| <= 1.05 * HALF_ULP * |ref|
             + [ K * 2^-23 * mag + (|g| + 4) * 2^-22 * |ref| ]
             + MIN_NORMAL
    mag = |silu'(g)| * |u| * (|x| |wg|^T) + |silu(g)| * (|x| |wu|^T)

    The first term is the one rounding to the storage type (1.05 is
    decode_step_cases.NORM_SLACK; fp32 outputs use 2^-24).  The bracket is the
    fp32 evaluation: a length-K fp32 dot in any order is within K * 2^-24 *
    (|x| |w|^T) of the exact one to first order, carried to h through
    dh/dg = silu'(g) u and dh/du = silu(g), allowed twice (the combine bound's
    form, tests/moe_cases.py); silu(g) = g / (1 + exp(-g)) takes the log2 e
    product, v_exp_f32, one add, a reciprocal or division and two products, each
    within an ulp or two of fp32 -- the error of the exponent's argument scales
    with |g|, hence (|g| + 4) * 2^-24 -- allowed four times.  At small K (b) is
    about 50 times tighter than (a); from K ~ 8192 on (a) is the tighter one.
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

SKINNY, SMALLM, W5, P256, MFMA, GENERIC = ("gemm_skinny_nt<swiglu>", "gemm_smallm_nt<swiglu>", "gemm_w5<swiglu>",
                                           "gemm_256p<swiglu>", "gemm_mfma<swiglu>", "gemm_generic<swiglu>")
SPLIT = "gemm_splitk_nt<swiglu>+gemm_splitk_reduce_swiglu"
ROUTES = (SKINNY, SMALLM, SPLIT, MFMA, W5, P256, GENERIC)


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ------------------------------------------------------------- route replay
def splitk_slices(m: int, n: int, k: int, target: int = 512, max_m: int = 256) -> int:
    """pli::splitk_slices: the largest power of two with tiles * ks <= target, slices >= 256 and % 64 == 0"""
    if m <= 16 or m > max_m or n % 32 != 0 or k % 64 != 0 or k < 64:
        return 0
    tiles = cdiv(n, 128) * cdiv(m, 128)
    ks = 1
    while tiles * ks * 2 <= target and k % (ks * 2 * 64) == 0 and k // (ks * 2) >= 256:
        ks *= 2
    return ks


def swiglu_slices(m: int, n: int, k: int, force: bool = False) -> int:
    if m <= 16 or m > 256:
        return 0
    if not force and m >= 256 and cdiv(m, 256) * cdiv(n, 128) >= 96:
        return 0
    return splitk_slices(m, n, k, 512)


def workspace_size(m: int, n: int, k: int, dt: str) -> int:
    """pli_gemm_swiglu_workspace_size: 2 * ks planes of m * n fp32, ks the most any variant uses"""
    if dt == "fp32" or m <= 0 or n <= 0 or k <= 0:
        return 0
    return 2 * swiglu_slices(m, n, k, True) * m * n * 4


Route = namedtuple("Route", "kernel inst")


def swiglu_route(m: int, n: int, k: int, dt: str, variant, workspace, aligned: bool = True, lds=None) -> Route:
    """The launch of pli_gemm_swiglu[_ws[_variant]] for m, n, k > 0.  variant None = 0; workspace: the bytes the call
    passes (0 / None: no workspace; True: as many as it asks for); aligned: x, wg, wu and h 16-byte aligned and
    ldh % 8 == 0; lds = (ldx, ldwg, ldwu), default (k, k, k)."""
    v = variant or 0
    ldx, ldwg, ldwu = lds or (k, k, k)
    vec = dt != "fp32" and k % 8 == 0 and n % 8 == 0 and aligned and ldx % 8 == ldwg % 8 == ldwu % 8 == 0
    ks = swiglu_slices(m, n, k, v == 1) if vec and v not in (2, 3, 4) else 0
    have = float("inf") if workspace is True else int(workspace or 0)
    if ks > 0 and have > 0 and have >= 2 * ks * m * n * 4:
        return Route(SPLIT, "MC{},ks{}".format(cdiv(min(m, 128), 32), ks))
    if vec and (m == 1 or (m <= 16 and not (k % 128 == 0 and n % 16 == 0))):
        return Route(SKINNY, "NB{}".format(1 if m <= 1 else 2 if m <= 2 else 4 if m <= 4 else 8 if m <= 8 else 16))
    if vec and m <= 128 and k % 128 == 0 and n % 16 == 0:
        return Route(SMALLM, "NBG{}".format(1 if m <= 16 else 2 if m <= 32 else 4 if m <= 64 else 8))
    tiles = cdiv(m, 256) * cdiv(n, 128)
    w5_ld = ldx * 512 < 2 ** 31 and ldwg * 256 < 2 ** 31 and ldwu * 256 < 2 ** 31
    if vec and v != 4 and (v == 3 or (m >= 256 and n >= 256)) and k % 64 == 0 and (v == 3 or tiles >= 96) and w5_ld:
        return Route(W5, "")
    if vec and m >= 256 and n >= 256 and k % 64 == 0 and tiles >= 96:
        return Route(P256, "")
    return Route(MFMA if vec else GENERIC, "")


# ---------------------------------------------------------------- case list
# xmode: "pad" ldx = k + 8; "ld4" ldx = k + 4; "off1" x one element into its storage (both leave the vector class)
SwigluCase = namedtuple("SwigluCase", "route inst m n k variant split_k kind xmode dts")
B16 = ("bf16", "fp16")


def _case(route, inst, mnk, variant=None, split_k=True, kind="default", xmode="pad", dts=B16):
    return SwigluCase(route, inst, *mnk, variant, split_k, kind, xmode, dts)


def _cases():
    cases = []
    # gemm_skinny_nt<NB, 4, SW>: one pass of the column loop is 2048 columns of K (CPL 4 chunks of 8 per lane)
    for nb, shapes in ((1, ((1, 8, 8), (1, 16, 2048), (1, 24, 2056), (1, 8, 4104))),   # one chunk, a full pass,
                       (2, ((2, 8, 136),)),                                            # + one chunk, third pass
                       (4, ((3, 24, 2056), (4, 8, 8))),
                       (8, ((5, 40, 72), (8, 8, 2048))),
                       (16, ((9, 24, 264), (16, 8, 8)))):
        cases += [_case(SKINNY, f"NB{nb}", s) for s in shapes]
    # gemm_smallm_nt<NBG, false, SW>: kw = K / 4 per wave, U = 4 steps of 32 ahead: one body step is K = 512.
    # K 128 remainder only, 512 exactly one body step, 640 / 1152 body + remainder, 1024 two body steps
    for nbg, shapes in ((1, ((2, 16, 128), (16, 16, 512), (7, 32, 640))),
                        (2, ((17, 16, 128), (32, 48, 640))),
                        (4, ((33, 16, 512), (64, 32, 1152))),
                        (8, ((65, 16, 128), (100, 16, 1024), (128, 32, 640)))):
        cases += [_case(SMALLM, f"NBG{nbg}", s, split_k=nbg == 1) for s in shapes]
    # gemm_splitk_lds_nt<MC, true, false> + gemm_splitk_reduce_swiglu
    for inst, s in (("MC1,ks1", (17, 32, 64)),          # one plane pair, one 64-k step
                    ("MC1,ks1", (32, 32, 128)),
                    ("MC2,ks2", (33, 160, 512)),        # two column tiles, the second 32 columns
                    ("MC2,ks2", (64, 32, 512)),
                    ("MC3,ks4", (65, 32, 1024)),
                    ("MC3,ks2", (96, 64, 512)),
                    ("MC4,ks2", (97, 32, 512)),
                    ("MC4,ks8", (128, 160, 2048)),
                    ("MC4,ks2", (129, 32, 512)),        # the second 128-row slab has one row
                    ("MC4,ks4", (130, 160, 1024)),
                    ("MC4,ks2", (256, 32, 512))):       # two full slabs
        cases.append(_case(SPLIT, inst, s))
    # gemm_mfma<T, true, false, true>: 128 x 64 outputs per workgroup, K tiles of 64
    cases += [_case(MFMA, "", (17, 8, 8)),                        # one chunk of K
              _case(MFMA, "", (129, 64, 64), split_k=False),      # the second row tile has one row
              _case(MFMA, "", (130, 72, 72)),                     # K tail of 8, column tail of 8
              _case(MFMA, "", (200, 136, 192))]
    # gemm_w5<swiglu>: forced (any m, n) and by default (>= 96 tiles of 256 x 128)
    cases += [_case(W5, "", (17, 8, 64), variant=3), _case(W5, "", (300, 128, 128), variant=3),
              _case(W5, "", (257, 136, 192), variant=3),
              _case(W5, "", (3072, 1024, 64)), _case(W5, "", (2817, 1000, 192))]
    # gemm_256p<T, true, false, 7, true>: the phased 256 x 128 tile, only where gemm_w5 is refused
    cases += [_case(P256, "", s, variant=4) for s in ((3072, 1024, 128), (2817, 1000, 64), (2817, 1000, 192))]
    # gemm_generic<T, true, true>: fp32, and 16-bit calls outside the vector class through n % 8, k % 8, ldx % 8
    # and a pointer that is not 16-byte aligned
    cases += [_case(GENERIC, "", (1, 1, 1), dts=("fp32",)), _case(GENERIC, "", (65, 33, 17), dts=("fp32",)),
              _case(GENERIC, "", (33, 100, 72)), _case(GENERIC, "", (5, 8, 12)),
              _case(GENERIC, "", (33, 64, 72), xmode="ld4"), _case(GENERIC, "", (33, 64, 72), xmode="off1")]
    # the "sat" kind once per route, at the route's second case
    for r in ROUTES:
        second = [c for c in cases if c.route == r][1]
        cases.append(second._replace(kind="sat"))
    return cases


SWIGLU_CASES = _cases()
PHASED_CASES = [c for c in SWIGLU_CASES if c.route == P256 and c.kind == "default"]
# the contiguous family (ld == k, ldh == n): the first default case of every route and instance that stays on its
# route without padding
CONTIG_CASES = list({(c.route, c.inst, c.dts): c for c in reversed(SWIGLU_CASES)
                     if c.kind == "default" and c.xmode == "pad"}.values())[::-1]


def case_id(c: SwigluCase) -> str:
    return "{}{}-m{}n{}k{}{}{}{}{}".format(c.route.split("+")[0].replace("<swiglu>", ""), "-" + c.inst if c.inst else "",
                                           c.m, c.n, c.k, f"-v{c.variant}" if c.variant else "",
                                           "" if c.split_k else "-nosplit", "" if c.kind == "default" else "-" + c.kind,
                                           "" if c.xmode == "pad" else "-" + c.xmode)


def leading_dims(c: SwigluCase, padded: bool = True):
    """(ldx, ldwg, ldwu, ldh) of the case's operands"""
    if not padded:
        return c.k, c.k, c.k, c.n
    return c.k + (4 if c.xmode == "ld4" else 8), c.k + 16, c.k + 8, c.n + 8


def case_route(c: SwigluCase, dt: str, padded: bool = True, workspace=None) -> Route:
    """the replay for the call pli_hip.gemm_swiglu(split_k=c.split_k, variant=c.variant) makes"""
    ws = (workspace_size(c.m, c.n, c.k, dt) if c.split_k else 0) if workspace is None else workspace
    return swiglu_route(c.m, c.n, c.k, dt, c.variant, ws, aligned=not (padded and c.xmode == "off1"),
                        lds=leading_dims(c, padded)[:3])


SCALES = {"default": (0.5, 1.0), "sat": (4.0, 4.0)}
# 2.8 million gates of 64 terms each reach 5.6 standard deviations: 90 at the "sat" deviation of 16, past the limit
# exp(-g) is held to, so this one case scales its weights by 3 (deviation 12)
SAT_SCALES = {(2817, 1000, 64): (4.0, 3.0)}


def case_seed(c: SwigluCase, dt: str) -> int:
    return 5000 + 3 * c.m + 7 * c.n + 11 * c.k + {"fp32": 0, "bf16": 100, "fp16": 600}[dt] + (50 if c.kind == "sat" else 0)


Operands = namedtuple("Operands", "x wg wu")


def operands(c: SwigluCase, dt: str) -> Operands:
    """float32 arrays holding values of dt"""
    sx, sw = SAT_SCALES.get((c.m, c.n, c.k), SCALES["sat"]) if c.kind == "sat" else SCALES[c.kind]
    seed = case_seed(c, dt)
    x = round_to_dtype(seeded_normal((c.m, c.k), seed) * np.float32(sx), dt)
    wg, wu = (round_to_dtype(seeded_normal((c.n, c.k), seed + i) * np.float32(sw * c.k ** -0.5), dt) for i in (1, 2))
    return Operands(x, wg, wu)


# ------------------------------------------------------ reference and bounds
Reference = namedtuple("Reference", "h g bracket")


def reference(op: Operands) -> Reference:
    """float64: h = silu(g) * u, g, and the bracket of bound (b) (see the module docstring)"""
    x, wg, wu = (np.asarray(a, np.float64) for a in op)
    K = x.shape[1]
    g, u = x @ wg.T, x @ wu.T
    den = 1.0 + np.exp(-g)
    sig, silu = 1.0 / den, g / den           # (silu as oracle.linear.silu writes it: h is the oracle's, bit for bit)
    dsilu = sig * (1.0 + g * (1.0 - sig))
    h = silu * u
    ax = np.abs(x)
    mag = np.abs(dsilu) * np.abs(u) * (ax @ np.abs(wg).T) + np.abs(silu) * (ax @ np.abs(wu).T)
    return Reference(h, g, K * 2.0 ** -23 * mag + (np.abs(g) + 4) * 2.0 ** -22 * np.abs(h))


@functools.lru_cache(maxsize=16)
def case_reference(c: SwigluCase, dt: str):
    """(operands, reference) of a case, computed once and shared (read-only) by the tests that need it"""
    op = operands(c, dt)
    ref = reference(op)
    for a in tuple(op) + tuple(ref):
        a.setflags(write=False)
    return op, ref


def bound_a(ref: Reference, dt: str) -> np.ndarray:
    return TOL_A[dt] * (np.abs(ref.h) + 1)


def bound_b(ref: Reference, dt: str) -> np.ndarray:
    return NORM_SLACK * ROUND[dt] * np.abs(ref.h) + ref.bracket + FLOOR[dt]


def ratios(got, ref: Reference, dt: str):
    """(max |err| / bound (a), max |err| / bound (b)) over the elements; inf for a non-finite output"""
    got = np.asarray(got, np.float64)
    if got.size == 0:
        return 0.0, 0.0
    if not np.isfinite(got).all():
        return float("inf"), float("inf")
    err = np.abs(got - ref.h)
    return float((err / bound_a(ref, dt)).max()), float((err / bound_b(ref, dt)).max())


def worst(got, ref: Reference, dt: str) -> str:
    """the element furthest over bound (b), and which term of the bound dominates there"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref.h)
    i = np.unravel_index(np.nanargmax(err / bound_b(ref, dt)), err.shape)
    return ("element {}: got {:.9g} ref {:.9g} g {:.6g} err {:.3e}; rounding term {:.3e}, bracket {:.3e}, (a) {:.3e}; "
            "{} elements over (b)").format(i, got[i], ref.h[i], ref.g[i], err[i], NORM_SLACK * ROUND[dt] * abs(ref.h[i]),
                                           ref.bracket[i], bound_a(ref, dt)[i], int((err > bound_b(ref, dt)).sum()))


# ---------------------------------------------------------------- emulation
def emulate_f32(op: Operands, ks: int = 1) -> np.ndarray:
    """the fused semantics on the CPU before the output rounding, float32 [m, n]: fp32 products and sums of the
    rounded inputs (ks > 1: the split route's ks fp32 partials over K / ks each, summed in order), then
    g / (1 + exp(-g)) * u in fp32"""
    x, wg, wu = (torch.from_numpy(np.array(a, dtype=np.float32)) for a in op)
    kslice = x.shape[1] // ks
    g = torch.zeros(x.shape[0], wg.shape[0])
    u = torch.zeros_like(g)
    for s in range(ks):
        sl = slice(s * kslice, (s + 1) * kslice if s + 1 < ks else None)
        g, u = g + x[:, sl] @ wg[:, sl].t(), u + x[:, sl] @ wu[:, sl].t()
    return (g / (1 + torch.exp(-g)) * u).numpy()


def emulate(op: Operands, dt: str, ks: int = 1) -> np.ndarray:
    """emulate_f32 with the one rounding to the storage type, as float64"""
    return f64(torch.from_numpy(emulate_f32(op, ks)).to(TDT3[dt]))


def chain_ratio(h32, ref: Reference) -> float:
    """max over elements of |h32 - ref| / the bracket of (b) (0 / 0 counts as 0)"""
    err = np.abs(np.asarray(h32, np.float64) - ref.h)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / ref.bracket)
    return float(r.max()) if r.size else 0.0


def split_ks(c: SwigluCase) -> int:
    return int(c.inst.split("ks")[1]) if c.route == SPLIT else 1


# ------------------------------------------------------------ device inputs
def _padded(a: np.ndarray, ld: int, dt: str, device, offset: int = 0) -> torch.Tensor:
    """[r, k] values as a view with row stride ld inside a NaN-filled buffer of r + 3 rows, `offset` elements in"""
    r, k = a.shape
    buf = torch.full(((r + 3) * ld + offset,), float("nan"), dtype=TDT3[dt], device=device)
    view = buf.as_strided((r, k), (ld, 1), offset)
    view.copy_(torch.from_numpy(np.array(a, dtype=np.float32)).to(TDT3[dt]))
    return view


def device_operands(c: SwigluCase, op: Operands, dt: str, device, padded: bool = True):
    """x, wg, wu on the device (see the module docstring) and the Guarded output: [m + 3, n] with row stride n + 8
    (n without padding), of which the call addresses [:m, :n]"""
    ldx, ldwg, ldwu, ldh = leading_dims(c, padded)
    if padded:
        x = _padded(op.x, ldx, dt, device, 1 if c.xmode == "off1" else 0)
        wg, wu = _padded(op.wg, ldwg, dt, device), _padded(op.wu, ldwu, dt, device)
    else:
        x, wg, wu = (torch.from_numpy(np.array(a, dtype=np.float32)).to(TDT3[dt]).to(device) for a in op)
    out = Guarded((c.m + 3, c.n), dt, device, strides=(ldh, 1))
    return x, wg, wu, out


# ------------------------------------------------------- import-time checks
for _family, _padded_family in ((SWIGLU_CASES, True), (CONTIG_CASES, False)):
    for _c in _family:
        for _dt in _c.dts:
            _r = case_route(_c, _dt, _padded_family)
            assert (_r.kernel, _r.inst) == (_c.route, _c.inst), (case_id(_c), _dt, _padded_family, _r)
assert len({case_id(c) for c in SWIGLU_CASES}) == len(SWIGLU_CASES)
assert {c.route for c in SWIGLU_CASES if c.kind == "sat"} == set(ROUTES)
assert {(c.route, c.inst, c.dts) for c in CONTIG_CASES} == {(c.route, c.inst, c.dts) for c in SWIGLU_CASES}
assert len(PHASED_CASES) == 3


def max_abs_gate(c: SwigluCase, dt: str) -> float:
    op = operands(c, dt)
    return float(np.abs(np.asarray(op.x, np.float64) @ np.asarray(op.wg, np.float64).T).max())


for _c in SWIGLU_CASES:
    if _c.kind == "sat":
        for _dt in _c.dts:
            assert 20 <= max_abs_gate(_c, _dt) <= 80, (case_id(_c), _dt, max_abs_gate(_c, _dt))
