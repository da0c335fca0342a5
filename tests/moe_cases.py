"""Inputs, float64 references, bounds and the case lists shared by the MoE
tests (tests/test_gpu_moe.py on the GPU, tests/test_moe_emulation_cpu.py on
the CPU).  The guarded outputs, padded views and the linear bound come from
tests/decode_step_cases.py.

Grouped GEMM (pli_gemm_grouped): `synthetic_routing` fixes every expert's row
count exactly, without the router.  X is [tokens, k], N(0,1) rounded to the
type; the rows of tokens no expert references are NaN, the row padding and the
weight padding of a padded case are NaN, and an expert without rows has
all-NaN weights, so a read of a wrong row or a wrong expert reaches the output
as NaN.  Reference: oracle.linear.linear / swiglu in float64 per expert on
x[gather[rows]].  rows_bound is always the number of sorted rows (sum of the
counts, include/pli.h).  `grouped_route` replays grouped_dispatch's branch
(csrc/gemm.hip) and every case's `route` field is asserted against it when
this module is imported.

Router (pli_moe_route): seeded logits in fp32 / bf16 / fp16, with an input
condition asserted at import time (`route_separation`).

Combine (pli_moe_combine): `combine_ratio`, the per-element bound

    |err| <= 1.05 * HALF_ULP[dt] * |ref| + K * 2^-23 * sum_j |w_j y_j| + MIN_NORMAL[dt]

The kernel accumulates acc_j = fma(w_j, y_j, acc_{j-1}) in fp32 from acc = 0:
K roundings, each at most 2^-24 relative to a partial sum that sum_j |w_j y_j|
bounds, so the chain is within K * 2^-24 * sum_j |w_j y_j| of the exact sum to
first order; the bound allows twice that.  Then one rounding to the storage
type, half an ulp of the rounded value (HALF_ULP is the unit roundoff, 2^-8 /
2^-11), with the 5 % slack norm_ratio gives the same step, and norm_ratio's
absolute floor, the smallest normal of the type.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from decode_step_cases import DTYPES, HALF_ULP, MIN_NORMAL, TDT, f64, row_view, t16, weight_view  # noqa: F401
from oracle import linear as olin
from oracle.numerics import round_to_dtype, seeded_normal


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ------------------------------------------------------------ grouped GEMM
def synthetic_routing(counts, tokens: int, seed: int):
    """offsets [E + 1] (the exclusive scan of counts) and gather [sum(counts)] (sorted row -> token), int32.
    Every token appears at most once per expert; token `tokens - 1 - seed % 2` is referenced by no expert; with two
    or more experts that have rows, one token is referenced by all of them."""
    counts = [int(c) for c in counts]
    assert tokens >= max(counts) + 1
    rs = np.random.RandomState(seed)
    unused = tokens - 1 - seed % 2
    pool = np.array([t for t in range(tokens) if t != unused])
    shared = int(pool[rs.randint(len(pool))])
    rest = pool[pool != shared]
    gather = []
    for c in counts:
        if c == 0:
            continue
        rows = np.concatenate([[shared], rs.choice(rest, c - 1, replace=False)])
        gather.append(rs.permutation(rows))
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return offsets, np.concatenate(gather).astype(np.int32)


def grouped_route(E: int, rows_bound: int, n: int, swiglu: bool, variant) -> str:
    """the kernel instance grouped_dispatch (csrc/gemm.hip) launches; variant None = pli_gemm_grouped.  The
    LDS-staged kernel indexes experts in blockIdx.z: past 65535 experts the default leaves it and variant 2, where
    it would have run, is an argument error (ValueError here)"""
    v, sw = variant or 0, int(bool(swiglu))
    lds_ok = rows_bound <= 1024 and n % (64 if swiglu else 128) == 0
    if lds_ok and v == 2 and E > 65535:
        raise ValueError("the LDS-staged route takes at most 65535 experts (blockIdx.z)")
    if lds_ok and E <= 65535 and v != 1 and (v == 2 or rows_bound > 16):
        return f"gemm_grouped_lds_nt<MC{cdiv(min(rows_bound, 128), 32)},SW{sw}>"
    if v != 2 and rows_bound >= 16 * E:
        return f"gemm_256g<SW{sw}>"
    nbg = 1 if rows_bound <= 16 else 2 if rows_bound <= 32 else 4 if rows_bound <= 64 else 8
    return f"gemm_grouped_nt<NBG{nbg},SW{sw}>"


GroupedCase = namedtuple("GroupedCase", "route E counts n k swiglu variant padded use_gather")


def _gc(route, E, counts, n, k, swiglu, variant=None, padded=False, use_gather=True):
    counts = tuple(counts) + (0,) * (E - len(counts))
    return GroupedCase(route, E, counts, n, k, bool(swiglu), variant, padded, use_gather)


def _grouped_cases():
    nt, lds, g256 = "gemm_grouped_nt<NBG{},SW{}>", "gemm_grouped_lds_nt<MC{},SW{}>", "gemm_256g<SW{}>"
    cases = [
        # gemm_grouped_nt: n = 48 (three column blocks, the LDS route never applies).  Per wave kw = k / 4 and the
        # unrolled body steps 32 * U (U 8 plain, 4 SwiGLU): it needs k >= 1024 plain, k >= 512 SwiGLU.
        _gc(nt.format(1, 0), 8, (1, 0, 7, 8), 48, 128, False, padded=True),             # remainder loop only
        _gc(nt.format(1, 1), 8, (16,), 48, 512, True),                                  # exactly one body step
        _gc(nt.format(2, 0), 8, (17, 0, 15), 48, 1024, False),                          # exactly one body step
        _gc(nt.format(4, 1), 8, (33, 31), 48, 640, True, padded=True),                  # body + remainder
        _gc(nt.format(8, 0), 8, (65, 20, 0, 15), 48, 1152, False, padded=True, use_gather=False),  # body + remainder
        _gc(nt.format(8, 1), 16, (130, 1) + (0,) * 13 + (69,), 48, 128, True),          # two chunks, the second 2 rows
        _gc(nt.format(2, 1), 8, (0, 17, 15), 48, 512, True, use_gather=False),          # (the two instances the
        _gc(nt.format(4, 0), 8, (31, 0, 0, 33), 48, 1152, False),                       # rows above leave out)
        _gc(nt.format(1, 0), 8, (3, 0, 5), 128, 256, False, variant=1),                 # n % 64 == 0: forced off LDS
        _gc(nt.format(4, 1), 8, (0, 40, 9), 64, 128, True, variant=1, padded=True),
    ]
    # gemm_grouped_lds_nt: one tile (n 128 plain / 64 SwiGLU); the MC 3 row takes three tiles (384 / 192)
    for mc, E, counts, k, variant, tiles, padded, ug in (
            (1, 4, (1, 0, 9, 6), 128, 2, 1, False, True),
            (2, 4, (33, 0, 31), 128, None, 1, True, True),
            (3, 4, (65, 1, 0, 30), 384, None, 3, True, True),
            (4, 4, (97, 3), 256, None, 1, False, False),
            (4, 4, (129, 0, 257, 128), 128, None, 1, True, True),   # slabs of 128 + 1, 128 + 128 + 1, 128 rows
            (4, 2, (1024, 0), 128, None, 1, False, True)):          # rows_bound at the limit, 8 slabs
        for sw in (False, True):
            cases.append(_gc(lds.format(mc, int(sw)), E, counts, tiles * (64 if sw else 128), k, sw, variant,
                             padded, ug))
    # gemm_256g: 256-row slots per expert
    for E, counts, n_plain, n_sw, k, variant, padded, ug in (
            (2, (255, 257), 256, 128, 128, 1, True, True),
            (3, (256, 0, 1), 272, 144, 384, None, False, True),     # ragged last column tile, empty expert inside
            (2, (1100, 1100), 128, 128, 128, None, False, True)):   # 10 slots: the rows_bound contract
        for sw in (False, True):
            cases.append(_gc(g256.format(int(sw)), E, counts, n_sw if sw else n_plain, k, sw, variant, padded,
                             ug and not (sw and E == 3)))
    return cases


GROUPED_CASES = _grouped_cases()
# shapes that more than one route accepts: each of variant None / 1 / 2 is held to the oracle per element
AGREEMENT_SHAPES = [
    _gc(None, 8, (3, 0, 5), 128, 256, False),         # NT NBG 1 (default, 1) / LDS MC 1 (2)
    _gc(None, 4, (33, 0, 31), 64, 128, True, padded=True),   # LDS MC 2 (default, 2) / 256g (1)
    _gc(None, 2, (255, 257), 256, 128, False),        # LDS MC 4 (default, 2) / 256g (1)
]
AGREEMENT_CASES = [c._replace(route=grouped_route(c.E, sum(c.counts), c.n, c.swiglu, v), variant=v)
                   for c in AGREEMENT_SHAPES for v in (None, 1, 2)]
# the chain h = SwiGLU grouped GEMM, y = W2 over the stored h, combine over the stored y: (first stage, n of W2)
CHAIN_CASES = [
    (_gc("gemm_grouped_lds_nt<MC2,SW1>", 4, (33, 0, 31), 128, 128, True, padded=True), 128),
    (_gc("gemm_256g<SW1>", 2, (255, 257), 128, 128, True, variant=1), 256),
]


def rows_bound(c: GroupedCase) -> int:
    return sum(c.counts)


def grouped_id(c: GroupedCase) -> str:
    return "{}-E{}-c{}-n{}-k{}-v{}{}{}".format(c.route, c.E, ".".join(str(x) for x in c.counts if x) +
                                               ("+%dx0" % c.counts.count(0) if 0 in c.counts else ""), c.n, c.k,
                                               c.variant or 0, "-pad" if c.padded else "",
                                               "" if c.use_gather else "-sorted")


for _c in GROUPED_CASES + AGREEMENT_CASES + [c for c, _ in CHAIN_CASES]:
    assert _c.route == grouped_route(_c.E, rows_bound(_c), _c.n, _c.swiglu, _c.variant), grouped_id(_c)
    assert len(_c.counts) == _c.E and _c.k % 128 == 0 and _c.n % 16 == 0, grouped_id(_c)
assert len({grouped_id(c) for c in GROUPED_CASES}) == len(GROUPED_CASES)


def grouped_seed(c: GroupedCase, dt: str) -> int:
    return 3000 + 11 * c.k + 7 * c.n + 13 * rows_bound(c) + 5 * c.E + 2 * c.swiglu + (500 if dt == "fp16" else 0)


GroupedOperands = namedtuple("GroupedOperands", "x w wu gather offsets tokens")


def grouped_operands(c: GroupedCase, dt: str) -> GroupedOperands:
    """float32 arrays rounded to dt: x [tokens, k] (NaN rows where no expert reads), one [n, k] weight per expert
    (and an up weight each with SwiGLU; all NaN for an expert without rows), gather, offsets"""
    seed = grouped_seed(c, dt)
    tokens = max(c.counts) + 3
    offsets, gather = synthetic_routing(c.counts, tokens, seed)
    x = round_to_dtype(seeded_normal((tokens, c.k), seed + 1), dt)
    used = np.zeros(tokens, bool)
    used[gather] = True
    x[~used] = np.nan

    def wgt(s, e):
        if c.counts[e] == 0:
            return np.full((c.n, c.k), np.nan, np.float32)
        return round_to_dtype(seeded_normal((c.n, c.k), s) * np.float32(c.k ** -0.5), dt)

    w = [wgt(seed + 10 + e, e) for e in range(c.E)]
    wu = [wgt(seed + 110 + e, e) for e in range(c.E)] if c.swiglu else None
    return GroupedOperands(x, w, wu, gather, offsets, tokens)


def grouped_reference(op: GroupedOperands, x_sorted=None) -> np.ndarray:
    """float64 [rows, n]: per expert, linear / swiglu on x[gather[rows]] (or on x_sorted's rows)"""
    xs = np.asarray(op.x, np.float64)[op.gather] if x_sorted is None else np.asarray(x_sorted, np.float64)
    out = np.zeros((xs.shape[0], op.w[0].shape[0]))
    for e in range(len(op.w)):
        a, b = int(op.offsets[e]), int(op.offsets[e + 1])
        if a == b:
            continue
        out[a:b] = olin.swiglu(xs[a:b], op.w[e], op.wu[e]) if op.wu is not None else olin.linear(xs[a:b], op.w[e])
    return out


def emulate_grouped(op: GroupedOperands, dt: str) -> np.ndarray:
    """the grouped kernels' semantics on the CPU: fp32 dot of the 16-bit operands, SwiGLU in fp32, one rounding"""
    xs = t16(op.x[op.gather], dt).float()
    out = torch.zeros(xs.shape[0], op.w[0].shape[0], dtype=TDT[dt])
    for e in range(len(op.w)):
        a, b = int(op.offsets[e]), int(op.offsets[e + 1])
        if a == b:
            continue
        r = xs[a:b] @ t16(op.w[e], dt).float().t()
        if op.wu is not None:
            r = r / (1 + torch.exp(-r)) * (xs[a:b] @ t16(op.wu[e], dt).float().t())
        out[a:b] = r.to(TDT[dt])
    return f64(out)


GroupedDevice = namedtuple("GroupedDevice", "x gather w wu offsets")


def grouped_device(c: GroupedCase, op: GroupedOperands, dt: str, device) -> GroupedDevice:
    """the operands on `device`: x a row_view (row stride k + 8 with NaN when padded; already sorted and gather
    None without use_gather), weight_view per expert, int32 gather / offsets"""
    pad = 8 if c.padded else 0
    if c.use_gather:
        x, gather = row_view(op.x, dt, device, pad), torch.from_numpy(op.gather).to(device)
    else:
        x, gather = row_view(op.x[op.gather], dt, device, pad), None
    w = [weight_view(a, dt, device, c.padded) for a in op.w]
    wu = [weight_view(a, dt, device, c.padded) for a in op.wu] if op.wu is not None else None
    return GroupedDevice(x, gather, w, wu, torch.from_numpy(op.offsets).to(device))


# ------------------------------------------------------------------ router
INT_SENTINEL = -1024


class GuardedInts:
    """n int32 elements inside a buffer filled with INT_SENTINEL (no index, count or offset the router writes is
    negative), `guard` elements of it before and after"""

    def __init__(self, n: int, device, guard: int = 64):
        self.n, self.guard = int(n), guard
        self.buf = torch.full((2 * guard + self.n,), INT_SENTINEL, dtype=torch.int32, device=device)
        self.view = self.buf[guard:guard + self.n]

    def stray_writes(self, written: int | None = None) -> torch.Tensor:
        """offsets from the view of the elements outside its first `written` (default all) that changed"""
        w = self.n if written is None else written
        bad = self.buf != INT_SENTINEL
        bad[self.guard:self.guard + w] = False
        return bad.nonzero().flatten() - self.guard


RouteCase =namedtuple("RouteCase", "T E k logits_dtype normalize ld_pad kind")
ROUTE_TEK = ((1, 1, 1), (3, 5, 5), (4, 8, 2), (5, 33, 8), (9, 64, 8), (37, 8, 2), (130, 64, 1), (256, 16, 4))
LOGITS_DTYPES = ("fp32", "bf16", "fp16")
ROUTE_KINDS = ("normal", "scaled", "equal_row", "dup", "dead")
DEAD = {8: (3, 7), 16: (3, 7, 11), 33: tuple(range(2, 33, 3)) + tuple(range(1, 33, 3))}  # experts at -100
SEPARATION = 1e-5  # an order of magnitude over the fp32 softmax's error


def _route_cases():
    cases = []
    for i, (T, E, k) in enumerate(ROUTE_TEK):
        for j, ld in enumerate(LOGITS_DTYPES):
            cases.append(RouteCase(T, E, k, ld, 1, (0, 3)[(i + j) % 2], "normal"))
    cases += [RouteCase(4, 8, 2, "fp32", 0, 0, "normal"), RouteCase(9, 64, 8, "bf16", 0, 3, "normal"),
              RouteCase(37, 8, 2, "fp16", 0, 1, "normal"), RouteCase(1, 1, 1, "fp32", 0, 5, "normal"),
              RouteCase(256, 16, 4, "fp16", 0, 0, "normal")]
    cases += [RouteCase(5, 33, 8, "fp32", 1, 0, "scaled"), RouteCase(9, 64, 8, "bf16", 1, 3, "scaled"),
              RouteCase(37, 8, 2, "fp16", 1, 0, "scaled"), RouteCase(4, 8, 2, "fp32", 0, 3, "scaled")]
    cases += [RouteCase(3, 5, 5, "bf16", 1, 0, "equal_row"), RouteCase(9, 64, 8, "fp32", 1, 0, "equal_row"),
              RouteCase(4, 8, 2, "fp16", 1, 3, "equal_row"), RouteCase(130, 64, 1, "fp32", 0, 3, "equal_row")]
    cases += [RouteCase(130, 64, 1, ld, 1, 0, "dup") for ld in LOGITS_DTYPES]
    cases += [RouteCase(4, 8, 2, "fp32", 1, 3, "dup"), RouteCase(9, 64, 8, "fp16", 0, 0, "dup")]
    cases += [RouteCase(37, 8, 2, "fp32", 1, 0, "dead"), RouteCase(256, 16, 4, "fp16", 1, 3, "dead"),
              RouteCase(5, 33, 8, "bf16", 1, 0, "dead")]
    return cases


ROUTE_CASES = _route_cases()


def route_id(c: RouteCase) -> str:
    return "moe_route_kernel<{}>-T{}-E{}-k{}-{}{}{}".format({"fp32": "float", "bf16": "bf16", "fp16": "f16"}[
        c.logits_dtype], c.T, c.E, c.k, c.kind, "" if c.normalize else "-raw", "-ld+%d" % c.ld_pad if c.ld_pad else "")


def route_logits(c: RouteCase) -> np.ndarray:
    """float32 [T, E] logits holding values of c.logits_dtype"""
    lg = seeded_normal((c.T, c.E), 7000 + c.T * c.E + c.k)
    if c.kind == "scaled":
        lg = lg * np.float32(30)   # exp overflows fp32 without the max subtraction
    elif c.kind == "dead":
        lg[:, list(DEAD[c.E])] -= np.float32(100)
    lg = round_to_dtype(lg, c.logits_dtype)
    if c.kind == "equal_row":
        lg[c.T // 2, :] = np.float32(0.5)          # top-k must be experts 0 .. k-1
    elif c.kind == "dup":
        for t in range(c.T):                       # two experts share the row maximum exactly
            m = int(np.argmax(lg[t]))
            lg[t, (m + 3 + t % 5) % c.E] = lg[t, m]
    return lg


def route_separation(logits: np.ndarray, k: int) -> float:
    """the input condition: per token, among the k + 1 largest oracle probabilities, adjacent ones are exactly equal
    or at least SEPARATION apart relative to the larger.  Returns the smallest non-zero relative gap (inf if none)."""
    lg = np.asarray(logits, np.float64)
    p = np.exp(lg - lg.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    top = -np.sort(-p, axis=-1)[:, :k + 1]
    if top.shape[1] < 2:
        return float("inf")
    gap = (top[:, :-1] - top[:, 1:]) / top[:, :-1]
    return float(gap[gap > 0].min()) if (gap > 0).any() else float("inf")


def _fp32_representable(logits: np.ndarray, k: int) -> bool:
    """every probability the top-k can select stays a normal fp32 number relative to the row maximum (exp(-80) is
    1.8e-35), so the fp32 softmax does not collapse two of them to zero"""
    lg = np.asarray(logits, np.float64)
    kth = -np.sort(-lg, axis=-1)[:, min(k, lg.shape[1]) - 1]
    return bool((lg.max(-1) - kth < 80).all())


for _c in ROUTE_CASES:
    assert _c.k <= _c.E and (_c.kind != "dead" or _c.k <= _c.E - len(DEAD[_c.E])), route_id(_c)
    assert route_separation(route_logits(_c), _c.k) >= SEPARATION, route_id(_c)
    assert _fp32_representable(route_logits(_c), _c.k), route_id(_c)
assert len({route_id(c) for c in ROUTE_CASES}) == len(ROUTE_CASES)


# ----------------------------------------------------------------- combine
CombineCase = namedtuple("CombineCase", "T K H padded")
COMBINE_CASES = [
    CombineCase(1, 1, 8, False), CombineCase(3, 2, 8, True), CombineCase(3, 8, 8, False),
    CombineCase(1, 2, 2048, True), CombineCase(3, 8, 2048, False),    # one pass of the column loop, all 256 threads
    CombineCase(1, 8, 2056, True), CombineCase(3, 1, 2056, False),    # the second pass: one thread
    CombineCase(3, 2, 2056, True),
    CombineCase(1, 1, 4104, False), CombineCase(3, 2, 4104, True),    # a third pass
    CombineCase(1, 8, 4104, True),
]


def combine_id(c: CombineCase) -> str:
    return "T{}-K{}-H{}{}".format(c.T, c.K, c.H, "-pad" if c.padded else "")


CombineOperands = namedtuple("CombineOperands", "y pos w")


def combine_operands(T: int, K: int, H: int, dt: str, rows: int | None = None, seed: int | None = None):
    """y [R, H] float32 rounded to dt with R > T * K and NaN in the rows no pos names, pos [T, K] a seeded injective
    map into the rows, w [T, K] fp32 N(0,1) (mixed signs) with one exact zero when there is more than one"""
    seed = 9000 + 17 * T + 5 * K + H + (500 if dt == "fp16" else 0) if seed is None else seed
    R = T * K + 3 if rows is None else rows
    assert R > T * K
    rs = np.random.RandomState(seed)
    pos = rs.permutation(R)[:T * K].astype(np.int32).reshape(T, K)
    y = round_to_dtype(seeded_normal((R, H), seed + 1), dt)
    named = np.zeros(R, bool)
    named[pos.ravel()] = True
    y[~named] = np.nan
    w = np.abs(seeded_normal((T, K), seed + 2)) * np.where(np.arange(T * K).reshape(T, K) % 2, -1, 1).astype(np.float32)
    if T * K > 1:
        w[0, 0] = 0.0
        assert T * K < 3 or ((w > 0).any() and (w < 0).any())
    return CombineOperands(y, pos, w)


def combine_reference(y, pos, w):
    """float64 out [T, H] = sum_j w y[pos] and the magnitude sum_j |w y[pos]|"""
    terms = np.asarray(w, np.float64)[:, :, None] * np.asarray(y, np.float64)[np.asarray(pos)]
    return terms.sum(1), np.abs(terms).sum(1)


def emulate_combine_f32(y, pos, w) -> np.ndarray:
    """the kernel's fp32 chain acc = fma(w_j, y_j, acc) from 0, before the output rounding: float32 [T, H].  The
    product of a 24-bit and an at most 11-bit significand is exact in float64, so one float64 add rounded to
    float32 is the fma up to double rounding."""
    y, w = np.asarray(y, np.float32), np.asarray(w, np.float32)
    acc = np.zeros((w.shape[0], y.shape[1]), np.float32)
    for j in range(w.shape[1]):
        acc = (w[:, j, None].astype(np.float64) * y[pos[:, j]].astype(np.float64) + acc.astype(np.float64)).astype(
            np.float32)
    return acc


def emulate_combine(y, pos, w, dt: str) -> np.ndarray:
    return f64(torch.from_numpy(emulate_combine_f32(y, pos, w)).to(TDT[dt]))


def combine_bound(ref, mag, K: int, dt: str) -> np.ndarray:
    return 1.05 * HALF_ULP[dt] * np.abs(ref) + K * 2.0 ** -23 * np.asarray(mag, np.float64) + MIN_NORMAL[dt]


def combine_ratio(got, ref, mag, K: int, dt: str) -> float:
    """max over elements of |got - ref| / combine_bound (see the module docstring); inf for a non-finite output"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / combine_bound(ref, mag, K, dt)).max())
