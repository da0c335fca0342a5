"""The sampling rule in float64, Philox4x32-10 in uint64 arithmetic, and the case
list shared by the sampling tests (tests/test_gpu_sample.py and
tests/test_gpu_sample_decode.py on the GPU; tests/test_sample_emulation_cpu.py,
tests/test_ch02_sampling_cpu.py and tests/test_sample_plan.py on the CPU).

The rule (DESIGN.md "Sampling", include/pli.h pli_sample), for one row of
logits x_i widened to float64 and the host parameters temperature, top_k,
top_p (each the fp32 value the entry point receives, widened):

 1. NaN counts as -inf, -0 as +0.  No logit above -inf: token -1.  With a +inf
    in the row the +inf logits weigh 1 and all others 0.
 2. "Before": larger value first, lower index first among equal values.
 3. temperature == 0: the first token.
 4. K1: the first top_k tokens (top_k <= 0 or >= vocab: all).
 5. w_i = exp((x_i - m) / temperature), S1 = sum over K1.
 6. token i of K1 is kept iff the weight of the K1 tokens before it is
    <= top_p * S1 (the first always; top_p >= 1: all).  K2, S2.
 7. walk K2 in ascending index, take the first token whose running sum exceeds
    u * S2 (the last token of K2 if rounding leaves none: never in float64).
 8. u = uniforms[row], or (r0 >> 8) * 2^-24 with r0 the first Philox4x32-10
    word for key {seed lo, seed hi}, counter {(uint32)offset, row, 0, 0}.

The input condition and delta
-----------------------------
The kernel computes w_i in fp32 and sums integers; the oracle sums float64.
Both pick the same token when no decision sits within the arithmetic's error of
its threshold.  Every row of every case therefore satisfies, asserted when this
module is imported (`check_row`):

  (u)  |u - c_j| >= 2 delta for every interior boundary c_j = (sum of the first
       j weights of K2 in index order) / S2, 0 < j < |K2|.  The ends 0 and 1 are
       no decisions: u is in [0, 1), so u = 0 and u = 1 - 2^-24 are allowed
       where the first / last token's own probability exceeds 2 delta.
  (p)  |top_p - b_j| >= 2 delta for every token j >= 1 of K1 in the order, b_j =
       (weight of the K1 tokens before j) / S1 -- the prefixes inside a group of
       tied tokens included, since the order lists ties one by one.  (Token 0 is
       always kept; top_p >= 1 and temperature == 0 take no such decision.)

delta comes from the kernel's arithmetic (csrc/sample.hip, csrc/sample_plan.h):

  * a_i = (x_i - m) / temperature: one fp32 subtraction and one correctly
    rounded fp32 division, |error| <= |a_i| 2^-23 to first order, which is a
    relative error |a_i| 2^-23 of w_i = exp(a_i);
  * the device expf: <= 2 ulp = 2^-22 relative (the library documents 1 ulp);
  * so each weight is off by at most e_i w_i, e_i = (|a_i| + 2) 2^-23.  For any
    subset A of the summed set, with p_i = w_i / S, |a_i| = ln(1 / w_i) <=
    ln(1 / p_i) because S >= 1 (the maximum weighs exactly 1), hence
    sum_i p_i |a_i| <= the entropy of p <= ln(vocab) <= ln(262144) < 12.5 and
    E = sum_i w_i e_i <= 14.5 * 2^-23 * S.  A ratio A / S then moves by at most
    (E S + A E) / (S S') <= 2 E / S' = 29 * 2^-23 (1 + O(2^-19));
  * the fixed point: floor(w 2^45) drops < 2^-45 per weight, < vocab 2^-45 <=
    2^-27 of S over a row; there is NO rounding in any sum (64-bit integer adds
    in LDS atomics, wave shuffles and serial loops: no terms-per-lane or tree
    depth enters), and top_p * S1 / u * S2 are one fp64 product and a floor
    each: 2^-53 relative + one unit of 2^-45;
  * total <= 29 * 2^-23 + 2^-26 < 29.2 * 2^-23 = 3.48e-6.

DELTA = 2^-18 = 3.81e-6 covers it; the conditions use 2 * DELTA = 2^-17.

A row that misses the condition is redrawn (its logits from the next seed);
no row is skipped and no case dropped.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from oracle.numerics import round_to_dtype

DELTA = 2.0 ** -18
WAVES, THREADS, MAX_VOCAB, FRAC_BITS = 16, 1024, 262144, 45   # csrc/sample_plan.h
DTYPES = ("fp32", "fp16", "bf16")
DTYPE_CODE = {"fp32": 0, "fp16": 1, "bf16": 2}
U_MAX = np.float32(1.0 - 2.0 ** -24)   # the largest fp32 below 1

# ------------------------------------------------------------------ Philox
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2; returns the 4 output words as uint64 arrays < 2^32"""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & _MASK for v in key]
    c = list(np.broadcast_arrays(*c))
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(_W0)) & _MASK, (k[1] + np.uint64(_W1)) & _MASK]
    return c


def philox_u(seed: int, offset: int, rows) -> np.ndarray:
    """u of rows `rows` (array) as float32: counter {(uint32)offset, row, 0, 0}, key {seed lo, seed hi}"""
    rows = np.asarray(rows, dtype=np.uint64)
    r0 = philox4x32_10((int(offset) & 0xFFFFFFFF, rows, 0, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[0]
    return ((r0 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


# ------------------------------------------------------------------ the rule
Pick = namedtuple("Pick", "token k1 k2 margin_u margin_p")


def oracle_row(x, temperature, top_k, top_p, u) -> Pick:
    """the rule on one row (values of any float dtype) in float64; margins are the distances of conditions (u), (p)
    (inf where no such decision is taken)"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x = np.asarray(x).astype(np.float64)
        x = np.where(np.isnan(x), -np.inf, x) + 0.0      # (-0 + 0 = +0)
        t, p, u = float(np.float32(temperature)), float(np.float32(top_p)), float(np.float32(u))
        V = x.size
        none = np.empty(0, dtype=np.int64)
        if not (x > -np.inf).any():
            return Pick(-1, none, none, np.inf, np.inf)
        order = np.lexsort((np.arange(V), -x))           # larger value first, lower index first
        if t == 0.0:
            return Pick(int(order[0]), order[:1], order[:1], np.inf, np.inf)
        m = x.max()
        w = (x == np.inf).astype(np.float64) if m == np.inf else np.exp((x - m) / t)
        k1 = order if (top_k <= 0 or top_k >= V) else order[:top_k]
        wk = w[k1]
        margin_p = np.inf
        if p >= 1.0:
            k2 = k1
        else:
            s1 = wk.sum()
            before = np.cumsum(wk) - wk
            keep = before <= p * s1
            keep[0] = True
            k2 = k1[keep]
            if k1.size > 1:
                margin_p = float(np.abs(p - before[1:] / s1).min())
        ids = np.sort(k2)
        c = np.cumsum(w[ids])
        hit = np.nonzero(c > u * c[-1])[0]
        token = int(ids[hit[0]]) if hit.size else int(ids[-1])
        margin_u = float(np.abs(u - c[:-1] / c[-1]).min()) if ids.size > 1 else np.inf
        return Pick(token, k1, k2, margin_u, margin_p)


def check_row(pick: Pick) -> bool:
    return pick.margin_u >= 2 * DELTA and pick.margin_p >= 2 * DELTA


# ------------------------------------------------------------------ cases
# kind: how a row's logits are made (make_row); uniforms: None (Philox) or a tuple of per-row u values cycled over
# the rows; offset_dev: None or the int32 the device tensor holds
Case = namedtuple("Case", "name rows vocab dtype kind temperature top_k top_p uniforms seed offset_dev offset_add")


def _case(name, rows, vocab, dtype, kind="normal", t=1.0, k=0, p=1.0, uniforms=None, seed=0, offset_dev=None,
          offset_add=0):
    return Case(name, rows, vocab, dtype, kind, float(t), int(k), float(p), uniforms, int(seed), offset_dev,
                int(offset_add))


def make_row(kind: str, vocab: int, dtype: str, seed: int) -> np.ndarray:
    """one row of logits as float32 values representable in `dtype` (NaN, +-inf and -0 kept)"""
    rs = np.random.RandomState(seed % (2 ** 32))
    x = (rs.standard_normal(vocab) * 2.0).astype(np.float32)
    if kind == "normal":
        pass
    elif kind == "equal":                      # every logit the same
        x[:] = np.float32(rs.standard_normal())
    elif kind == "bf16q":                      # bf16-quantised N(0, 1): ties en masse at a large vocab
        x = round_to_dtype(rs.standard_normal(vocab).astype(np.float32), "bf16")
    elif kind == "tie_top":                    # a group of ties around the head of the order (straddles small top_k
        g = min(vocab, 6)                      # cuts and top_p cuts): 6 tokens share the 2nd largest value
        srt = np.sort(x)[::-1]
        x[rs.permutation(vocab)[:g]] = srt[min(1, vocab - 1)]
    elif kind == "tie_p":                      # one token at 2, ten tied at 1, the rest near -6: at temperature 1 the
        x = (-6.0 + 0.25 * x).astype(np.float32)   # top_p cuts 0.5 and 0.9 fall inside the tie group
        idx = rs.permutation(vocab)[:11]
        x[idx[0]], x[idx[1:]] = 2.0, 1.0
    elif kind == "zeros":                     # +0 and -0 mixed in, some of them the maximum's ties
        x = -np.abs(x)
        idx = rs.permutation(vocab)[:max(2, vocab // 4)]
        x[idx[::2]] = np.float32(0.0)
        x[idx[1::2]] = np.float32(-0.0)
    elif kind == "special":                    # NaN and -inf scattered
        idx = rs.permutation(vocab)[:max(1, vocab // 3)]
        x[idx[::2]] = np.nan
        x[idx[1::2]] = -np.inf
    elif kind == "none":                       # only -inf and NaN: token -1
        x[:] = -np.inf
        x[rs.permutation(vocab)[:vocab // 2]] = np.nan
    elif kind == "inf1":                       # one +inf (and a NaN, a -inf)
        x[rs.randint(vocab)] = np.inf
        if vocab > 2:
            free = np.nonzero(x != np.inf)[0]
            x[free[0]], x[free[-1]] = np.nan, -np.inf
    elif kind == "infs":                       # several +inf
        x[rs.permutation(vocab)[:min(vocab, 5)]] = np.inf
    else:
        raise ValueError(kind)
    return round_to_dtype(x, dtype)


def case_uniforms(case: Case):
    """u per row (float32): the caller's array, or the Philox values of (seed, offset, row)"""
    if case.uniforms is not None:
        return np.array([case.uniforms[r % len(case.uniforms)] for r in range(case.rows)], dtype=np.float32)
    return philox_u(case.seed, (case.offset_dev or 0) + case.offset_add, np.arange(case.rows))


_built: dict = {}


def build(case: Case):
    """(logits float32 [rows, vocab] of dtype-representable values, u float32 [rows], expected tokens int64 [rows]);
    each row is redrawn until it meets the input condition, then asserted; computed once per case"""
    if case.name in _built:
        return _built[case.name]
    u = case_uniforms(case)
    base = sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)) * 7919
    logits = np.empty((case.rows, case.vocab), dtype=np.float32)
    want = np.empty(case.rows, dtype=np.int64)
    for r in range(case.rows):
        for attempt in range(400):
            x = make_row(case.kind, case.vocab, case.dtype, base + 104729 * r + attempt)
            pick = oracle_row(x, case.temperature, case.top_k, case.top_p, u[r])
            if check_row(pick):
                break
        assert check_row(pick), f"{case.name} row {r}: no draw meets the input condition ({pick.margin_u}, {pick.margin_p})"
        logits[r], want[r] = x, pick.token
    _built[case.name] = (logits, u, want)
    return _built[case.name]


def _cases():
    cs = []
    # (temperature, top_k, top_p) products walked over the vocab sweep ("v" = vocab)
    combos = [(1.0, 0, 1.0), (0.25, 7, 0.9), (4.0, 2, 0.5), (1.0, 50, 0.999), (0.0, 3, 0.5), (1.0, "v-1", 0.1),
              (0.25, "v", 0.5), (4.0, "v+5", 0.9), (1.0, 1, 1.0), (1.0, 0, 0.0), (0.25, 0, 0.5)]
    vocabs = (1, 2, 63, 64, 65, 255, 256, 257, THREADS - 1, THREADS, THREADS + 1)

    def tk(k, v):
        return {"v-1": v - 1, "v": v, "v+5": v + 5}.get(k, k)

    n = 0
    for v in vocabs:
        for dt in DTYPES:
            t, k, p = combos[n % len(combos)]
            cs.append(_case(f"vocab{v}_{dt}", (1, 3, 33)[n % 3], v, dt, t=t, k=tk(k, v), p=p, seed=1000 + n,
                            offset_add=n))
            n += 1
    # top_k x top_p x temperature at one vocab past the 1024-element step and one below a wave
    for v, dt in ((1025, "bf16"), (257, "fp32"), (50, "fp16")):
        for k in (1, 2, 7, 50, "v-1", "v", "v+5", 0):
            for p in (0.0, 0.1, 0.5, 0.9, 0.999, 1.0):
                t = (0.25, 1.0, 4.0)[n % 3]
                cs.append(_case(f"kp_v{v}_k{k}_p{p}", 3, v, dt, t=t, k=tk(k, v), p=p, seed=n, offset_add=3 * n))
                n += 1
    for dt in DTYPES:
        for t in (0.0, 0.25, 1.0, 4.0):
            cs.append(_case(f"temp{t}_{dt}", 33, 300, dt, t=t, k=40, p=0.9, seed=77 + n))
            n += 1
    # ties
    for dt in DTYPES:
        for t, k, p in ((0.0, 0, 1.0), (1.0, 0, 1.0), (1.0, 5, 1.0), (1.0, 0, 0.5), (1.0, 9, 0.5)):
            cs.append(_case(f"equal_{dt}_t{t}_k{k}_p{p}", 3, 131, dt, "equal", t=t, k=k, p=p, seed=n))
            n += 1
        for k, p in ((3, 1.0), (4, 1.0), (5, 0.9), (1, 1.0)):    # the top-k cut inside the tie group
            cs.append(_case(f"tie_top_{dt}_k{k}_p{p}", 3, 200, dt, "tie_top", t=1.0, k=k, p=p, seed=n))
            n += 1
        for k, p in ((0, 0.5), (0, 0.9), (8, 0.5)):              # the top-p cut inside it (after top-k cut it: k = 8)
            cs.append(_case(f"tie_p_{dt}_k{k}_p{p}", 3, 200, dt, "tie_p", t=1.0, k=k, p=p, seed=n))
            n += 1
        cs.append(_case(f"tie_top_greedy_{dt}", 3, 200, dt, "tie_top", t=0.0))
        for t, k, p in ((0.0, 0, 1.0), (1.0, 0, 1.0), (1.0, 4, 0.9), (0.25, 0, 0.5)):
            cs.append(_case(f"zeros_{dt}_t{t}_k{k}_p{p}", 3, 96, dt, "zeros", t=t, k=k, p=p, seed=n))
            n += 1
    # special values
    for dt in DTYPES:
        for kind in ("special", "none", "inf1", "infs"):
            for t, k, p in ((0.0, 0, 1.0), (1.0, 0, 1.0), (1.0, 3, 0.5), (0.25, 90, 0.9)):
                cs.append(_case(f"{kind}_{dt}_t{t}_k{k}_p{p}", 3, 90, dt, kind, t=t, k=k, p=p, seed=n))
                n += 1
    # the caller's uniforms, 0 and the largest fp32 below 1 among them
    us = (0.0, float(U_MAX), 0.5, 0.123456789, 0.75)
    for dt in DTYPES:
        cs.append(_case(f"uniforms_{dt}", 33, 70, dt, t=1.0, uniforms=us))
        cs.append(_case(f"uniforms_kp_{dt}", 3, 1025, dt, t=0.25, k=20, p=0.9, uniforms=us))
        cs.append(_case(f"uniforms_equal_{dt}", 5, 67, dt, "equal", t=1.0, uniforms=us))
    # Philox: offset_dev, offset_add, rows; offset_dev + offset_add past 2^32 and below 0
    for i, (od, oa) in enumerate(((None, 0), (0, 0), (7, 0), (None, 12345), (100, 2 ** 32 - 50), (2 ** 31 - 1, 2 ** 31 + 9),
                                  (-1, 0), (-5, 2), (3, 2 ** 40 + 11))):
        cs.append(_case(f"philox_{i}", (1, 3, 33)[i % 3], 257, DTYPES[i % 3], t=1.0, k=30, p=0.9,
                        seed=(0x9E3779B97F4A7C15 * (i + 1)) & (2 ** 64 - 1), offset_dev=od, offset_add=oa))
    # the kernel loads 8 steps of 1024 elements at a time: one batch exactly, one element less, one more
    for i, v in enumerate((8 * THREADS - 1, 8 * THREADS, 8 * THREADS + 1)):
        cs.append(_case(f"batch{v}_k40_p0.9", 3, v, DTYPES[i], t=1.0, k=40, p=0.9, seed=v))
        cs.append(_case(f"batch{v}_draw", 1, v, DTYPES[(i + 1) % 3], t=0.25, seed=v + 1))
        cs.append(_case(f"batch{v}_greedy", 1, v, DTYPES[(i + 2) % 3], t=0.0))
    # one row each at 32000 and 128256
    for v in (32000, 128256):
        for dt in DTYPES:
            cs.append(_case(f"big{v}_{dt}_k50_p0.9", 1, v, dt, t=1.0, k=50, p=0.9, seed=v))
            cs.append(_case(f"big{v}_{dt}_draw", 1, v, dt, t=0.25, seed=v + 1))
        cs.append(_case(f"big{v}_bf16q_draw", 1, v, "bf16", "bf16q", t=0.25, seed=v + 2))
        cs.append(_case(f"big{v}_bf16q_k50_p0.5", 1, v, "bf16", "bf16q", t=1.0, k=50, p=0.5, seed=v + 3))
        cs.append(_case(f"big{v}_bf16q_greedy", 1, v, "bf16", "bf16q", t=0.0))
    return cs


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)
VOCABS = sorted({c.vocab for c in CASES})


def _check_straddle():
    """the tie cases cut inside their tie group: some, not all, of the tied tokens are kept"""
    for c in CASES:
        if c.kind not in ("tie_top", "tie_p") or c.temperature == 0 or c.top_k == 1:
            continue
        logits, u, _ = build(c)
        for r in range(c.rows):
            pick = oracle_row(logits[r], c.temperature, c.top_k, c.top_p, u[r])
            tied = np.nonzero(logits[r] == np.sort(logits[r])[::-1][1])[0]   # (both kinds tie the 2nd largest value)
            kept = np.intersect1d(tied, pick.k2).size
            assert tied.size >= 6 and 0 < kept < tied.size, (c.name, r, kept, tied.size)
            if c.kind == "tie_p":   # top-p, not top-k, made the cut: top-k alone keeps more of the group
                assert kept < np.intersect1d(tied, pick.k1).size, (c.name, r)


for _c in CASES:   # the input condition, every row of every case (build asserts it)
    build(_c)
_check_straddle()
