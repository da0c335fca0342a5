"""The sampling kernel's arithmetic, emulated in numpy on the CPU, against the
float64 oracle over the whole case list; and the oracle's own draw statistics.

`emulate_row` follows csrc/sample.hip pass by pass with the numbers the kernel
uses: integer keys (restated here, not imported from the package), the row
maximum as a key, 8-bit digit histograms from the top for the top-k cut (counts)
and the top-p cut (weights), weights exp((x - m) / temperature) in float32 turned
into floor(w * 2^45) integers, the two thresholds as one float64 product and a
floor, tie ranks by index, an integer running sum for the draw.  Every sum is
an integer sum, so the kernel's reduction shape (LDS atomics, wave shuffles,
serial loops) cannot change a result and is not modelled.  What differs
between this emulation and the device is the last bits of exp alone, which
the input condition of tests/sample_cases.py (2 * DELTA) covers.

That the emulation picks the oracle's token on EVERY row of EVERY case shows,
without a GPU, that the condition leaves no row undecided.
"""
from __future__ import annotations

import numpy as np
import pytest

import sample_cases as sc

ONE = 1 << sc.FRAC_BITS


def keys_of(x: np.ndarray, dtype: str) -> np.ndarray:
    """order-preserving integer keys of float32 values representable in dtype (NaN -> -inf's key, -0 -> +0's)"""
    if dtype == "fp32":
        b = x.astype(np.float32).view(np.uint32).astype(np.uint64)
        sign, full, ninf, absmask, inf = 0x80000000, 0xFFFFFFFF, 0xFF800000, 0x7FFFFFFF, 0x7F800000
    else:
        if dtype == "fp16":
            b = x.astype(np.float16).view(np.uint16).astype(np.uint64)
            inf = 0x7C00
        else:
            b = (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint64)
            inf = 0x7F80
        sign, full, absmask = 0x8000, 0xFFFF, 0x7FFF
        ninf = sign | inf
    b = np.where((b & np.uint64(absmask)) > np.uint64(inf), np.uint64(ninf), b)
    b = np.where(b == np.uint64(sign), np.uint64(0), b)
    return np.where(b & np.uint64(sign) != 0, ~b & np.uint64(full), b | np.uint64(sign)).astype(np.uint64)


def radix_select(keys, values, q, passes):
    """largest key t with sum{values : key >= t} > q, walking 8-bit digits from the top; returns (t, q left)"""
    prefix = 0
    for p in range(passes):
        shift = 8 * (passes - 1 - p)
        match = (keys >> np.uint64(shift + 8)) == np.uint64(prefix) if p else np.ones(keys.size, dtype=bool)
        hist = [0] * 256
        for d, v in zip(((keys[match] >> np.uint64(shift)) & np.uint64(255)).tolist(), values[match].tolist()):
            hist[d] += v
        run, digit = 0, None
        for d in range(255, -1, -1):
            if run + hist[d] > q:
                digit = d
                break
            run += hist[d]
        if digit is None:
            digit, run = 0, run - hist[0]
        prefix, q = (prefix << 8) | digit, q - run
    return prefix, q


def emulate_row(x, dtype, temperature, top_k, top_p, u) -> int:
    t, p, u = np.float32(temperature), np.float32(top_p), np.float32(u)
    V = x.size
    keys = keys_of(x, dtype)
    passes = 4 if dtype == "fp32" else 2
    neg_inf = int(keys_of(np.array([-np.inf], dtype=np.float32), dtype)[0])
    pos_inf = int(keys_of(np.array([np.inf], dtype=np.float32), dtype)[0])
    maxkey = int(keys.max())
    if maxkey == neg_inf:
        return -1
    if t == 0:
        return int(np.nonzero(keys == np.uint64(maxkey))[0][0])
    # canonical values back from the data (NaN -> -inf, -0 -> +0), float32 arithmetic from here
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xc = np.where(np.isnan(x), np.float32(-np.inf), x).astype(np.float32) + np.float32(0.0)
        if maxkey == pos_inf:
            w = (keys == np.uint64(maxkey)).astype(np.float32)
        else:
            w = np.exp(((xc - xc.max()) / t).astype(np.float32)).astype(np.float32)
            w[xc == -np.inf] = 0.0
    wfx = np.floor(w.astype(np.float64) * float(ONE)).astype(np.uint64)   # (w * 2^45 is exact in fp32 and in fp64)
    ALL = 1 << 40
    keep_all = top_k <= 0 or top_k >= V
    t1, need1 = 0, ALL
    if not keep_all:
        t1, left = radix_select(keys, np.ones(V, dtype=np.uint64), top_k - 1, passes)
        need1 = left + 1
    tc, n_eq = t1, need1
    if p < 1:
        above = keys > np.uint64(t1)
        w_t1 = int(wfx[keys == np.uint64(t1)][0]) if not keep_all else 0
        tie_add = need1 * w_t1 if not keep_all else 0
        s1 = int(wfx[above].sum()) + tie_add
        limit = int(float(p) * float(s1))
        k, v = keys[above], wfx[above]
        if tie_add:   # the kept ties at t1 enter their bucket as one value
            k, v = np.append(k, np.uint64(t1)), np.append(v, np.uint64(tie_add))
        tc, left = radix_select(k, v, limit, passes)
        at = wfx[keys == np.uint64(tc)]
        wc = int(at[0]) if at.size else 0
        n_p = ALL if wc == 0 else left // wc + 1
        lim = need1 if (not keep_all and tc == t1) else ALL
        n_eq = min(n_p, lim)
    eq = keys == np.uint64(tc)
    rank = np.cumsum(eq) - 1
    contrib = np.where(keys > np.uint64(tc), wfx, np.where(eq & (rank < n_eq), wfx, np.uint64(0))).astype(np.uint64)
    run = np.cumsum(contrib)
    target = int(float(u) * float(int(run[-1])))
    return int(np.nonzero(run > np.uint64(target))[0][0])


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_emulation_picks_the_oracle_token_on_every_row(case):
    logits, u, want = sc.build(case)
    got = [emulate_row(logits[r], case.dtype, case.temperature, case.top_k, case.top_p, u[r]) for r in range(case.rows)]
    assert got == want.tolist(), case


def test_case_list_covers_what_the_kernel_can_get_wrong():
    cs = sc.CASES
    assert {1, 2, 63, 64, 65, 255, 256, 257, sc.THREADS - 1, sc.THREADS, sc.THREADS + 1, 8 * sc.THREADS - 1,
            8 * sc.THREADS, 8 * sc.THREADS + 1, 32000, 128256} <= set(sc.VOCABS)
    assert {c.rows for c in cs} >= {1, 3, 33} and {c.dtype for c in cs} == set(sc.DTYPES)
    assert {c.temperature for c in cs} >= {0.0, 0.25, 1.0, 4.0}
    assert {c.top_p for c in cs} >= {0.0, 0.1, 0.5, 0.9, 0.999, 1.0}
    for v in (1025, 257, 50):
        ks = {c.top_k for c in cs if c.vocab == v}
        assert ks >= {1, 2, 7, 50, v - 1, v, v + 5, 0}, v
        assert {(c.top_k, c.top_p) for c in cs if c.vocab == v} >= {(k, p) for k in (2, 7, 0) for p in (0.1, 0.5, 0.9)}
    assert {c.kind for c in cs} >= {"equal", "bf16q", "tie_top", "tie_p", "zeros", "special", "none", "inf1", "infs"}
    assert any(c.kind == "bf16q" and c.vocab == 32000 for c in cs)
    us = {float(v) for c in cs if c.uniforms for v in c.uniforms}
    assert 0.0 in us and float(sc.U_MAX) in us and float(sc.U_MAX) < 1.0 and np.nextafter(sc.U_MAX, np.float32(2)) == 1
    offs = [(c.offset_dev or 0) + c.offset_add for c in cs if c.uniforms is None]
    assert any(o >= 2 ** 32 for o in offs) and any(o < 0 for o in offs) and any(c.offset_dev for c in cs)
    # -1 rows, rows with +inf, rows with -0 / NaN really occur in the built inputs
    built = {c.kind: sc.build(c) for c in cs if c.dtype == "fp32" and c.temperature == 1.0 and c.top_k == 0}
    assert (built["none"][2] == -1).all() and np.isinf(built["infs"][0]).sum() >= 3 * 5
    assert np.signbit(built["zeros"][0][built["zeros"][0] == 0]).any() and np.isnan(built["special"][0]).any()


def test_oracle_draw_frequencies_over_philox():
    """2^16 draws (rows 0 .. 2^16 - 1 of one seed and offset) from a fixed 16-token distribution: every token's
    frequency within 5 sqrt(p (1 - p) / N) of p.  The u sequence is fixed, so this is deterministic."""
    N = 1 << 16
    x = (np.random.RandomState(5).standard_normal(16) * 1.5).astype(np.float32)
    w = np.exp(x.astype(np.float64) - x.astype(np.float64).max())
    prob = w / w.sum()
    u = sc.philox_u(0x0123456789ABCDEF, 17, np.arange(N)).astype(np.float64)
    c = np.cumsum(w)
    tokens = np.searchsorted(c, u * c[-1], side="right")     # the first token whose running sum exceeds u * S
    for r in (0, 1, 2, 777, N - 1):                          # (the same rule, through the oracle's own code)
        assert sc.oracle_row(x, 1.0, 0, 1.0, u[r]).token == tokens[r]
    freq = np.bincount(tokens, minlength=16) / N
    bound = 5 * np.sqrt(prob * (1 - prob) / N)
    assert (np.abs(freq - prob) <= bound).all(), (freq - prob) / bound
    assert 0.0 <= u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 5 / np.sqrt(12 * N)
