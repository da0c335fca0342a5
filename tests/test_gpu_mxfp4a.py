"""MXFP4 weights x fp8 activations (pli_gemm_mxfp4, linear_mxfp4a) on the device.

Outputs sit inside sentinel-filled buffers, padded leading dimensions hold NaN codes / 0xFF scale bytes in the padding,
pli_last_route is asserted in each case.  Tests 1-3 are bit for bit on data whose every partial sum is exact in fp32
in any order: the e2m1 lane map and nibble order, the scale byte per (row, block), the ends of the scale contract and
the 0xFF rule, on gemm_mxfp4_mx and (through a w4 view one byte into its buffer) on gemm_mxfp4_generic.  Test 4 holds
both routes to the float64 oracle over the dequantised operands, per element, with the two bounds of
tests/fp8a_cases.py: (a) LIN_TOL * (|ref| + 1) and (b) NORM_SLACK * u * |ref| + (K + 2) * 2^-23 * mag + MIN_NORMAL,
mag = (x_scale |X8|) |W|^T + |bias|.  Operands of test 4: x = N(0,1) * 0.5 through the CPU rule of quantize_rows_fp8,
w = N(0,1) * k^-0.5 with row j scaled by 2^((j % 9) - 4), through quantize_weight_mxfp4; "u" cases give every block
of a row the scale byte of its first block (one scale per row, gemm_fp8_mx's precedent for bound (b))."""
from __future__ import annotations

import functools
import os
import re

import numpy as np
import pytest
import torch

import fp8a_cases as fc
from conftest import PKG
from decode_step_cases import SENTINEL, TDT, Guarded, assert_untouched
from oracle.numerics import round_to_dtype, seeded_normal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MX, GENERIC = "gemm_mxfp4_mx", "gemm_mxfp4_generic"
E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])
_PLAN = open(os.path.join(PKG, "csrc", "mxfp4a_plan.h")).read()
KSTEP, STAGES = (int(re.search(r"constexpr int " + c + r" = (\d+);", _PLAN).group(1)) for c in ("kMxfp4aKStep", "kMxfp4aStages"))
TM, TN = fc.TM, fc.TN  # the tile is gemm_fp8_mx's


@pytest.fixture(scope="module")
def pli(built_lib):
    import pli_hip
    return pli_hip


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def pack(nib):
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)


def weight64(nib, exps):
    return E2M1[nib] * np.repeat(np.exp2(exps.astype(np.float64) - 127), 32, axis=1)


def dev_u8(a, fill, pad=0, col0=0, off1=False):
    """bytes [rows, w] on the device: contiguous, columns col0.. of a [rows, w + pad] matrix of `fill`, or a view that
    starts one byte into its buffer"""
    rows, w = a.shape
    t = torch.from_numpy(np.ascontiguousarray(a))
    if off1:
        buf = torch.full((rows * w + 1,), fill, dtype=torch.uint8, device=DEV)
        buf[1:] = t.reshape(-1).to(DEV)
        return buf[1:].view(rows, w)
    wide = torch.full((rows, w + pad), fill, dtype=torch.uint8)
    wide[:, col0:col0 + w] = t
    return wide.to(DEV)[:, col0:col0 + w]


def launch(pli, x8, xs, nib, exps, dt, kernel, bias=None, pad=False, off1=False, soff1=False):
    m, n = x8.shape[0], nib.shape[0]
    p = (lambda v: v) if pad else (lambda v: 0)
    g = Guarded((m, n), dt, DEV, strides=(n + p(8), 1))
    pli.gemm_mxfp4(dev_u8(x8, 0x7F, p(16)), None if xs is None else torch.from_numpy(xs).to(DEV),
                   dev_u8(pack(nib), 0xFF, p(48), p(16), off1), dev_u8(exps, 0xFF, p(8), p(4), soff1),
                   bias=None if bias is None else torch.from_numpy(bias).to(TDT[dt]).to(DEV), out=g.view,
                   out_dtype=TDT[dt])
    assert pli.last_route() == kernel
    torch.cuda.synchronize()
    assert_untouched(g, lambda v: v)
    return g.view.clone().cpu()


def assert_bitwise_on_both_routes(pli, x8, xs, nib, exps, want64, dt):
    """want64: float64, exact in fp32, so one rounding to T; NaN where the rule says NaN and nowhere else"""
    finite = want64[~np.isnan(want64)]
    assert np.array_equal(finite.astype(np.float32).astype(np.float64), finite)
    want, want_nan = torch.from_numpy(want64).to(TDT[dt]), torch.from_numpy(np.isnan(want64))
    got = {}
    for kernel in (MX, GENERIC):
        got[kernel] = launch(pli, x8, xs, nib, exps, dt, kernel, off1=kernel == GENERIC)
        assert torch.equal(torch.isnan(got[kernel]), want_nan), (kernel, "NaN exactly where the rule says")
        diff = (bits(got[kernel]) != bits(want)) & ~want_nan
        assert int(diff.sum()) == 0, (kernel, int(diff.sum()), diff.nonzero()[:8].tolist())
    return got[MX]


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("k", [KSTEP, 2 * KSTEP])
def test_lane_map_nibble_order_and_all_code_pairs_bitwise(pli, k, dt):
    """x8 row r = code r, w4 row j = nibble j everywhere, scale 2^0: C[r, j] = k * a * b with a * b of at most 6
    significant bits (subnormal e4m3 codes included); the NaN codes 0x7F / 0xFF poison exactly their rows"""
    x8 = np.repeat(np.arange(256, dtype=np.uint8)[:, None], k, axis=1)
    nib = np.repeat(np.arange(16, dtype=np.uint8)[:, None], k, axis=1)
    want64 = k * np.outer(fc.DECODE, E2M1) + 0.0  # the sum starts from +0
    assert int(np.isnan(want64).all(axis=1).sum()) == 2
    assert_bitwise_on_both_routes(pli, x8, None, nib, np.full((16, k // 32), 127, np.uint8), want64, dt)


@pytest.mark.parametrize("dt", fc.DTYPES)
def test_scale_byte_per_row_and_block_bitwise(pli, dt):
    m, n, k = 33, 128, 256
    r, j, i = np.arange(m)[:, None], np.arange(n)[:, None], np.arange(k)[None, :]
    xv = ((3 * r + 5 * i + (r * i) // 7) % 7) - 3
    nib = ((7 * j + 2 * i + (j * i) // 5 + 1) % 16).astype(np.uint8)
    exps = (127 + ((j + 3 * np.arange(k // 32)[None, :]) % 9 - 4)).astype(np.uint8)
    xd, wd = xv.astype(np.float64), weight64(nib, exps)
    # every term a multiple of 2^-5 and every partial sum below 2^17: 22 bits, exact in fp32 in any order
    assert np.array_equal(np.rint(wd * 32), wd * 32) and float((np.abs(xd) @ np.abs(wd).T).max()) < 2 ** 17
    assert len(np.unique(nib)) == 16 and len(np.unique(exps)) == 9
    assert_bitwise_on_both_routes(pli, fc.small_int_code(xv), None, nib, exps, xd @ wd.T + 0.0, dt)


@pytest.mark.parametrize("dt", fc.DTYPES)
def test_contract_ends_and_nan_scale_byte_bitwise(pli, dt):
    m, n, k = 17, 196, 128
    j = np.arange(n)
    nib, exps = np.zeros((n, k), np.uint8), np.full((n, k // 32), 127, np.uint8)
    nib[j, 32 * (j % 4) + j % 32] = 3                       # one code of 1.5 in block j % 4 ...
    exps[j, j % 4] = 31 + j % 193                           # ... at every scale from 2^-96 to 2^96
    x8 = np.full((m, k), 0x38, np.uint8)                    # 1.0
    want64 = np.repeat((1.5 * np.exp2(exps[j, j % 4].astype(np.float64) - 127))[None, :], m, axis=0)
    before = assert_bitwise_on_both_routes(pli, x8, None, nib, exps, want64, dt)
    exps[77, 2] = 0xFF                                      # a block of zero codes: the whole column, nothing else
    want64[:, 77] = np.nan
    after = assert_bitwise_on_both_routes(pli, x8, None, nib, exps, want64, dt)
    keep = j != 77
    assert torch.equal(bits(after[:, keep]), bits(before[:, keep]))


# ---- 4. the f64 oracle per element -------------------------------------------------------------------
def _cases():
    S, out = STAGES, []
    mx = [(17, 4, 1), (17, 128, S), (17, 132, 32), (127, 124, 1), (127, 132, S + 1), (127, 128, 32), (128, 128, 1),
          (128, 128, S), (128, 4, S + 1), (128, 124, S), (129, 128, 1), (129, 132, S), (129, 124, 32), (259, 132, S + 1),
          (259, 128, 1), (259, 4, S), (259, 3 * 128 + 4, S), ((8 + 1) * 128 + 5, 132, 1)]
    for idx, (m, n, steps) in enumerate(mx):
        out.append((m, n, steps * KSTEP, MX, "u" if idx % 3 == 0 else ""))
    out += [(129, 132, KSTEP * (S + 1), MX, "bias,pad"), (17, 124, KSTEP * S, MX, "bias,noxs,u"),
            (259, 128, KSTEP, MX, "noxs,pad"), (128, 132, KSTEP * S, MX, "bias,u,pad"),
            (17, 6, 96, GENERIC, "bias"), (17, 24, 96, GENERIC, "pad,noxs"), (16, 128, KSTEP, GENERIC, ""),
            (17, 128, KSTEP, GENERIC, "soff1,u"), (33, 128, KSTEP, GENERIC, "off1,bias")]
    return out


@functools.lru_cache(maxsize=None)
def case_operands(case, dt):
    import pli_hip
    m, n, k, _, flags = case
    seed = 52000 + 7 * m + 13 * n + k + 500 * (dt == "fp16") + 1000 * len(flags)
    x = torch.from_numpy(round_to_dtype(seeded_normal((m, k), seed) * np.float32(0.5), dt))
    if "noxs" in flags:  # NULL x_scale: the codes of 4 x at scale one
        x8, xs = pli_hip.quantize_weight_fp8(x * 4.0, scale=torch.ones(m))[0].view(torch.uint8).numpy(), None
    else:
        c8, s = pli_hip.quantize_rows_fp8(x.to(TDT[dt]))
        x8, xs = c8.view(torch.uint8).numpy(), s.numpy()
    w = seeded_normal((n, k), seed + 1) * np.float32(k ** -0.5) * np.exp2(np.arange(n) % 9 - 4.0)[:, None].astype(np.float32)
    codes, exps = (t.numpy() for t in pli_hip.quantize_weight_mxfp4(torch.from_numpy(w)))
    if "u" in flags.split(","):
        exps = np.repeat(exps[:, :1], k // 32, axis=1)
    nib = np.stack((codes & 15, codes >> 4), axis=2).reshape(n, k)
    bias = round_to_dtype(seeded_normal((n,), seed + 2), dt) if "bias" in flags else None
    xd, wd = fc.DECODE[x8] * (1.0 if xs is None else xs.astype(np.float64)[:, None]), weight64(nib, exps)
    b64 = 0.0 if bias is None else bias.astype(np.float64)
    ref = fc.Reference(xd @ wd.T + b64, (k + 2) * 2.0 ** -23 * (np.abs(xd) @ np.abs(wd).T + np.abs(b64)), k)
    return x8, xs, nib, exps, bias, ref


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("case", _cases(), ids=lambda c: "m{}n{}k{}-{}".format(*c[:3], c[4]))
def test_gemm_against_f64_oracle(pli, case, dt):
    x8, xs, nib, exps, bias, ref = case_operands(case, dt)
    flags = case[4].split(",")
    got = launch(pli, x8, xs, nib, exps, dt, case[3], bias=bias, pad="pad" in flags, off1="off1" in flags,
                 soff1="soff1" in flags)
    ra, rb = fc.ratios(got.double().numpy(), ref, dt)
    print(f"{case} {dt}: err / (a) {ra:.3f}, err / (b) {rb:.3f}")
    assert ra <= 1.0 and rb <= 1.0, (case, dt, ra, rb)


# ---- 5. empty shapes, capture ------------------------------------------------------------------------
def test_k0_and_empty(pli):
    x8 = torch.zeros(19, 0, dtype=torch.uint8, device=DEV)
    codes, exps = torch.zeros(8, 0, dtype=torch.uint8, device=DEV), torch.zeros(8, 0, dtype=torch.uint8, device=DEV)
    bias = torch.arange(8, dtype=torch.bfloat16, device=DEV)
    out = torch.full((19, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    pli.gemm_mxfp4(x8, None, codes, exps, out=out)
    assert pli.last_route() == GENERIC and bool((out == 0).all())
    pli.gemm_mxfp4(x8, None, codes, exps, bias=bias, out=out)
    assert torch.equal(out, bias.expand(19, 8))
    assert tuple(pli.gemm_mxfp4(x8[:0], None, codes, exps).shape) == (0, 8) and pli.last_route() == ""


def test_graph_replays_after_in_place_changes(pli):
    case = (TM + 1, TN + 4, KSTEP * (STAGES + 1), MX, "")
    x8, xs, nib, exps, _, _ = case_operands(case, "bf16")
    x8, xs = torch.from_numpy(x8.copy()).to(DEV), torch.from_numpy(xs.copy()).to(DEV)
    codes, exps = torch.from_numpy(pack(nib)).to(DEV), torch.from_numpy(exps.copy()).to(DEV)
    out = torch.empty(case[0], case[1], dtype=torch.bfloat16, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pli.gemm_mxfp4(x8, xs, codes, exps, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pli.gemm_mxfp4(x8, xs, codes, exps, out=out)
    assert pli.last_route() == MX
    seen = []
    for change in (False, True, True):  # several replays, each against the eager call on the same operands
        if change:
            exps[5, 1] += 3
            codes[7].copy_(torch.roll(codes[7], 1))
        g.replay()
        torch.cuda.synchronize()
        seen.append(out.clone())
        assert torch.equal(bits(seen[-1]), bits(pli.gemm_mxfp4(x8, xs, codes, exps)))
    assert not torch.equal(bits(seen[0]), bits(seen[1])) and not torch.equal(bits(seen[1]), bits(seen[2]))


# ---- 6. linear_mxfp4a is the two calls ---------------------------------------------------------------
@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("m,n,k,kernel", [(TM + 1, TN, 2 * KSTEP, MX), (17, 24, 96, GENERIC)])
def test_linear_mxfp4a_is_quantise_then_gemm(pli, m, n, k, kernel, dt):
    tdt = TDT[dt]
    x = torch.from_numpy(seeded_normal((m, k), 54000 + k, dt)).to(tdt).to(DEV)
    codes, exps = (t.to(DEV) for t in pli.quantize_weight_mxfp4(torch.from_numpy(seeded_normal((n, k), 54001 + k, "fp32"))))
    bias = torch.from_numpy(seeded_normal((n,), 54002, dt)).to(tdt).to(DEV)
    got = pli.linear_mxfp4a(x, codes, exps, bias=bias)
    assert pli.last_route() == kernel and got.dtype == tdt
    x8, xs = pli.quantize_rows_fp8(x)
    assert torch.equal(bits(got), bits(pli.gemm_mxfp4(x8, xs, codes, exps, bias=bias, out_dtype=tdt)))
