"""MXFP4 activations x MXFP4 weights (pli_quantize_rows_mxfp4, pli_gemm_mxfp4_a4, linear_mxfp4a4) on the device.

Outputs sit inside sentinel-filled buffers, padded leading dimensions hold 0xFF bytes, pli_last_route is asserted in
each case.  Test 1: the quantiser byte for byte against its CPU mirror.  Tests 2-4: bit for bit on data whose every
partial sum is exact in fp32 in any order, on gemm_mxfp4_a4_mx and (through a w4 view one byte into its buffer) on
gemm_mxfp4_a4_generic.  Test 5: the float64 oracle over the dequantised operands, per element, with the two bounds of
tests/fp8a_cases.py, mag = |X| |W|^T + |bias|; x = N(0,1) * 0.5 through the CPU rule of quantize_rows_mxfp4, w =
N(0,1) * k^-0.5 with row j scaled by 2^((j % 9) - 4) through quantize_weight_mxfp4."""
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
MX, GENERIC, QUANT = "gemm_mxfp4_a4_mx", "gemm_mxfp4_a4_generic", "quant_rows_mxfp4"
E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])
_PLAN = open(os.path.join(PKG, "csrc", "mxfp4x_plan.h")).read()
KSTEP, STAGES = (int(re.search(r"constexpr int " + c + r" = (\d+);", _PLAN).group(1)) for c in ("kMxfp4xKStep", "kMxfp4xStages"))


@pytest.fixture(scope="module")
def pli(built_lib):
    import pli_hip
    return pli_hip


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def pack(nib):
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)


def value64(nib, exps):
    return E2M1[nib] * np.repeat(np.exp2(exps.astype(np.float64) - 127), 32, axis=1)


def dev_u8(a, fill=0xFF, pad=0, col0=0, off1=False):  # as test_gpu_mxfp4a.py's
    rows, w = a.shape
    t = torch.from_numpy(np.ascontiguousarray(a))
    if off1:
        buf = torch.full((rows * w + 1,), fill, dtype=torch.uint8, device=DEV)
        buf[1:] = t.reshape(-1).to(DEV)
        return buf[1:].view(rows, w)
    wide = torch.full((rows, w + pad), fill, dtype=torch.uint8)
    wide[:, col0:col0 + w] = t
    return wide.to(DEV)[:, col0:col0 + w]


def launch(pli, xnib, xexp, xs, wnib, wexp, dt, kernel, bias=None, pad=False, off1=False):
    m, n = xnib.shape[0], wnib.shape[0]
    p = (lambda v: v) if pad else (lambda v: 0)
    g = Guarded((m, n), dt, DEV, strides=(n + p(8), 1))
    pli.gemm_mxfp4_a4(dev_u8(pack(xnib), pad=p(32), col0=p(16)), dev_u8(xexp, pad=p(12), col0=p(8)),
                      None if xs is None else torch.from_numpy(xs).to(DEV),
                      dev_u8(pack(wnib), pad=p(48), col0=p(16), off1=off1), dev_u8(wexp, pad=p(8), col0=p(4)),
                      bias=None if bias is None else torch.from_numpy(bias).to(TDT[dt]).to(DEV), out=g.view,
                      out_dtype=TDT[dt])
    assert pli.last_route() == kernel
    torch.cuda.synchronize()
    assert_untouched(g, lambda v: v)
    return g.view.clone().cpu()


def assert_bitwise_on_both_routes(pli, xnib, xexp, wnib, wexp, want64, dt):
    finite = want64[~np.isnan(want64)]
    assert np.array_equal(finite.astype(np.float32).astype(np.float64), finite)
    want, want_nan = torch.from_numpy(want64).to(TDT[dt]), torch.from_numpy(np.isnan(want64))
    got = {}
    for kernel in (MX, GENERIC):
        got[kernel] = launch(pli, xnib, xexp, None, wnib, wexp, dt, kernel, off1=kernel == GENERIC)
        assert torch.equal(torch.isnan(got[kernel]), want_nan), (kernel, "NaN exactly where the rule says")
        diff = (bits(got[kernel]) != bits(want)) & ~want_nan
        assert int(diff.sum()) == 0, (kernel, int(diff.sum()), diff.nonzero()[:8].tolist(), got[kernel][diff][:8].tolist())
    return got[MX]


def quant_rows(m, k, dt):
    x = torch.from_numpy(seeded_normal((m, k), 61000 + m + k)) * torch.exp2(torch.arange(k // 32).float() % 11 - 5
                                                                             ).repeat_interleave(32)[None, :]
    ties = torch.tensor([.25, .75, 1.25, 1.75, 2.5, 3.5, 5., 6., -.25, -.75, -1.25, -1.75, -2.5, -3.5, -5., -6.])
    x[0, :16] = ties
    x[0, 16:64] = 0.0
    if k >= 96:
        x[1, 40], x[1, 41], x[1, 70] = float("inf"), float("-inf"), float("nan")
        x[2] = 0.0
        x[m - 1, k - 1] = float("nan")
    return x.to(TDT[dt])


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("m,k,mode", [(1, 32, ""), (3, 256, ""), (17, 8192 + 32, ""), (5, 96, "pad"), (5, 96, "off1")])
def test_quantiser_bitwise_against_cpu_mirror(pli, m, k, mode, dt):
    x = quant_rows(m, k, dt)
    want = pli.quantize_rows_mxfp4(x)
    if mode == "off1":  # the source one element into its buffer: the scalar class
        buf = torch.full((m * k + 1,), float("nan"), dtype=x.dtype, device=DEV)
        buf[1:] = x.reshape(-1).to(DEV)
        xd = buf[1:].view(m, k)
    else:
        pad = 8 if mode == "pad" else 0
        wide = torch.full((m, k + pad), float("nan"), dtype=x.dtype, device=DEV)
        wide[:, :k] = x.to(DEV)
        xd = wide[:, :k]
    guard = 64
    bufs = [torch.full((m + 2, (w + 2 * guard + 3) // 4 * 4), 0xA5, dtype=torch.uint8, device=DEV)  # ld % 4 == 0
            for w in (k // 2, k // 32)]
    sbuf = torch.full((m + 2 * guard,), SENTINEL, dtype=torch.float32, device=DEV)
    outs = (bufs[0][1:m + 1, guard:guard + k // 2], bufs[1][1:m + 1, guard:guard + k // 32], sbuf[guard:guard + m])
    got = pli.quantize_rows_mxfp4(xd, out=outs)
    assert pli.last_route() == QUANT
    torch.cuda.synchronize()
    for name, g, w in zip(("codes", "exps", "scale"), got, want):
        assert torch.equal(g.cpu().contiguous().view(torch.uint8), w.view(torch.uint8)), name
    for b, o in zip(bufs, outs):  # nothing outside the addressed bytes
        keep = torch.ones_like(b, dtype=torch.bool)
        keep[1:m + 1, guard:guard + o.shape[1]] = False
        assert bool((b[keep] == 0xA5).all())
    assert bool((sbuf[:guard] == SENTINEL).all()) and bool((sbuf[guard + m:] == SENTINEL).all())


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("k", [KSTEP, 2 * KSTEP])
def test_lane_map_nibble_order_and_all_code_pairs_bitwise(pli, k, dt):
    xnib = np.repeat((np.arange(32, dtype=np.uint8) % 16)[:, None], k, axis=1)
    wnib = np.repeat(np.arange(16, dtype=np.uint8)[:, None], k, axis=1)
    ones = lambda rows: np.full((rows, k // 32), 127, np.uint8)
    want64 = k * np.outer(E2M1[xnib[:, 0]], E2M1) + 0.0  # the sum starts from +0
    assert_bitwise_on_both_routes(pli, xnib, ones(32), wnib, ones(16), want64, dt)


@pytest.mark.parametrize("dt", fc.DTYPES)
def test_position_and_scale_bytes_per_row_and_block_bitwise(pli, dt):
    m, n, k = 33, 132, 2 * KSTEP
    r, j, i, b = np.arange(m)[:, None], np.arange(n)[:, None], np.arange(k)[None, :], np.arange(k // 32)[None, :]
    xnib = ((3 * r + 5 * i + (r * i) // 7) % 16).astype(np.uint8)
    wnib = ((7 * j + 2 * i + (j * i) // 5 + 1) % 16).astype(np.uint8)
    xexp = (127 - (2 * r + b + (r * b) // 3) % 3).astype(np.uint8)
    wexp = (127 + ((j + 3 * b) % 5 - 2)).astype(np.uint8)
    xd, wd = value64(xnib, xexp), value64(wnib, wexp)
    # every term a multiple of 2^-6 and every partial sum below 2^18: 24 bits, exact in fp32 in any order
    assert np.array_equal(np.rint(xd * 8), xd * 8) and np.array_equal(np.rint(wd * 8), wd * 8)
    assert float((np.abs(xd) @ np.abs(wd).T).max()) < 2 ** 18
    assert len(np.unique(xnib)) == 16 and len(np.unique(wnib)) == 16 and len(np.unique(xexp)) == 3 and len(np.unique(wexp)) == 5
    assert_bitwise_on_both_routes(pli, xnib, xexp, wnib, wexp, xd @ wd.T + 0.0, dt)


@pytest.mark.parametrize("dt", fc.DTYPES)
def test_contract_ends_and_nan_scale_bytes_bitwise(pli, dt):
    XLO, XHI = pli.MXFP4X_EXP_RANGE
    span, k, n = XHI - XLO + 1, KSTEP, 8
    m = 2 * span
    r, j = np.arange(m), np.arange(n)
    xnib, xexp = np.zeros((m, k), np.uint8), np.full((m, k // 32), 127, np.uint8)
    xnib[r, 32 * (r % 8) + r % 32] = np.where(r < span, 1, 15)  # 0.5 / -6, one code per row, in block r % 8
    xexp[r, r % 8] = 127 + XLO + r % span
    wnib = np.repeat(np.where(j % 2 == 0, 1, 7).astype(np.uint8)[:, None], k, axis=1)
    wexp = np.repeat(np.where(j % 4 < 2, 127 - 96, 127 + 96).astype(np.uint8)[:, None], k // 32, axis=1)
    want64 = value64(xnib, xexp) @ value64(wnib, wexp).T + 0.0
    assert np.abs(want64).min() == 2.0 ** -124 and np.abs(want64).max() == 36 * 2.0 ** 122
    before = assert_bitwise_on_both_routes(pli, xnib, xexp, wnib, wexp, want64, dt)
    xexp[40, 3], wexp[5, 6] = 0xFF, 0xFF  # 40 % 8 == 0: a block of zero codes on the X side
    want64[40, :], want64[:, 5] = np.nan, np.nan
    after = assert_bitwise_on_both_routes(pli, xnib, xexp, wnib, wexp, want64, dt)
    keep = torch.from_numpy(~np.isnan(want64))
    assert torch.equal(bits(after)[keep], bits(before)[keep])


def _cases():
    S = STAGES
    mx = [(17, 4, 1), (17, 128, S), (17, 132, 32), (128, 128, 1), (128, 4, S + 1), (128, 132, S), (129, 128, S + 1),
          (129, 132, 1), (129, 4, 32), (259, 132, S + 1), (259, 128, 32), (259, 4, S)]
    out = [(m, n, steps * KSTEP, MX, "") for m, n, steps in mx]
    out += [(129, 132, KSTEP * (S + 1), MX, "bias,pad"), (17, 128, KSTEP * S, MX, "bias,noxs"),
            (259, 128, KSTEP, MX, "noxs,pad"), (17, 24, 96, GENERIC, "bias"), (16, 128, KSTEP, GENERIC, ""),
            (33, 128, KSTEP, GENERIC, "off1,bias")]
    return out


@functools.lru_cache(maxsize=None)
def case_operands(case, dt):
    import pli_hip
    m, n, k, _, flags = case
    seed = 62000 + 7 * m + 13 * n + k + 500 * (dt == "fp16") + 1000 * len(flags)
    x = torch.from_numpy(round_to_dtype(seeded_normal((m, k), seed) * np.float32(0.5), dt)).to(TDT[dt])
    codes, xexp, xs = (t.numpy() for t in pli_hip.quantize_rows_mxfp4(x))
    if "noxs" in flags:  # NULL x_scale: plain MXFP4, the row exponent folded into the block bytes
        xexp, xs = (xexp.astype(np.int64) + np.frexp(xs)[1][:, None] - 1).astype(np.uint8), None
    w = seeded_normal((n, k), seed + 1) * np.float32(k ** -0.5) * np.exp2(np.arange(n) % 9 - 4.0)[:, None].astype(np.float32)
    wcodes, wexp = (t.numpy() for t in pli_hip.quantize_weight_mxfp4(torch.from_numpy(w)))
    xnib, wnib = (np.stack((c & 15, c >> 4), axis=2).reshape(c.shape[0], -1) for c in (codes, wcodes))
    bias = round_to_dtype(seeded_normal((n,), seed + 2), dt) if "bias" in flags else None
    xd = value64(xnib, xexp) * (1.0 if xs is None else xs.astype(np.float64)[:, None])
    wd, b64 = value64(wnib, wexp), 0.0 if bias is None else bias.astype(np.float64)
    ref = fc.Reference(xd @ wd.T + b64, (k + 2) * 2.0 ** -23 * (np.abs(xd) @ np.abs(wd).T + np.abs(b64)), k)
    return xnib, xexp, xs, wnib, wexp, bias, ref


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("case", _cases(), ids=lambda c: "m{}n{}k{}-{}".format(*c[:3], c[4]))
def test_gemm_against_f64_oracle(pli, case, dt):
    xnib, xexp, xs, wnib, wexp, bias, ref = case_operands(case, dt)
    flags = case[4].split(",")
    got = launch(pli, xnib, xexp, xs, wnib, wexp, dt, case[3], bias=bias, pad="pad" in flags, off1="off1" in flags)
    ra, rb = fc.ratios(got.double().numpy(), ref, dt)
    print(f"{case} {dt}: err / (a) {ra:.3f}, err / (b) {rb:.3f}")
    assert ra <= 1.0 and rb <= 1.0, (case, dt, ra, rb)


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("m,n,k,kernel", [(fc.TM + 1, fc.TN, 2 * KSTEP, MX), (17, 24, 96, GENERIC)])
def test_linear_mxfp4a4_is_quantise_then_gemm(pli, m, n, k, kernel, dt):
    tdt = TDT[dt]
    x = torch.from_numpy(seeded_normal((m, k), 64000 + k, dt)).to(tdt).to(DEV)
    codes, exps = (t.to(DEV) for t in pli.quantize_weight_mxfp4(torch.from_numpy(seeded_normal((n, k), 64001 + k, "fp32"))))
    bias = torch.from_numpy(seeded_normal((n,), 64002, dt)).to(tdt).to(DEV)
    got = pli.linear_mxfp4a4(x, codes, exps, bias=bias)
    assert pli.last_route() == kernel and got.dtype == tdt
    x4, xe, xs = pli.quantize_rows_mxfp4(x)
    assert torch.equal(bits(got), bits(pli.gemm_mxfp4_a4(x4, xe, xs, codes, exps, bias=bias, out_dtype=tdt)))


def test_graph_replays_after_in_place_changes(pli):
    case = (fc.TM + 1, fc.TN + 4, KSTEP * (STAGES + 1), MX, "")
    xnib, xexp, xs, wnib, wexp, _, _ = case_operands(case, "bf16")
    x4, xe, xs = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (pack(xnib), xexp, xs))
    codes, exps = torch.from_numpy(pack(wnib)).to(DEV), torch.from_numpy(wexp.copy()).to(DEV)
    out = torch.empty(case[0], case[1], dtype=torch.bfloat16, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pli.gemm_mxfp4_a4(x4, xe, xs, codes, exps, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pli.gemm_mxfp4_a4(x4, xe, xs, codes, exps, out=out)
    assert pli.last_route() == MX
    seen = []
    for change in (False, True, True):  # several replays, each against the eager call on the same operands
        if change:
            exps[5, 1] += 3
            xe[9, 2] -= 1
            x4[7].copy_(torch.roll(x4[7], 1))
        g.replay()
        torch.cuda.synchronize()
        seen.append(out.clone())
        assert torch.equal(bits(seen[-1]), bits(pli.gemm_mxfp4_a4(x4, xe, xs, codes, exps)))
    assert not torch.equal(bits(seen[0]), bits(seen[1])) and not torch.equal(bits(seen[1]), bits(seen[2]))


def test_k0_and_empty(pli):
    z = lambda rows: torch.zeros(rows, 0, dtype=torch.uint8, device=DEV)
    bias = torch.arange(8, dtype=torch.bfloat16, device=DEV)
    out = torch.full((19, 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    pli.gemm_mxfp4_a4(z(19), z(19), None, z(8), z(8), out=out)
    assert pli.last_route() == GENERIC and bool((out == 0).all())
    pli.gemm_mxfp4_a4(z(19), z(19), None, z(8), z(8), bias=bias, out=out)
    assert torch.equal(out, bias.expand(19, 8))
    assert tuple(pli.gemm_mxfp4_a4(z(0), z(0), None, z(8), z(8)).shape) == (0, 8) and pli.last_route() == ""
    c, e, s = pli.quantize_rows_mxfp4(torch.zeros(3, 0, dtype=torch.bfloat16, device=DEV))
    assert tuple(c.shape) == tuple(e.shape) == (3, 0) and bool((s == 1).all())
