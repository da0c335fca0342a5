"""The split-K block-scaled GEMM for 17 .. 256 rows (pli_gemm_fp8_ws / pli_gemm_mxfp4_ws through gemm_fp8 / gemm_mxfp4
with workspace=) on the device, both weight formats, bf16 and fp16.

Outputs and the workspace sit inside sentinel-filled buffers (the workspace is exactly the reported size, so a byte
past it is a guard byte); pli_last_route is asserted in every case.  Tests 1 and 3 are bit for bit on data whose every
partial sum is exact in fp32 in any order (tests/fp8a_cases.py's asymmetric codes; the (row, block) scale pattern of
tests/test_gpu_mxfp4a.py).  Test 2 holds the route to the float64 oracle per element with both bounds of
tests/fp8a_cases.py as they stand: a split sum is one more order of the same K exact products, which the
(K + 2) * 2^-23 * mag term of bound (b) covers."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import fp8a_cases as fc
from decode_step_cases import TDT, Guarded, assert_untouched
from test_gpu_mxfp4a import DEV, bits, case_operands, dev_u8, pack, weight64

pytestmark = pytest.mark.gpu
SPLIT = "gemm_mx_splitk+gemm_mx_splitk_reduce"
PLAIN = {"fp8": "gemm_fp8_mx", "mxfp4": "gemm_mxfp4_mx"}
FMTS = ("fp8", "mxfp4")


@pytest.fixture(scope="module")
def pli(built_lib):
    import pli_hip
    return pli_hip


def put(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def weights(fmt, w, pad=False):
    """device weight operands: fp8 (codes [n, k], scale [n] or None), mxfp4 (nibbles [n, k], scale bytes [n, k / 32])"""
    p = (lambda v: v) if pad else (lambda v: 0)
    if fmt == "fp8":
        return dev_u8(w[0], 0x7F, p(48)), put(w[1])
    return dev_u8(pack(w[0]), 0xFF, p(48), p(16)), dev_u8(w[1], 0xFF, p(8), p(4))


def run(pli, fmt, x8, xs, w, dt, splits=0, bias=None, pad=False, ws="exact", route=SPLIT):
    """one call on fresh device operands into guarded buffers; ws: "exact" (the reported size), "short" (one byte
    less), None"""
    m, n, k = x8.shape[0], w[0].shape[0], x8.shape[1]
    g = Guarded((m, n), dt, DEV, strides=(n + (8 if pad else 0), 1))
    need = getattr(pli, f"gemm_{fmt}_workspace_bytes")(m, n, k, splits)
    gw = Guarded((max(need // 4, 4),), "fp32", DEV)
    work = {None: None, "exact": gw.view, "short": gw.view.view(torch.uint8)[:need - 1]}[ws]
    fn = pli.gemm_fp8 if fmt == "fp8" else pli.gemm_mxfp4
    fn(dev_u8(x8, 0x7F, 16 if pad else 0), put(xs), *weights(fmt, w, pad),
       bias=None if bias is None else torch.from_numpy(bias).to(TDT[dt]).to(DEV), out=g.view, out_dtype=TDT[dt],
       workspace=work, splits=splits)
    assert pli.last_route() == route
    torch.cuda.synchronize()
    assert_untouched(g, lambda v: v)
    assert_untouched(gw, (lambda v: v) if route == SPLIT else (lambda v: v[:0]), what="workspace")
    return g.view.clone().cpu()


def exact_data(fmt, m, n, k):
    """(x8, w, want64): small-integer patterns whose every partial sum is exact in fp32 in any order"""
    if fmt == "fp8":
        x8, w8, xd, wd = fc.asymmetric_codes(m, n, k)
        w = (w8, None)
    else:
        r, j, i = np.arange(m)[:, None], np.arange(n)[:, None], np.arange(k)[None, :]
        xd = (((3 * r + 5 * i + (r * i) // 7) % 7) - 3).astype(np.float64)
        nib = ((7 * j + 2 * i + (j * i) // 5 + 1) % 16).astype(np.uint8)
        exps = (127 + ((j + 3 * np.arange(k // 32)[None, :]) % 9 - 4)).astype(np.uint8)
        x8, wd, w = fc.small_int_code(xd), weight64(nib, exps), (nib, exps)
    # every term a multiple of 2^-5 and every partial sum below 2^19: 24 bits; the results inside fp16's range
    assert np.array_equal(np.rint(wd * 32), wd * 32) and float((np.abs(xd) @ np.abs(wd).T).max()) < 2 ** 19
    want = xd @ wd.T + 0.0
    assert float(np.abs(want).max()) < 65504
    return x8, w, want


# ---- 1. bitwise on exact data: each MC, the ragged last block, two m tiles, one-step and unequal chunks -------
EXACT = [(17, 128, 256, 2), (32, 132, 640, 3), (33, 260, 1024, 5), (64, 128, 640, 5), (65, 132, 1024, 2),
         (96, 260, 256, 2), (97, 128, 640, 3), (128, 132, 1024, 3), (129, 260, 640, 2), (256, 128, 1024, 5)]


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("m,n,k,splits", EXACT)
def test_split_is_the_f64_result_and_the_plain_call_bitwise(pli, m, n, k, splits, fmt, dt):
    x8, w, want = exact_data(fmt, m, n, k)
    got = run(pli, fmt, x8, None, w, dt, splits=splits)
    assert torch.equal(bits(got), bits(torch.from_numpy(want).to(TDT[dt])))
    assert torch.equal(bits(got), bits(run(pli, fmt, x8, None, w, dt, ws=None, route=PLAIN[fmt])))


# ---- 2. the f64 oracle per element ---------------------------------------------------------------------
@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("splits", [0, 16])
@pytest.mark.parametrize("m", [48, 128, 200])
def test_split_against_f64_oracle(pli, m, splits, fmt, dt):
    n, k = 256, 2048
    if fmt == "fp8":
        op, ref = fc.case_reference(fc.Case(m, n, k, fc.MX, True, "both", "pad"), dt)
        x8, xs, w, bias = op.x8, op.xs, (op.w8, op.ws), op.bias
    else:
        x8, xs, nib, exps, bias, ref = case_operands((m, n, k, PLAIN[fmt], "bias,pad"), dt)
        w = (nib, exps)
    got = run(pli, fmt, x8, xs, w, dt, splits=splits, bias=bias, pad=True)
    ra, rb = fc.ratios(got.double().numpy(), ref, dt)
    print(f"{fmt} m{m} splits {splits} {dt}: err / (a) {ra:.3f}, err / (b) {rb:.3f}")
    assert ra <= 1.0 and rb <= 1.0, (fmt, m, splits, dt, ra, rb)


# ---- 3. NaN rules, each in a chunk other than chunk 0 --------------------------------------------------
@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_nan_poisons_exactly_its_row_or_column(pli, fmt, dt):
    m, n, k, splits = 33, 132, 640, 5  # five chunks of one K-step
    x8, w, _ = exact_data(fmt, m, n, k)
    clean = run(pli, fmt, x8, None, w, dt, splits=splits)
    xn = x8.copy()
    xn[20, 3 * 128 + 77] = 0x7F  # chunk 3
    wn = (w[0].copy(), None if w[1] is None else w[1].copy())
    if fmt == "fp8":
        wn[0][130, 4 * 128 + 5] = 0xFF  # a NaN code in w8, chunk 4
    else:
        wn[1][130, (2 * 128 + 64) // 32] = 0xFF  # a NaN scale byte, chunk 2
    for got, row, col in ((run(pli, fmt, xn, None, w, dt, splits=splits), 20, None),
                          (run(pli, fmt, x8, None, wn, dt, splits=splits), None, 130)):
        want_nan = torch.zeros(m, n, dtype=torch.bool)
        want_nan[row if row is not None else slice(None), col if col is not None else slice(None)] = True
        assert torch.equal(torch.isnan(got), want_nan)
        assert torch.equal(bits(got)[~want_nan], bits(clean)[~want_nan])


# ---- 4. replay, determinism, fallback ------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_graph_replays_after_in_place_changes_and_calls_repeat(pli, fmt):
    m, n, k, dt = 65, 132, 1024, "bf16"
    x8, w, _ = exact_data(fmt, m, n, k)
    x8d, xs = put(x8), torch.rand(m, device=DEV) + 0.5
    wd = weights(fmt, w)
    fn = pli.gemm_fp8 if fmt == "fp8" else pli.gemm_mxfp4
    work = torch.empty(getattr(pli, f"gemm_{fmt}_workspace_bytes")(m, n, k, 3), dtype=torch.uint8, device=DEV)
    out = torch.empty(m, n, dtype=TDT[dt], device=DEV)
    call = lambda o=None: fn(x8d, xs, *wd, out=o, out_dtype=TDT[dt], workspace=work, splits=3)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(out)
    assert pli.last_route() == SPLIT
    seen = []
    for change in (False, True, True):  # several replays, each against the eager call on the same operands
        if change:
            xs[7] *= 2
            x8d[9].copy_(torch.roll(x8d[9], 1))
            wd[0][11].copy_(torch.roll(wd[0][11], 1))
        g.replay()
        torch.cuda.synchronize()
        seen.append(out.clone())
        assert torch.equal(bits(seen[-1]), bits(call())) and torch.equal(bits(seen[-1]), bits(call()))
    assert not torch.equal(bits(seen[0]), bits(seen[1])) and not torch.equal(bits(seen[1]), bits(seen[2]))


@pytest.mark.parametrize("dt", fc.DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_fallback_is_the_plain_call(pli, fmt, dt):
    m, n, k = 65, 132, 640
    x8, w, _ = exact_data(fmt, m, n, k)
    plain = run(pli, fmt, x8, None, w, dt, ws=None, route=PLAIN[fmt])
    for kw in (dict(ws="short", splits=2), dict(splits=1), dict(ws=None, splits=2)):
        assert torch.equal(bits(run(pli, fmt, x8, None, w, dt, route=PLAIN[fmt], **kw)), bits(plain)), kw
