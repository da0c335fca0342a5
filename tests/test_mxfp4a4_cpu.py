"""MXFP4 activations (W4A4) without a GPU: the argument rules of pli_quantize_rows_mxfp4 / pli_gemm_mxfp4_a4, and
quantize_rows_mxfp4 on CPU tensors against a float64 nearest-of-16 search over 2^(E_r + e_b) * E2M1."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from decode_step_cases import TDT

EINVAL, OK = 1000, 0
F32, F16, BF16 = 0, 1, 2
P = ctypes.c_void_p(4096)  # never dereferenced: validation fails first
E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])


@pytest.fixture()
def L(built_lib):
    import pli_hip
    return pli_hip.lib()


def _gemm(L, **kw):
    a = dict(x4=P, xe=P, xs=P, w4=P, we=P, bias=None, c=P, m=32, n=64, k=512, ldx4=256, ldxs=16, ldw=256, lds=16,
             ldc=64, dtype=BF16)
    a.update(kw)
    return L.pli_gemm_mxfp4_a4(a["x4"], a["xe"], a["xs"], a["w4"], a["we"], a["bias"], a["c"], a["m"], a["n"], a["k"],
                               a["ldx4"], a["ldxs"], a["ldw"], a["lds"], a["ldc"], a["dtype"], None)


def _quant(L, **kw):
    a = dict(x=P, ldx=512, x4=P, ldx4=256, xe=P, ldxs=16, xs=P, m=32, k=512, dtype=BF16)
    a.update(kw)
    return L.pli_quantize_rows_mxfp4(a["x"], a["ldx"], a["x4"], a["ldx4"], a["xe"], a["ldxs"], a["xs"], a["m"], a["k"],
                                     a["dtype"], None)


@pytest.mark.parametrize("call,name,shapes,lds,ptrs", [
    (_gemm, b"pli_gemm_mxfp4_a4", ("m", "n"), dict(ldx4=255, ldxs=15, ldw=255, lds=15, ldc=63),
     ("x4", "xe", "w4", "we", "c")),
    (_quant, b"pli_quantize_rows_mxfp4", ("m",), dict(ldx=511, ldx4=255, ldxs=15), ("x", "x4", "xe", "xs")),
], ids=["gemm", "quant"])
def test_argument_rules_in_order_without_gpu(L, call, name, shapes, lds, ptrs):
    err = L.pli_last_error
    for dt in (F32, 7, -1):
        assert call(L, dtype=dt) == EINVAL and name + b": bad dtype" in err(), dt
    for kw in [{s: -1} for s in shapes] + [dict(k=-32)]:
        assert call(L, **kw) == EINVAL and name + b": bad shape" in err(), kw
    for k in (16, 48, 500):
        assert call(L, k=k) == EINVAL and b"not a multiple of the MX block of 32" in err(), k
    for ld, v in lds.items():
        assert call(L, **{ld: v}) == EINVAL and b"leading dimension too small" in err(), ld
    for p in ptrs:
        assert call(L, **{p: None}) == EINVAL and b"null pointer" in err(), p
    # the order: dtype, shape, k % 32, leading dimension, pointers
    bad = dict(k=48, **{ptrs[0]: None}, **{next(iter(lds)): 0})
    assert call(L, dtype=F32, m=-1, **bad) == EINVAL and b"bad dtype" in err()
    assert call(L, m=-1, **bad) == EINVAL and b"bad shape" in err()
    assert call(L, **bad) == EINVAL and b"MX block" in err()
    assert call(L, **dict(bad, k=512)) == EINVAL and b"leading dimension" in err()
    assert L.pli_last_route() == b""  # nothing was launched


def test_grid_rule_and_empty_calls_without_gpu(L):
    assert _gemm(L, xs=None, m=1 << 30, n=1024, ldc=1024) == EINVAL and b"grid too large" in L.pli_last_error()
    assert _gemm(L, c=None, m=1 << 30, n=1024, ldc=1024) == EINVAL and b"null pointer" in L.pli_last_error()
    none = dict(x4=None, xe=None, xs=None, w4=None, we=None, c=None)
    assert _gemm(L, m=0, **none) == OK and _gemm(L, n=0, ldc=0, **none) == OK
    assert _gemm(L, m=0, n=0, k=0, ldx4=0, ldxs=0, ldw=0, lds=0, ldc=0, **none) == OK
    assert _quant(L, m=0, x=None, x4=None, xe=None, xs=None) == OK
    assert _gemm(L, k=0, **none) == EINVAL and b"null pointer" in L.pli_last_error()
    assert _quant(L, k=0, x=None, x4=None, xe=None, xs=None) == EINVAL and b"null pointer" in L.pli_last_error()
    assert _gemm(L, m=0, k=48) == EINVAL and _quant(L, m=0, dtype=9) == EINVAL
    assert L.pli_last_route() == b""


def mirror_rows(dt: str, rows: int = 128, k: int = 96) -> torch.Tensor:
    """seeded rows, then: exact ties, a zero block, a zero row, infinities, NaN, a block far below its row's amax"""
    g = torch.Generator().manual_seed(4040 + (dt == "fp16"))
    x = torch.randn(rows, k, generator=g) * torch.exp2(torch.randint(-6, 7, (rows, k // 32, 1), generator=g).float()
                                                       ).expand(-1, -1, 32).reshape(rows, k)
    ties = torch.tensor([.25, .75, 1.25, 1.75, 2.5, 3.5, 5., 6.])
    x[0, :32] = torch.cat((ties, -ties, ties * 0.5, -ties * 0.5))  # block amax 6, row amax 6: grid step as written
    x[0, 32:] = 0.0
    x[1, 32:64] = 0.0
    x[1, 40] = -0.0
    x[2] = 0.0
    x[3, 5], x[3, 70] = float("inf"), float("-inf")
    x[4, 33], x[5, 0] = float("nan"), float("nan")
    x[5, 1:32] = 0.0
    x[6, :32] = torch.randn(32, generator=g) * 2.0 ** -14
    x[6, 32] = 2.0 ** 15
    x[7] = float("inf")
    return x.to(TDT[dt])


@pytest.mark.parametrize("dt", ("bf16", "fp16"))
def test_quantiser_mirror_against_f64_nearest_search(built_lib, dt):
    import pli_hip
    lo, hi = pli_hip.MXFP4X_EXP_RANGE
    x = mirror_rows(dt)
    codes, exps, scale = pli_hip.quantize_rows_mxfp4(x)
    m, k = x.shape
    xd = x.double().numpy().reshape(m, k // 32, 32)
    nan, fin = np.isnan(xd), np.isfinite(xd)
    a = np.where(fin, np.abs(xd), 0.0)
    # the exponent rule: x_scale a power of two, bytes inside the contract and as the rule says
    frac, sexp = np.frexp(scale.double().numpy())
    row_exp = np.where(a.max(axis=(1, 2)) > 0, np.frexp(a.max(axis=(1, 2)))[1] - 3, 0)
    assert (frac == 0.5).all() and np.array_equal(sexp - 1, row_exp)
    want_e = np.where(a.max(axis=2) > 0, np.maximum(np.frexp(a.max(axis=2))[1] - 3 - row_exp[:, None], lo), 0)
    e = exps.numpy().astype(np.int64) - 127
    assert np.array_equal(exps.numpy() == 0xFF, nan.any(axis=2)) and int(nan.any(axis=2).sum()) == 2
    ok = ~nan.any(axis=2)
    assert np.array_equal(e[ok], want_e[ok]) and e[ok].min() == lo and e[ok].max() == 0 <= hi
    # every code a nearest grid value, the even code on a tie
    c = codes.numpy()
    nib = np.stack((c & 15, c >> 4), axis=2).reshape(m, k // 32, 32)
    grid = np.exp2((row_exp[:, None] + want_e).astype(np.float64))[:, :, None, None] * E2M1
    d = np.abs(np.where(fin, xd, np.sign(xd) * 1e300)[..., None] - grid)
    chosen = np.take_along_axis(d, nib[..., None].astype(np.int64), axis=3)[..., 0]
    tie = (d == d.min(axis=3, keepdims=True))[..., np.arange(16) != 8].sum(axis=3) > 1  # two distinct grid values
    assert (chosen == d.min(axis=3))[~nan].all()
    assert (nib[tie & fin] & 1 == 0).all() and int(tie[0, 0].sum()) == 20  # +-{.25 .75 1.25 1.75 2.5 3.5 5 1.25 1.75 2.5}
    assert (nib[nan] == 0).all() and (nib[np.isinf(xd)] == np.where(xd[np.isinf(xd)] > 0, 7, 15)).all()
    assert np.array_equal(nib[1, 1] >> 3, np.signbit(xd[1, 1]).astype(np.uint8))  # the sign of a zero is kept
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.gemm_mxfp4_a4(codes, exps, None, codes, exps)
