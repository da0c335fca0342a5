"""The fp8-activation entry points of include/pli.h without a GPU: the two symbols are declared and exported, each
argument rule returns PLI_EINVAL with its message before any HIP call and in the documented order, empty calls
return PLI_OK with NULL operands, the grid guard, and the Python wrappers refusing CPU tensors and wrong dtypes."""
from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

EINVAL, OK = 1000, 0
F32, F16, BF16 = 0, 1, 2
P = ctypes.c_void_p(4096)  # never dereferenced: validation fails first
NAMES = ("pli_quantize_rows_fp8", "pli_gemm_fp8")


@pytest.fixture()
def L(built_lib):
    import pli_hip
    return pli_hip.lib()


def _quant(L, **kw):
    a = dict(x=P, ldx=512, x8=P, ldx8=512, s=P, m=4, k=512, dtype=BF16)
    a.update(kw)
    return L.pli_quantize_rows_fp8(a["x"], a["ldx"], a["x8"], a["ldx8"], a["s"], a["m"], a["k"], a["dtype"], None)


def _gemm(L, **kw):
    a = dict(x8=P, xs=P, w8=P, ws=P, bias=None, c=P, m=32, n=64, k=512, ldx8=512, ldw=512, ldc=64, dtype=BF16)
    a.update(kw)
    return L.pli_gemm_fp8(a["x8"], a["xs"], a["w8"], a["ws"], a["bias"], a["c"], a["m"], a["n"], a["k"], a["ldx8"],
                          a["ldw"], a["ldc"], a["dtype"], None)


def test_symbols_declared_and_exported(L):
    header = open(os.path.join(ROOT, "include", "pli.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\(", header), name
        assert getattr(L, name) is not None


def test_quantiser_argument_validation_without_gpu(L):
    err = L.pli_last_error
    for dt in (F32, 7, -1):
        assert _quant(L, dtype=dt) == EINVAL and b"pli_quantize_rows_fp8: bad dtype" in err(), dt
    for kw in (dict(m=-1), dict(k=-1)):
        assert _quant(L, **kw) == EINVAL and b"pli_quantize_rows_fp8: bad shape" in err(), kw
    for kw in (dict(ldx=511), dict(ldx8=511)):
        assert _quant(L, **kw) == EINVAL and b"leading dimension too small" in err(), kw
    for name in ("x", "x8", "s"):
        assert _quant(L, **{name: None}) == EINVAL and b"null pointer" in err(), name
    # k == 0 needs only the scales
    assert _quant(L, k=0, x=None, x8=None, s=None) == EINVAL and b"null pointer" in err()
    # the order: dtype, shape, leading dimension, pointers
    assert _quant(L, dtype=F32, m=-1, ldx=0, x=None) == EINVAL and b"bad dtype" in err()
    assert _quant(L, m=-1, ldx=0, x=None) == EINVAL and b"bad shape" in err()
    assert _quant(L, ldx=0, x=None) == EINVAL and b"leading dimension" in err()
    assert L.pli_last_route() == b""  # nothing was launched


def test_gemm_argument_validation_without_gpu(L):
    err = L.pli_last_error
    for dt in (F32, 7, -1):
        assert _gemm(L, dtype=dt) == EINVAL and b"pli_gemm_fp8: bad dtype" in err(), dt
    for kw in (dict(m=-1), dict(n=-1), dict(k=-1)):
        assert _gemm(L, **kw) == EINVAL and b"pli_gemm_fp8: bad shape" in err(), kw
    for kw in (dict(ldx8=511), dict(ldw=511), dict(ldc=63)):
        assert _gemm(L, **kw) == EINVAL and b"leading dimension too small" in err(), kw
    for name in ("x8", "w8", "c"):
        assert _gemm(L, **{name: None}) == EINVAL and b"null pointer" in err(), name
    assert _gemm(L, k=0, ldx8=0, ldw=0, x8=None, w8=None, c=None) == EINVAL and b"null pointer" in err()
    # the order: dtype, shape, leading dimension, pointers
    assert _gemm(L, dtype=F32, n=-1, ldc=0, c=None) == EINVAL and b"bad dtype" in err()
    assert _gemm(L, n=-1, ldc=0, c=None) == EINVAL and b"bad shape" in err()
    assert _gemm(L, ldc=0, c=None) == EINVAL and b"leading dimension" in err()
    assert L.pli_last_route() == b""


def test_grid_guard_without_gpu(L):
    """one thread per output in the generic kernel: m * n / 256 workgroups must fit the grid's x dimension; the rule
    holds on every route, as in the fp8w calls"""
    big = 1 << 30
    assert _gemm(L, m=big, n=1024, ldc=1024) == EINVAL and b"grid too large" in L.pli_last_error()
    assert _gemm(L, m=big, n=1023, k=40, ldx8=40, ldw=40, ldc=1023) == EINVAL and b"grid too large" in L.pli_last_error()
    assert L.pli_last_route() == b""


def test_empty_calls_without_gpu(L):
    """m == 0 (n == 0) returns PLI_OK before any HIP call and every operand, the scales among them, may be NULL"""
    assert _quant(L, m=0, x=None, x8=None, s=None) == OK
    assert _quant(L, m=0, k=0, ldx=0, ldx8=0, x=None, x8=None, s=None) == OK
    none = dict(x8=None, xs=None, w8=None, ws=None, c=None)
    assert _gemm(L, m=0, **none) == OK
    assert _gemm(L, n=0, ldc=0, **none) == OK
    assert _gemm(L, m=0, n=0, k=0, ldx8=0, ldw=0, ldc=0, **none) == OK
    assert L.pli_last_route() == b""
    # the argument checks still come first
    assert _quant(L, m=0, dtype=F32) == EINVAL
    assert _gemm(L, m=0, k=-1) == EINVAL
    assert _gemm(L, n=0, dtype=9) == EINVAL


def test_wrappers_refuse_cpu_tensors_and_wrong_dtypes(built_lib):
    import pli_hip
    x = torch.zeros(20, 128, dtype=torch.bfloat16)
    codes = torch.zeros(32, 128, dtype=torch.float8_e4m3fn)
    scale = torch.ones(32)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.gemm_fp8(codes[:20], scale[:20], codes, scale)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.linear_fp8a(x, codes, scale)
    with pytest.raises(pli_hip.PliError, match="2-D"):
        pli_hip.quantize_rows_fp8(x[0])
    with pytest.raises(pli_hip.PliError, match="fp16 or bf16"):
        pli_hip.quantize_rows_fp8(x.float())
    with pytest.raises(pli_hip.PliError, match="device path"):
        pli_hip.quantize_rows_fp8(x, out=(codes[:20], scale[:20]))
    # the CPU path of the quantiser is torch ops
    c8, s = pli_hip.quantize_rows_fp8(x)
    assert c8.dtype == torch.float8_e4m3fn and tuple(c8.shape) == (20, 128) and torch.equal(s, torch.ones(20))


@pytest.mark.gpu
def test_wrappers_refuse_wrong_operands_on_the_device(built_lib):
    import pli_hip
    dev = "cuda:0"
    x8 = torch.zeros(20, 128, dtype=torch.uint8, device=dev)
    w8 = torch.zeros(32, 128, dtype=torch.uint8, device=dev)
    xs, ws = torch.ones(20, device=dev), torch.ones(32, device=dev)
    with pytest.raises(pli_hip.PliError, match="float8_e4m3fn or torch.uint8"):
        pli_hip.gemm_fp8(x8.to(torch.int8), xs, w8, ws)
    with pytest.raises(pli_hip.PliError, match="x_scale must be"):
        pli_hip.gemm_fp8(x8, xs.double(), w8, ws)
    with pytest.raises(pli_hip.PliError, match="w_scale must be"):
        pli_hip.gemm_fp8(x8, xs, w8, ws[:31])
    with pytest.raises(pli_hip.PliError, match="shape mismatch"):
        pli_hip.gemm_fp8(x8[:, :64], xs, w8, ws)
    with pytest.raises(pli_hip.PliError, match="out_dtype"):
        pli_hip.gemm_fp8(x8, xs, w8, ws, out_dtype=torch.float32)
    with pytest.raises(pli_hip.PliError, match="out has shape"):
        pli_hip.gemm_fp8(x8, xs, w8, ws, out=torch.empty(20, 31, dtype=torch.bfloat16, device=dev))
    with pytest.raises(pli_hip.PliError, match="bias must be"):
        pli_hip.gemm_fp8(x8, xs, w8, ws, bias=torch.zeros(32, dtype=torch.float16, device=dev))
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.gemm_fp8(x8, xs, w8.cpu(), ws)
