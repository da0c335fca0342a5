"""pli_gemm_mxfp4 of include/pli.h without a GPU (tests/test_capi.py holds the exported set to the header): each
argument rule returns PLI_EINVAL with its message before any HIP call and in the documented order, empty calls return
PLI_OK with NULL operands, and the Python wrappers refuse CPU tensors."""
from __future__ import annotations

import ctypes

import pytest
import torch

EINVAL, OK = 1000, 0
F32, F16, BF16 = 0, 1, 2
P = ctypes.c_void_p(4096)  # never dereferenced: validation fails first


@pytest.fixture()
def L(built_lib):
    import pli_hip
    return pli_hip.lib()


def _gemm(L, **kw):
    a = dict(x8=P, xs=P, w4=P, we=P, bias=None, c=P, m=32, n=64, k=512, ldx8=512, ldw=256, lds=16, ldc=64, dtype=BF16)
    a.update(kw)
    return L.pli_gemm_mxfp4(a["x8"], a["xs"], a["w4"], a["we"], a["bias"], a["c"], a["m"], a["n"], a["k"], a["ldx8"],
                            a["ldw"], a["lds"], a["ldc"], a["dtype"], None)


def test_argument_validation_in_order_without_gpu(L):
    err = L.pli_last_error
    for dt in (F32, 7, -1):
        assert _gemm(L, dtype=dt) == EINVAL and b"pli_gemm_mxfp4: bad dtype" in err(), dt
    for kw in (dict(m=-1), dict(n=-1), dict(k=-32)):
        assert _gemm(L, **kw) == EINVAL and b"pli_gemm_mxfp4: bad shape" in err(), kw
    for k in (16, 48, 500):
        assert _gemm(L, k=k) == EINVAL and b"not a multiple of the MX block of 32" in err(), k
    for kw in (dict(ldx8=511), dict(ldw=255), dict(lds=15), dict(ldc=63)):
        assert _gemm(L, **kw) == EINVAL and b"leading dimension too small" in err(), kw
    for name in ("x8", "w4", "we", "c"):
        assert _gemm(L, **{name: None}) == EINVAL and b"null pointer" in err(), name
    assert _gemm(L, xs=None, bias=None, m=1 << 30, n=1024, ldc=1024) == EINVAL and b"grid too large" in err()
    # k == 0 needs only C
    assert _gemm(L, k=0, ldx8=0, ldw=0, lds=0, x8=None, w4=None, we=None, c=None) == EINVAL and b"null pointer" in err()
    # the order: dtype, shape, k % 32, leading dimension, pointers, grid
    assert _gemm(L, dtype=F32, n=-1, k=48, ldc=0, c=None) == EINVAL and b"bad dtype" in err()
    assert _gemm(L, n=-1, k=48, ldc=0, c=None) == EINVAL and b"bad shape" in err()
    assert _gemm(L, k=48, ldc=0, c=None) == EINVAL and b"MX block" in err()
    assert _gemm(L, ldc=0, c=None) == EINVAL and b"leading dimension" in err()
    assert _gemm(L, c=None, m=1 << 30, n=1024, ldc=1024) == EINVAL and b"null pointer" in err()
    assert L.pli_last_route() == b""  # nothing was launched


def test_empty_calls_without_gpu(L):
    none = dict(x8=None, xs=None, w4=None, we=None, c=None)
    assert _gemm(L, m=0, **none) == OK
    assert _gemm(L, n=0, ldc=0, **none) == OK
    assert _gemm(L, m=0, n=0, k=0, ldx8=0, ldw=0, lds=0, ldc=0, **none) == OK
    assert L.pli_last_route() == b""
    # the argument checks still come first
    assert _gemm(L, m=0, k=-32) == EINVAL and _gemm(L, n=0, dtype=9) == EINVAL and _gemm(L, m=0, k=48) == EINVAL


def test_wrappers_refuse_cpu_tensors(built_lib):
    import pli_hip
    x8 = torch.zeros(20, 128, dtype=torch.uint8)
    codes, exps = torch.zeros(32, 64, dtype=torch.uint8), torch.full((32, 4), 127, dtype=torch.uint8)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.gemm_mxfp4(x8, None, codes, exps)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.linear_mxfp4a(torch.zeros(20, 128, dtype=torch.bfloat16), codes, exps)
