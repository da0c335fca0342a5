"""The weight-only fp8 linear entry points of include/pli.h without a GPU: the
five symbols are declared and exported, each argument rule returns PLI_EINVAL
with its message before any HIP call, empty calls return PLI_OK with NULL
operands, the workspace sizes, and the Python wrappers refusing CPU tensors
and wrong dtypes."""
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
NAMES = ("pli_gemv_fp8w", "pli_linear_fp8w_workspace_size", "pli_linear_fp8w", "pli_linear_swiglu_fp8w_workspace_size",
         "pli_linear_swiglu_fp8w")


@pytest.fixture()
def L(built_lib):
    import pli_hip
    return pli_hip.lib()


def _linear(L, **kw):
    a = dict(x=P, w=P, s=P, bias=None, c=P, m=4, n=64, k=512, ldx=512, ldw=512, ldc=64, dtype=BF16, ws=None, ws_bytes=0)
    a.update(kw)
    return L.pli_linear_fp8w(a["x"], a["w"], a["s"], a["bias"], a["c"], a["m"], a["n"], a["k"], a["ldx"], a["ldw"],
                             a["ldc"], a["dtype"], a["ws"], a["ws_bytes"], None)


def _swiglu(L, **kw):
    a = dict(x=P, wg=P, sg=P, wu=P, su=P, h=P, m=4, n=64, k=512, ldx=512, ldwg=512, ldwu=512, ldh=64, dtype=BF16, ws=None,
             ws_bytes=0)
    a.update(kw)
    return L.pli_linear_swiglu_fp8w(a["x"], a["wg"], a["sg"], a["wu"], a["su"], a["h"], a["m"], a["n"], a["k"], a["ldx"],
                                    a["ldwg"], a["ldwu"], a["ldh"], a["dtype"], a["ws"], a["ws_bytes"], None)


def _gemv(L, **kw):
    a = dict(w=P, s=P, x=P, y=P, m=64, k=512, ldw=512, dtype=BF16)
    a.update(kw)
    return L.pli_gemv_fp8w(a["w"], a["s"], a["x"], a["y"], a["m"], a["k"], a["ldw"], a["dtype"], None)


def test_symbols_declared_and_exported(L):
    header = open(os.path.join(ROOT, "include", "pli.h")).read()
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\(", header), name
        assert getattr(L, name) is not None


def test_linear_argument_validation_without_gpu(L):
    err = L.pli_last_error
    for dt in (F32, 7, -1):
        assert _linear(L, dtype=dt) == EINVAL and b"pli_linear_fp8w: bad dtype" in err(), dt
    for kw in (dict(m=-1), dict(n=-1), dict(k=-1)):
        assert _linear(L, **kw) == EINVAL and b"pli_linear_fp8w: bad shape" in err(), kw
    for kw in (dict(ldx=511), dict(ldw=511), dict(ldc=63)):
        assert _linear(L, **kw) == EINVAL and b"leading dimension too small" in err(), kw
    for name in ("x", "w", "c"):
        assert _linear(L, **{name: None}) == EINVAL and b"null pointer" in err(), name
    # the widen route (m > 16, no fast route, a workspace): the workspace must be aligned and large enough
    shape = dict(m=17, n=24, k=40, ldx=40, ldw=40, ldc=24)
    need = L.pli_linear_fp8w_workspace_size(17, 24, 40, BF16)
    assert need == 24 * 40 * 2
    assert _linear(L, ws=P, ws_bytes=need - 1, **shape) == EINVAL and b"workspace" in err()
    assert _linear(L, ws=ctypes.c_void_p(4104), ws_bytes=need, **shape) == EINVAL and b"16-byte aligned" in err()
    assert L.pli_last_route() == b""  # nothing was launched


def test_swiglu_and_gemv_argument_validation_without_gpu(L):
    err = L.pli_last_error
    assert _swiglu(L, dtype=F32) == EINVAL and b"pli_linear_swiglu_fp8w: bad dtype" in err()
    for kw in (dict(m=-1), dict(n=-1), dict(k=-1)):
        assert _swiglu(L, **kw) == EINVAL and b"pli_linear_swiglu_fp8w: bad shape" in err(), kw
    for kw in (dict(ldx=8), dict(ldwg=8), dict(ldwu=8), dict(ldh=8)):
        assert _swiglu(L, **kw) == EINVAL and b"leading dimension too small" in err(), kw
    for name in ("x", "wg", "wu", "h"):
        assert _swiglu(L, **{name: None}) == EINVAL and b"null pointer" in err(), name
    shape = dict(m=17, n=24, k=40, ldx=40, ldwg=40, ldwu=40, ldh=24)
    need = L.pli_linear_swiglu_fp8w_workspace_size(17, 24, 40, F16)
    assert need == 2 * 24 * 40 * 2
    assert _swiglu(L, ws=P, ws_bytes=need // 2, **shape) == EINVAL and b"workspace" in err()
    assert _swiglu(L, ws=ctypes.c_void_p(4100), ws_bytes=need, **shape) == EINVAL and b"16-byte aligned" in err()

    assert _gemv(L, dtype=F32) == EINVAL and b"pli_gemv_fp8w: bad dtype" in err()
    for kw in (dict(m=-1), dict(k=-1)):
        assert _gemv(L, **kw) == EINVAL and b"pli_gemv_fp8w: bad shape" in err(), kw
    assert _gemv(L, ldw=500) == EINVAL and b"leading dimension too small" in err()
    for name in ("w", "x", "y"):
        assert _gemv(L, **{name: None}) == EINVAL and b"null pointer" in err(), name
    assert L.pli_last_route() == b""


def test_empty_calls_without_gpu(L):
    """m == 0 or n == 0 returns PLI_OK before any HIP call and the operands, the scales among them, may be NULL"""
    none = dict(x=None, w=None, s=None, c=None)
    assert _linear(L, m=0, **none) == OK
    assert _linear(L, n=0, ldc=0, **none) == OK
    assert _linear(L, m=0, n=0, k=0, ldx=0, ldw=0, ldc=0, **none) == OK
    none = dict(x=None, wg=None, sg=None, wu=None, su=None, h=None)
    assert _swiglu(L, m=0, **none) == OK
    assert _swiglu(L, n=0, ldh=0, **none) == OK
    assert _gemv(L, m=0, w=None, s=None, x=None, y=None) == OK
    assert L.pli_last_route() == b""
    # the argument checks still come first
    assert _linear(L, m=0, dtype=F32) == EINVAL
    assert _swiglu(L, m=0, k=-1) == EINVAL
    assert _gemv(L, m=0, dtype=9) == EINVAL


def test_workspace_sizes(L):
    al = lambda b: (b + 15) // 16 * 16  # noqa: E731
    for m, n, k in ((1, 4096, 4096), (16, 24, 40), (17, 4096, 4096), (128, 14336, 4096), (64, 32000, 2048)):
        for dt in (F16, BF16):
            assert L.pli_linear_fp8w_workspace_size(m, n, k, dt) == 0, (m, n, k)
            assert L.pli_linear_swiglu_fp8w_workspace_size(m, n, k, dt) == 0, (m, n, k)
    for m, n, k in ((17, 24, 40), (129, 4096, 4096), (2048, 32000, 2048), (64, 33, 257), (128, 48, 384), (17, 3, 3)):
        for dt in (F16, BF16):
            assert L.pli_linear_fp8w_workspace_size(m, n, k, dt) == al(n * k * 2), (m, n, k)
            assert L.pli_linear_swiglu_fp8w_workspace_size(m, n, k, dt) == 2 * al(n * k * 2), (m, n, k)
    assert L.pli_linear_fp8w_workspace_size(129, 64, 64, F32) == 0
    assert L.pli_linear_fp8w_workspace_size(-1, 64, 64, BF16) == 0 and L.pli_linear_fp8w_workspace_size(129, 0, 64, BF16) == 0


def test_wrappers_refuse_cpu_tensors_and_wrong_dtypes(built_lib):
    import pli_hip
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    codes = torch.zeros(32, 64, dtype=torch.float8_e4m3fn)
    scale = torch.ones(32)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.linear_fp8w(x, codes, scale)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.gemv_fp8w(codes, scale, x[0])
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.linear_swiglu_fp8w(x, codes, scale, codes, scale)
    with pytest.raises(pli_hip.PliError, match="2-D"):
        pli_hip.linear_fp8w(x[0], codes, scale)
    with pytest.raises(pli_hip.PliError, match="1-D"):
        pli_hip.gemv_fp8w(codes, scale, x)
    assert pli_hip.linear_fp8w_workspace_bytes(17, 24, 40, torch.float16) == 24 * 40 * 2
    assert pli_hip.linear_fp8w_workspace_bytes(17, 24, 40, torch.bfloat16, swiglu=True) == 2 * 24 * 40 * 2
    assert pli_hip.linear_fp8w_workspace_bytes(16, 24, 40) == 0
    assert pli_hip.linear_fp8w_workspace_bytes(17, 24, 40, torch.float32) == 0


@pytest.mark.gpu
def test_wrappers_refuse_wrong_dtypes_on_the_device(built_lib):
    import pli_hip
    dev = "cuda:0"
    x = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    codes = torch.zeros(32, 64, dtype=torch.uint8, device=dev)
    scale = torch.ones(32, device=dev)
    with pytest.raises(pli_hip.PliError, match="fp16 or bf16"):
        pli_hip.linear_fp8w(x.float(), codes, scale)
    with pytest.raises(pli_hip.PliError, match="float8_e4m3fn or torch.uint8"):
        pli_hip.linear_fp8w(x, codes.to(torch.int8), scale)
    with pytest.raises(pli_hip.PliError, match="scale must be"):
        pli_hip.linear_fp8w(x, codes, scale.double())
    with pytest.raises(pli_hip.PliError, match="shape mismatch"):
        pli_hip.linear_fp8w(x[:, :32], codes, scale)
    with pytest.raises(pli_hip.PliError, match="out has shape"):
        pli_hip.linear_fp8w(x, codes, scale, out=torch.empty(4, 31, dtype=torch.bfloat16, device=dev))
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.linear_fp8w(x, codes.cpu(), scale)
