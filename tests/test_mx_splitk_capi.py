"""pli_gemm_fp8_ws / pli_gemm_mxfp4_ws and their size functions without a GPU: the plain calls' PLI_EINVAL rules in
their order and then splits < 0, before any HIP call; the workspace sizes against a replay of the split rule; and the
conditions under which the call is the plain one, seen through a reported size of 0."""
from __future__ import annotations

import ctypes

import pytest

EINVAL, OK = 1000, 0
F32, BF16 = 0, 2
P = ctypes.c_void_p(4096)  # never dereferenced: validation fails first


@pytest.fixture()
def L(built_lib):
    import pli_hip
    return pli_hip.lib()


def _call(L, fmt, **kw):
    a = dict(x8=P, xs=P, w=P, ws=P, we=P, bias=None, c=P, m=32, n=64, k=512, ldx8=512, ldw=512 if fmt == "fp8" else 256,
             lds=16, ldc=64, dtype=BF16, work=P, bytes=1 << 20, splits=0)
    a.update(kw)
    tail = (a["dtype"], a["work"], a["bytes"], a["splits"], None)
    if fmt == "fp8":
        return L.pli_gemm_fp8_ws(a["x8"], a["xs"], a["w"], a["ws"], a["bias"], a["c"], a["m"], a["n"], a["k"],
                                 a["ldx8"], a["ldw"], a["ldc"], *tail)
    return L.pli_gemm_mxfp4_ws(a["x8"], a["xs"], a["w"], a["we"], a["bias"], a["c"], a["m"], a["n"], a["k"], a["ldx8"],
                               a["ldw"], a["lds"], a["ldc"], *tail)


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_argument_validation_in_order_without_gpu(L, fmt):
    err, name = L.pli_last_error, f"pli_gemm_{fmt}_ws: ".encode()
    big = dict(m=1 << 30, n=1024, ldc=1024)
    # each rule alone, then with every later rule broken too: the earliest one reports
    rules = [(dict(dtype=F32), dict(n=-1, c=None, splits=-1), b"bad dtype"),
             (dict(n=-1), dict(k=48, c=None, splits=-1), b"bad shape"),
             (dict(ldc=0), dict(c=None, splits=-1), b"leading dimension too small"),
             (dict(c=None), dict(splits=-1, **big), b"null pointer"),
             (big, dict(splits=-1), b"grid too large"),
             (dict(splits=-1), {}, b"bad splits")]
    if fmt == "mxfp4":
        rules.insert(2, (dict(k=48), dict(ldc=0, c=None, splits=-1), b"MX block"))
    for kw, later, msg in rules:
        for broken in (kw, {**later, **kw}):
            assert _call(L, fmt, **broken) == EINVAL and err().startswith(name) and msg in err(), (broken, err())
    none = dict(x8=None, xs=None, w=None, ws=None, we=None, c=None, work=None, bytes=0)
    assert _call(L, fmt, m=0, **none) == OK and _call(L, fmt, n=0, ldc=0, **none) == OK
    assert _call(L, fmt, m=0, splits=-1, **none) == EINVAL and b"bad splits" in err()
    assert L.pli_last_route() == b""  # nothing was launched


def rule(m, n, k, splits):
    """the split rule of include/pli.h, restated"""
    ks, tiles = k // 128, -(-n // 128) * -(-m // 128)
    s = max(1, min(16, min(splits, ks) if splits else min(-(-256 // tiles) if tiles <= 128 else 1, ks // 4)))
    return -(-ks // -(-ks // s))


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_workspace_sizes_and_fallback_conditions(L, fmt):
    size = getattr(L, f"pli_gemm_{fmt}_workspace_size")
    for m in (17, 64, 128, 129, 256):
        for n, k in ((4096, 4096), (14336, 4096), (4096, 14336), (8192, 8192), (132, 640), (4, 128), (4096, 512)):
            for splits in (0, 1, 2, 3, 5, 16, 40):
                s = rule(m, n, k, splits)
                assert size(m, n, k, splits) == (s * m * n * 4 if s >= 2 else 0), (m, n, k, splits, s)
    assert size(64, 4096, 4096, 0) == 8 * 64 * 4096 * 4 and size(64, 4096, 4096, 1) == 0
    # the call is the plain one: fewer than 17 or more than 256 rows, k % 128, n % 4, one K-step, negative splits
    for m, n, k, splits in ((16, 4096, 4096, 0), (257, 4096, 4096, 0), (512, 4096, 4096, 4), (64, 4096, 4160, 0),
                            (64, 4098, 4096, 0), (64, 4096, 128, 4), (64, 4096, 4096, -1), (0, 4096, 4096, 0)):
        assert size(m, n, k, splits) == 0, (m, n, k, splits)
