"""The packed variable-length paged entry points of include/pli.h without a
GPU: every argument check answers PLI_EINVAL with its message before any HIP
call, empty calls return PLI_OK with NULL operands, and the Python wrappers
refuse CPU tensors and mismatched shapes."""
from __future__ import annotations

import ctypes

import pytest
import torch

EINVAL, OK = 1000, 0
BF16 = 2


def _attn(L, **kw):
    """pli_attn_varlen_paged on never-dereferenced pointers, one argument changed at a time"""
    p = ctypes.c_void_p(16)
    a = dict(q=p, k=p, v=p, o=p, cu=p, table=p, lens=p, batch=2, max_tokens=5, heads=8, kv_heads=2, head_dim=128,
             block_size=16, num_blocks=32, max_blocks=4, max_kv=64, strides=(ctypes.c_int64 * 10)(*([8] * 10)),
             scale=0.1, causal=1, dtype=BF16)
    a.update(kw)
    return L.pli_attn_varlen_paged(a["q"], a["k"], a["v"], a["o"], a["cu"], a["table"], a["lens"], a["batch"],
                                   a["max_tokens"], a["heads"], a["kv_heads"], a["head_dim"], a["block_size"],
                                   a["num_blocks"], a["max_blocks"], a["max_kv"], a["strides"], a["scale"],
                                   a["causal"], a["dtype"], None)


def _append(L, **kw):
    p = ctypes.c_void_p(16)
    a = dict(kn=p, vn=p, k=p, v=p, cu=p, table=p, lens=p, batch=2, max_tokens=5, kv_heads=2, head_dim=128,
             block_size=16, num_blocks=32, max_blocks=4, strides=(ctypes.c_int64 * 10)(*([8] * 10)), dtype=BF16)
    a.update(kw)
    return L.pli_kv_append_varlen_paged(a["kn"], a["vn"], a["k"], a["v"], a["cu"], a["table"], a["lens"], a["batch"],
                                        a["max_tokens"], a["kv_heads"], a["head_dim"], a["block_size"],
                                        a["num_blocks"], a["max_blocks"], a["strides"], a["dtype"], None)


def test_varlen_argument_validation_without_gpu(built_lib):
    import pli_hip
    L = pli_hip.lib()
    err = lambda: L.pli_last_error()  # noqa: E731
    for kw in (dict(batch=-1), dict(max_tokens=-1), dict(heads=0), dict(kv_heads=0), dict(head_dim=0), dict(max_kv=-1),
               dict(num_blocks=-1), dict(max_blocks=-1)):
        assert _attn(L, **kw) == EINVAL and b"bad shape" in err(), kw
    assert _attn(L, heads=6, kv_heads=4) == EINVAL and b"multiple of kv_heads" in err()
    assert _attn(L, dtype=7) == EINVAL and b"dtype" in err()
    for s in (float("nan"), float("inf")):
        assert _attn(L, scale=s) == EINVAL and b"non-finite scale" in err()
    for bs in (0, -16):
        assert _attn(L, block_size=bs) == EINVAL and b"block_size" in err()
    assert _attn(L, max_kv=65) == EINVAL and b"max_kv" in err()  # 4 blocks of 16 hold 64
    assert _attn(L, block_size=1 << 20, max_blocks=1 << 11) == EINVAL and b"2^31" in err()
    for name in ("q", "k", "v", "o", "cu", "table", "lens", "strides"):
        assert _attn(L, **{name: None}) == EINVAL and b"null" in err(), name
    assert _attn(L, num_blocks=0) == EINVAL and b"empty pool" in err()
    assert _attn(L, max_blocks=0, max_kv=0) == EINVAL and b"empty pool or table" in err()
    # the generic path's limits (head_dim 264 is not a fast-path shape)
    assert _attn(L, head_dim=264) == EINVAL and b"head_dim" in err()
    assert _attn(L, head_dim=80, max_tokens=1 << 28) == EINVAL and b"grid too large" in err()
    # the MFMA path's grid: 2^29 tiles x 8 kv heads
    assert _attn(L, max_tokens=2 ** 31 - 1, heads=128, kv_heads=8) == EINVAL and b"grid too large" in err()
    assert L.pli_last_route() == b""  # nothing was launched


def test_varlen_append_validation_without_gpu(built_lib):
    import pli_hip
    L = pli_hip.lib()
    err = lambda: L.pli_last_error()  # noqa: E731
    for kw in (dict(batch=-1), dict(max_tokens=-1), dict(kv_heads=0), dict(head_dim=0), dict(num_blocks=-1),
               dict(max_blocks=-1)):
        assert _append(L, **kw) == EINVAL and b"bad shape" in err(), kw
    assert _append(L, dtype=9) == EINVAL and b"dtype" in err()
    assert _append(L, block_size=0) == EINVAL and b"block_size" in err()
    assert _append(L, block_size=1 << 20, max_blocks=1 << 11) == EINVAL and b"2^31" in err()
    for name in ("kn", "vn", "k", "v", "cu", "table", "lens", "strides"):
        assert _append(L, **{name: None}) == EINVAL and b"null" in err(), name
    assert _append(L, head_dim=12) == EINVAL and b"16-byte" in err()
    assert _append(L, k=ctypes.c_void_p(8)) == EINVAL and b"16-byte" in err()
    assert _append(L, strides=(ctypes.c_int64 * 10)(*([8] * 4 + [4] + [8] * 5))) == EINVAL and b"stride 4" in err()
    assert _append(L, max_blocks=0) == EINVAL and b"empty pool or table" in err()
    assert _append(L, num_blocks=0) == EINVAL and b"empty pool or table" in err()


def test_varlen_empty_calls_without_gpu(built_lib):
    """an empty call returns PLI_OK before any HIP call; its operands may be NULL"""
    import pli_hip
    L = pli_hip.lib()
    none = dict(q=None, k=None, v=None, o=None, cu=None, table=None, lens=None, strides=None)
    assert _attn(L, batch=0, **none) == OK
    assert _attn(L, max_tokens=0, **none) == OK
    assert _attn(L, batch=0, max_tokens=0, num_blocks=0, max_blocks=0, max_kv=0, **none) == OK
    assert L.pli_last_route() == b""
    none = dict(kn=None, vn=None, k=None, v=None, cu=None, table=None, lens=None, strides=None)
    assert _append(L, batch=0, **none) == OK
    assert _append(L, max_tokens=0, **none) == OK
    # the argument checks still come first
    assert _attn(L, batch=0, block_size=0, q=None) == EINVAL
    assert _append(L, max_tokens=0, block_size=-1) == EINVAL


def test_varlen_wrappers_refuse_cpu_tensors_and_bad_shapes(built_lib):
    import pli_hip
    q = torch.zeros(5, 8, 128, dtype=torch.bfloat16)
    pool = torch.zeros(8, 2, 16, 2, 128, dtype=torch.bfloat16)
    table = torch.zeros(2, 4, dtype=torch.int32)
    lens = torch.zeros(2, dtype=torch.int32)
    cu = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.attn_varlen_paged(q, pool[:, 0], pool[:, 1], table, lens, cu)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.kv_append_varlen_paged(q[:, :2], q[:, :2], pool[:, 0], pool[:, 1], table, lens, cu)
    for name in ("attn_varlen_paged", "kv_append_varlen_paged"):
        assert callable(getattr(pli_hip, name))
