"""The paged entry points of include/pli.h without a GPU: every argument
check answers PLI_EINVAL with its message before any HIP call, empty outputs
return PLI_OK with NULL operands, and the Python wrappers refuse CPU tensors.
(tests/test_capi.py derives the export list from the header; this file covers
what the new calls validate.)"""
from __future__ import annotations

import ctypes

import pytest
import torch

EINVAL, OK = 1000, 0
BF16 = 2


def _paged(L, **kw):
    """pli_attn_decode_paged on never-dereferenced pointers, one argument changed at a time"""
    p = ctypes.c_void_p(16)
    a = dict(q=p, k=p, v=p, o=p, table=p, lens=p, batch=2, heads=8, kv_heads=2, n_q=1, head_dim=128, block_size=16,
             num_blocks=32, max_blocks=4, max_kv=64, strides=(ctypes.c_int64 * 12)(*([8] * 12)), scale=0.1, causal=1,
             n_kv_add=0, ws=None, ws_bytes=0, dtype=BF16)
    a.update(kw)
    return L.pli_attn_decode_paged(a["q"], a["k"], a["v"], a["o"], a["table"], a["lens"], a["batch"], a["heads"],
                                   a["kv_heads"], a["n_q"], a["head_dim"], a["block_size"], a["num_blocks"],
                                   a["max_blocks"], a["max_kv"], a["strides"], a["scale"], a["causal"], a["n_kv_add"],
                                   a["ws"], a["ws_bytes"], a["dtype"], None)


def _append(L, **kw):
    p = ctypes.c_void_p(16)
    a = dict(kn=p, vn=p, k=p, v=p, table=p, lens=p, batch=2, n_new=1, kv_heads=2, head_dim=128, block_size=16,
             num_blocks=32, max_blocks=4, strides=(ctypes.c_int64 * 12)(*([8] * 12)), dtype=BF16)
    a.update(kw)
    return L.pli_kv_append_paged(a["kn"], a["vn"], a["k"], a["v"], a["table"], a["lens"], a["batch"], a["n_new"],
                                 a["kv_heads"], a["head_dim"], a["block_size"], a["num_blocks"], a["max_blocks"],
                                 a["strides"], a["dtype"], None)


def test_paged_argument_validation_without_gpu(built_lib):
    import pli_hip
    L = pli_hip.lib()
    err = lambda: L.pli_last_error()  # noqa: E731
    # bad shapes
    for kw in (dict(batch=-1), dict(heads=0), dict(kv_heads=0), dict(n_q=-1), dict(head_dim=0), dict(max_kv=-1),
               dict(num_blocks=-1), dict(max_blocks=-1)):
        assert _paged(L, **kw) == EINVAL and b"bad shape" in err(), kw
    assert _paged(L, heads=6, kv_heads=4) == EINVAL and b"multiple of kv_heads" in err()
    assert _paged(L, dtype=7) == EINVAL and b"dtype" in err()
    for s in (float("nan"), float("inf")):
        assert _paged(L, scale=s) == EINVAL and b"non-finite scale" in err()
    for bs in (0, -16):
        assert _paged(L, block_size=bs) == EINVAL and b"block_size" in err()
    assert _paged(L, max_kv=65) == EINVAL and b"max_kv" in err()  # 4 blocks of 16 hold 64
    # null pointers, each operand
    for name in ("q", "k", "v", "o", "table", "lens", "strides"):
        assert _paged(L, **{name: None}) == EINVAL and b"null" in err(), name
    assert _paged(L, num_blocks=0) == EINVAL and b"empty pool" in err()
    # split-K needs its workspace: refused, not silently single-split, when short or missing
    shape = dict(batch=1, heads=32, kv_heads=8, max_blocks=2048, max_kv=32768, num_blocks=4096)
    need = L.pli_attn_decode_paged_workspace_size(1, 32, 8, 1, 32768, 128)
    assert need == L.pli_attn_decode_workspace_size(1, 32, 8, 1, 32768, 128) > 0
    assert _paged(L, ws=ctypes.c_void_p(16), ws_bytes=need - 1, **shape) == EINVAL and b"workspace" in err()
    assert _paged(L, ws=None, ws_bytes=need, **shape) == EINVAL and b"workspace" in err()
    assert _paged(L, ws=ctypes.c_void_p(24), ws_bytes=need, **shape) == EINVAL and b"16-byte aligned" in err()
    # the generic path's limit
    assert _paged(L, head_dim=264) == EINVAL and b"head_dim" in err()


def test_paged_append_validation_without_gpu(built_lib):
    import pli_hip
    L = pli_hip.lib()
    err = lambda: L.pli_last_error()  # noqa: E731
    for kw in (dict(batch=-1), dict(n_new=-1), dict(kv_heads=0), dict(head_dim=0), dict(num_blocks=-1), dict(max_blocks=-1)):
        assert _append(L, **kw) == EINVAL and b"bad shape" in err(), kw
    assert _append(L, dtype=9) == EINVAL and b"dtype" in err()
    assert _append(L, block_size=0) == EINVAL and b"block_size" in err()
    for name in ("kn", "vn", "k", "v", "table", "lens", "strides"):
        assert _append(L, **{name: None}) == EINVAL and b"null" in err(), name
    assert _append(L, head_dim=12) == EINVAL and b"16-byte" in err()
    assert _append(L, k=ctypes.c_void_p(8)) == EINVAL and b"16-byte" in err()
    assert _append(L, strides=(ctypes.c_int64 * 12)(*([8] * 5 + [4] + [8] * 6))) == EINVAL and b"stride 5" in err()
    assert _append(L, max_blocks=0) == EINVAL and b"empty pool or table" in err()


def test_paged_empty_operands_without_gpu(built_lib):
    """an empty output returns PLI_OK before any HIP call; its operands may be NULL"""
    import pli_hip
    L = pli_hip.lib()
    none = dict(q=None, k=None, v=None, o=None, table=None, lens=None, strides=None)
    assert _paged(L, batch=0, **none) == OK
    assert _paged(L, n_q=0, **none) == OK
    assert _paged(L, batch=0, num_blocks=0, max_blocks=0, max_kv=0, **none) == OK
    assert L.pli_last_route() == b""
    none = dict(kn=None, vn=None, k=None, v=None, table=None, lens=None, strides=None)
    assert _append(L, batch=0, **none) == OK
    assert _append(L, n_new=0, **none) == OK
    # the argument checks still come first
    assert _paged(L, batch=0, block_size=0, **dict(q=None)) == EINVAL
    assert _append(L, n_new=0, block_size=-1) == EINVAL
    assert L.pli_attn_decode_paged_workspace_size(0, 8, 2, 1, 64, 128) == 0
    assert L.pli_attn_decode_paged_workspace_size(2, 8, 3, 1, 64, 128) == 0  # heads % kv_heads


def test_paged_wrappers_refuse_cpu_tensors(built_lib):
    import pli_hip
    q = torch.zeros(2, 1, 8, 128, dtype=torch.bfloat16)
    pool = torch.zeros(8, 2, 16, 2, 128, dtype=torch.bfloat16)
    table = torch.zeros(2, 4, dtype=torch.int32)
    lens = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.attn_decode_paged(q, pool[:, 0], pool[:, 1], table, lens)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.kv_append_paged(q[:, :, :2], q[:, :, :2], pool[:, 0], pool[:, 1], table, lens)
    assert pli_hip.attn_decode_paged_workspace_bytes(1, 32, 8, 1, 32768, 128) == 8 * 128 * 4 * (128 + 2) * 4
