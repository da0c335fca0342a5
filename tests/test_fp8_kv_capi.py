"""The fp8 KV-cache entry points of include/pli.h without a GPU: the argument
checks of tests/test_paged_capi.py and tests/test_varlen_capi.py for the four
*_fp8 calls (PLI_EINVAL with its message before any HIP call), NULL scales
accepted, empty calls returning PLI_OK with NULL operands, and the Python
wrappers refusing CPU tensors and pools of another dtype."""
from __future__ import annotations

import ctypes

import pytest
import torch

EINVAL, OK = 1000, 0
BF16 = 2
P = ctypes.c_void_p(16)  # never dereferenced: validation fails first


def i64(n, v=16, **at):
    s = [v] * n
    for i, x in at.items():
        s[int(i[1:])] = x
    return (ctypes.c_int64 * n)(*s)


def _decode(L, **kw):
    a = dict(q=P, k=P, v=P, o=P, table=P, lens=P, ks=P, vs=P, batch=2, heads=8, kv_heads=2, n_q=1, head_dim=128,
             block_size=16, num_blocks=32, max_blocks=4, max_kv=64, strides=i64(12), scale=0.1, causal=1, n_kv_add=0,
             ws=None, ws_bytes=0, dtype=BF16)
    a.update(kw)
    return L.pli_attn_decode_paged_fp8(a["q"], a["k"], a["v"], a["o"], a["table"], a["lens"], a["ks"], a["vs"], a["batch"],
                                       a["heads"], a["kv_heads"], a["n_q"], a["head_dim"], a["block_size"],
                                       a["num_blocks"], a["max_blocks"], a["max_kv"], a["strides"], a["scale"],
                                       a["causal"], a["n_kv_add"], a["ws"], a["ws_bytes"], a["dtype"], None)


def _append(L, **kw):
    a = dict(kn=P, vn=P, k=P, v=P, table=P, lens=P, ks=P, vs=P, batch=2, n_new=1, kv_heads=2, head_dim=128,
             block_size=16, num_blocks=32, max_blocks=4, strides=i64(12), dtype=BF16)
    a.update(kw)
    return L.pli_kv_append_paged_fp8(a["kn"], a["vn"], a["k"], a["v"], a["table"], a["lens"], a["ks"], a["vs"], a["batch"],
                                     a["n_new"], a["kv_heads"], a["head_dim"], a["block_size"], a["num_blocks"],
                                     a["max_blocks"], a["strides"], a["dtype"], None)


def _varlen(L, **kw):
    a = dict(q=P, k=P, v=P, o=P, cu=P, table=P, lens=P, ks=P, vs=P, batch=2, max_tokens=5, heads=8, kv_heads=2,
             head_dim=128, block_size=16, num_blocks=32, max_blocks=4, max_kv=64, strides=i64(10), scale=0.1, causal=1,
             dtype=BF16)
    a.update(kw)
    return L.pli_attn_varlen_paged_fp8(a["q"], a["k"], a["v"], a["o"], a["cu"], a["table"], a["lens"], a["ks"], a["vs"],
                                       a["batch"], a["max_tokens"], a["heads"], a["kv_heads"], a["head_dim"],
                                       a["block_size"], a["num_blocks"], a["max_blocks"], a["max_kv"], a["strides"],
                                       a["scale"], a["causal"], a["dtype"], None)


def _vappend(L, **kw):
    a = dict(kn=P, vn=P, k=P, v=P, cu=P, table=P, lens=P, ks=P, vs=P, batch=2, max_tokens=5, kv_heads=2, head_dim=128,
             block_size=16, num_blocks=32, max_blocks=4, strides=i64(10), dtype=BF16)
    a.update(kw)
    return L.pli_kv_append_varlen_paged_fp8(a["kn"], a["vn"], a["k"], a["v"], a["cu"], a["table"], a["lens"], a["ks"],
                                            a["vs"], a["batch"], a["max_tokens"], a["kv_heads"], a["head_dim"],
                                            a["block_size"], a["num_blocks"], a["max_blocks"], a["strides"], a["dtype"],
                                            None)


@pytest.fixture()
def L(built_lib):
    import pli_hip
    return pli_hip.lib()


def test_decode_argument_validation_without_gpu(L):
    err = L.pli_last_error
    for kw in (dict(batch=-1), dict(heads=0), dict(kv_heads=0), dict(n_q=-1), dict(head_dim=0), dict(max_kv=-1),
               dict(num_blocks=-1), dict(max_blocks=-1)):
        assert _decode(L, **kw) == EINVAL and b"pli_attn_decode_paged_fp8: bad shape" in err(), kw
    assert _decode(L, heads=6, kv_heads=4) == EINVAL and b"multiple of kv_heads" in err()
    assert _decode(L, dtype=7) == EINVAL and b"dtype" in err()
    for s in (float("nan"), float("inf")):
        assert _decode(L, scale=s) == EINVAL and b"non-finite scale" in err()
    for bs in (0, -16):
        assert _decode(L, block_size=bs) == EINVAL and b"block_size" in err()
    assert _decode(L, max_kv=65) == EINVAL and b"max_kv" in err()  # 4 blocks of 16 hold 64
    assert _decode(L, block_size=1 << 20, max_blocks=1 << 11, max_kv=0) == EINVAL and b"2^31" in err()
    for name in ("q", "k", "v", "o", "table", "lens", "strides"):
        assert _decode(L, **{name: None}) == EINVAL and b"null" in err(), name
    assert _decode(L, num_blocks=0) == EINVAL and b"empty pool" in err()
    # split-K needs its workspace (sized by the 16-bit call's function): refused when short, missing or misaligned,
    # with the scales given and with NULL scales alike
    shape = dict(batch=1, heads=32, kv_heads=8, max_blocks=2048, max_kv=32768, num_blocks=4096)
    need = L.pli_attn_decode_paged_workspace_size(1, 32, 8, 1, 32768, 128)
    assert need > 0
    for sc in (dict(), dict(ks=None, vs=None)):
        assert _decode(L, ws=P, ws_bytes=need - 1, **shape, **sc) == EINVAL and b"workspace" in err()
        assert _decode(L, ws=None, ws_bytes=need, **shape, **sc) == EINVAL and b"workspace" in err()
        assert _decode(L, ws=ctypes.c_void_p(24), ws_bytes=need, **shape, **sc) == EINVAL and b"16-byte aligned" in err()
    # a pool stride of 8 bytes is not the MFMA kernel's: no workspace is asked for, the generic limits apply
    assert _decode(L, head_dim=264) == EINVAL and b"head_dim" in err()
    assert _decode(L, strides=i64(12, s4=8), head_dim=264) == EINVAL and b"head_dim" in err()
    assert L.pli_last_route() == b""  # nothing was launched


def test_varlen_argument_validation_without_gpu(L):
    err = L.pli_last_error
    for kw in (dict(batch=-1), dict(max_tokens=-1), dict(heads=0), dict(kv_heads=0), dict(head_dim=0), dict(max_kv=-1),
               dict(num_blocks=-1), dict(max_blocks=-1)):
        assert _varlen(L, **kw) == EINVAL and b"pli_attn_varlen_paged_fp8: bad shape" in err(), kw
    assert _varlen(L, heads=6, kv_heads=4) == EINVAL and b"multiple of kv_heads" in err()
    assert _varlen(L, dtype=7) == EINVAL and b"dtype" in err()
    for s in (float("nan"), float("inf")):
        assert _varlen(L, scale=s) == EINVAL and b"non-finite scale" in err()
    for bs in (0, -16):
        assert _varlen(L, block_size=bs) == EINVAL and b"block_size" in err()
    assert _varlen(L, max_kv=65) == EINVAL and b"max_kv" in err()
    assert _varlen(L, block_size=1 << 20, max_blocks=1 << 11) == EINVAL and b"2^31" in err()
    for name in ("q", "k", "v", "o", "cu", "table", "lens", "strides"):
        assert _varlen(L, **{name: None}) == EINVAL and b"null" in err(), name
    assert _varlen(L, num_blocks=0) == EINVAL and b"empty pool" in err()
    assert _varlen(L, max_blocks=0, max_kv=0) == EINVAL and b"empty pool or table" in err()
    assert _varlen(L, head_dim=264) == EINVAL and b"head_dim" in err()
    assert _varlen(L, head_dim=80, max_tokens=1 << 28) == EINVAL and b"grid too large" in err()
    # the MFMA path's grid (2^29 tiles x 8 kv heads), with NULL scales too
    for sc in (dict(), dict(ks=None, vs=None)):
        assert _varlen(L, max_tokens=2 ** 31 - 1, heads=128, kv_heads=8, **sc) == EINVAL and b"grid too large" in err()
    assert L.pli_last_route() == b""


@pytest.mark.parametrize("call,n,first", [(_append, 12, "n_new"), (_vappend, 10, "max_tokens")])
def test_append_validation_without_gpu(L, call, n, first):
    err = L.pli_last_error
    name = b"pli_kv_append_paged_fp8" if call is _append else b"pli_kv_append_varlen_paged_fp8"
    for kw in (dict(batch=-1), {first: -1}, dict(kv_heads=0), dict(head_dim=0), dict(num_blocks=-1), dict(max_blocks=-1)):
        assert call(L, **kw) == EINVAL and name + b": bad shape" in err(), kw
    assert call(L, dtype=9) == EINVAL and b"dtype" in err()
    assert call(L, block_size=0) == EINVAL and b"block_size" in err()
    assert call(L, block_size=1 << 20, max_blocks=1 << 11) == EINVAL and b"2^31" in err()
    operands = ("kn", "vn", "k", "v", "table", "lens", "strides") + (("cu",) if call is _vappend else ())
    for op in operands:
        assert call(L, **{op: None}) == EINVAL and b"null" in err(), op
    assert call(L, head_dim=12) == EINVAL and b"8-element chunks" in err()
    assert call(L, k=ctypes.c_void_p(8)) == EINVAL and b"16-byte" in err()
    assert call(L, strides=i64(n, s4=4)) == EINVAL and b"stride 4" in err()
    assert call(L, max_blocks=0) == EINVAL and b"empty pool or table" in err()
    assert call(L, num_blocks=0) == EINVAL and b"empty pool or table" in err()
    assert L.pli_last_route() == b""


def test_empty_calls_without_gpu(L):
    """an empty call returns PLI_OK before any HIP call; its operands, the scales among them, may be NULL"""
    none = dict(q=None, k=None, v=None, o=None, table=None, lens=None, ks=None, vs=None, strides=None)
    assert _decode(L, batch=0, **none) == OK
    assert _decode(L, n_q=0, **none) == OK
    assert _decode(L, batch=0, num_blocks=0, max_blocks=0, max_kv=0, **none) == OK
    assert _varlen(L, batch=0, cu=None, **none) == OK
    assert _varlen(L, max_tokens=0, cu=None, **none) == OK
    assert L.pli_last_route() == b""
    none = dict(kn=None, vn=None, k=None, v=None, table=None, lens=None, ks=None, vs=None, strides=None)
    assert _append(L, batch=0, **none) == OK
    assert _append(L, n_new=0, **none) == OK
    assert _vappend(L, batch=0, cu=None, **none) == OK
    assert _vappend(L, max_tokens=0, cu=None, **none) == OK
    # the argument checks still come first
    assert _decode(L, batch=0, block_size=0, q=None) == EINVAL
    assert _varlen(L, batch=0, block_size=0, q=None) == EINVAL
    assert _append(L, n_new=0, block_size=-1) == EINVAL
    assert _vappend(L, max_tokens=0, block_size=-1) == EINVAL


def test_wrappers_refuse_cpu_tensors_and_other_pools(built_lib):
    import pli_hip
    q = torch.zeros(2, 1, 8, 128, dtype=torch.bfloat16)
    pool = torch.zeros(8, 2, 16, 2, 128, dtype=torch.float8_e4m3fn)
    table = torch.zeros(2, 4, dtype=torch.int32)
    lens = torch.zeros(2, dtype=torch.int32)
    cu = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.attn_decode_paged_fp8(q, pool[:, 0], pool[:, 1], table, lens)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.kv_append_paged_fp8(q[:, :, :2], q[:, :, :2], pool[:, 0], pool[:, 1], table, lens)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.attn_varlen_paged_fp8(q[:, 0], pool[:, 0], pool[:, 1], table, lens, cu)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.kv_append_varlen_paged_fp8(q[:, 0, :2], q[:, 0, :2], pool[:, 0], pool[:, 1], table, lens, cu)
    # the 16-bit calls keep their mixed-dtype check: an fp8 pool is not theirs
    with pytest.raises(pli_hip.PliError, match="CPU tensor|mixed dtypes"):
        pli_hip.attn_decode_paged(q, pool[:, 0], pool[:, 1], table, lens)
    assert pli_hip.FP8_POOL_DTYPES == (torch.float8_e4m3fn, torch.uint8)
