"""The MXFP4 KV-cache entry points of include/pli.h and the cache option without a
GPU: every argument rule of the three calls with its message (PLI_EINVAL before
any HIP call, the order of the fp8 calls plus head_dim % 32, the scale pools and
their strides), empty calls with NULL operands, the wrappers refusing CPU
tensors, and ch07.PagedKVCache(kv_dtype=torch.float4_e2m1fn_x2) off-device."""
from __future__ import annotations

import ctypes

import pytest
import torch

from test_fp8_kv_capi import BF16, EINVAL, OK, P, i64

MX = torch.float4_e2m1fn_x2
NAMES = {"decode": b"pli_attn_decode_paged_mxfp4", "append": b"pli_kv_append_paged_mxfp4",
         "vappend": b"pli_kv_append_varlen_paged_mxfp4"}


def call(L, which, **kw):
    a = dict(q=P, k=P, v=P, o=P, ke=P, ve=P, cu=P, table=P, lens=P, batch=2, heads=8, kv_heads=2, n=1, head_dim=128,
             block_size=16, num_blocks=32, max_blocks=4, max_kv=64, strides=i64(10 if which == "vappend" else 12),
             exp_strides=i64(6, 4), scale=0.1, ws=None, ws_bytes=0, dtype=BF16)
    a.update(kw)
    tail = (a["head_dim"], a["block_size"], a["num_blocks"], a["max_blocks"])
    if which == "decode":
        return L.pli_attn_decode_paged_mxfp4(a["q"], a["k"], a["v"], a["o"], a["table"], a["lens"], a["ke"], a["ve"],
                                             a["batch"], a["heads"], a["kv_heads"], a["n"], *tail, a["max_kv"],
                                             a["strides"], a["exp_strides"], a["scale"], 1, 0, a["ws"], a["ws_bytes"],
                                             a["dtype"], None)
    if which == "append":
        return L.pli_kv_append_paged_mxfp4(a["q"], a["o"], a["k"], a["v"], a["ke"], a["ve"], a["table"], a["lens"],
                                           a["batch"], a["n"], a["kv_heads"], *tail, a["strides"], a["exp_strides"],
                                           a["dtype"], None)
    return L.pli_kv_append_varlen_paged_mxfp4(a["q"], a["o"], a["k"], a["v"], a["ke"], a["ve"], a["cu"], a["table"],
                                              a["lens"], a["batch"], a["n"], a["kv_heads"], *tail, a["strides"],
                                              a["exp_strides"], a["dtype"], None)


@pytest.fixture()
def L(built_lib):
    import pli_hip
    return pli_hip.lib()


# (arguments, message), in the order the calls check them: each row also carries the fault of the row after it
# (where one call can hold both), so the earlier message winning shows the order
SHARED = [(dict(batch=-1, dtype=9), b": bad shape"), (dict(n=-1), b": bad shape"), (dict(kv_heads=0), b": bad shape"),
          (dict(num_blocks=-1), b": bad shape"), (dict(dtype=9, head_dim=48), b"bad dtype"),
          (dict(head_dim=48, block_size=0), b"multiple of the MX block of 32"),
          (dict(block_size=0, k=None), b"block_size"), (dict(block_size=1 << 20, max_blocks=1 << 11, max_kv=0, k=None), b"2^31"),
          (dict(ke=None, num_blocks=0), b"null"), (dict(ve=None), b"null"), (dict(exp_strides=None), b"null"),
          (dict(k=None), b"null"), (dict(table=None), b"null"), (dict(strides=None), b"null"),
          (dict(num_blocks=0, exp_strides=i64(6, 3)), b"empty pool or table"),
          (dict(exp_strides=i64(6, 4, s4=3)), b"scale-pool stride is below head_dim / 32 = 4")]
ONLY = {"decode": [(dict(heads=6, kv_heads=4, dtype=9), b"multiple of kv_heads"), (dict(scale=float("nan")), b"non-finite scale"),
                   (dict(max_kv=65), b"max_kv"), (dict(head_dim=288, exp_strides=i64(6)), b"head_dim 288 > 256"),
                   (dict(batch=1, heads=32, kv_heads=8, max_blocks=2048, max_kv=32768, num_blocks=4096, ws=P, ws_bytes=64),
                    b"workspace of"),
                   (dict(batch=1, heads=32, kv_heads=8, max_blocks=2048, max_kv=32768, num_blocks=4096,
                         ws=ctypes.c_void_p(24), ws_bytes=1 << 30), b"16-byte aligned")],
        "append": [(dict(k=ctypes.c_void_p(8)), b"16-byte aligned"), (dict(strides=i64(12, s0=4)), b"stride 0 not a multiple of 8"),
                   (dict(strides=i64(12, s4=6)), b"stride 4 not a multiple of 4")],
        "vappend": [(dict(cu=None), b"null"), (dict(strides=i64(10, s9=4)), b"stride 9 not a multiple of 8"),
                    (dict(strides=i64(10, s3=2)), b"stride 3 not a multiple of 4")]}


@pytest.mark.parametrize("which", NAMES)
def test_argument_rules_without_gpu(L, which):
    for kw, msg in SHARED + ONLY[which]:
        assert call(L, which, **kw) == EINVAL and NAMES[which] in L.pli_last_error() and msg in L.pli_last_error(), (kw, L.pli_last_error())
    assert L.pli_last_route() == b""  # nothing was launched


@pytest.mark.parametrize("which", NAMES)
def test_empty_calls_without_gpu(L, which):
    """an empty call returns PLI_OK before any HIP call, its operands (the scale pools among them) may be NULL; the
    argument checks still come first"""
    none = dict(q=None, k=None, v=None, o=None, ke=None, ve=None, cu=None, table=None, lens=None, strides=None,
                exp_strides=None)
    assert call(L, which, batch=0, **none) == OK and call(L, which, n=0, **none) == OK
    assert call(L, which, batch=0, num_blocks=0, max_blocks=0, max_kv=0, **none) == OK
    assert call(L, which, n=0, head_dim=48, **none) == EINVAL and call(L, which, batch=0, block_size=-1, **none) == EINVAL
    assert L.pli_last_route() == b""


def test_wrappers_refuse_cpu_tensors(built_lib):
    import pli_hip
    q = torch.zeros(2, 1, 8, 128, dtype=torch.bfloat16)
    codes, exps = torch.zeros(8, 16, 2, 64, dtype=torch.uint8), torch.zeros(8, 16, 2, 4, dtype=torch.uint8)
    table, lens, cu = (torch.zeros(s, dtype=torch.int32) for s in ((2, 4), (2,), (3,)))
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.attn_decode_paged_mxfp4(q, codes, codes, exps, exps, table, lens)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.kv_append_paged_mxfp4(q[:, :, :2], q[:, :, :2], codes, codes, exps, exps, table, lens)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.kv_append_varlen_paged_mxfp4(q[:, 0, :2], q[:, 0, :2], codes, codes, exps, exps, table, lens, cu)


# ------------------------------------------------------------ the cache option --
SHAPE = dict(num_blocks=10, block_size=16, num_layers=3, num_heads=4, head_dim=128)


def test_cache_option_off_device():
    from ch07 import PagedKVCache
    c = PagedKVCache(**SHAPE, device="cpu", kv_dtype=MX)
    assert c.kv_dtype is MX and c.k_cache is None and c.k_exp_cache is None and c.k_scale is None
    assert c.pool_shapes() == ((10, 3, 16, 4, 64), (10, 3, 16, 4, 4))
    ref = PagedKVCache(**SHAPE, device="cpu")
    assert ref.kv_dtype is None and ref.pool_shapes() == ((10, 3, 16, 4, 128), None)  # no leak between instances
    ratio = c.get_memory_usage()["bytes_per_block"] / ref.get_memory_usage()["bytes_per_block"]
    assert ratio == (128 / 2 + 128 / 32) / (2 * 128)
    with pytest.raises(ValueError, match="fp8 cache"):
        c.set_scales(0, [1.0] * 4, [1.0] * 4)
    for method, args in ((c.packed_workspace_bytes, (2, 8, 8)), (c.packed_workspace, (2, 8, 8)),
                         (c.attend_packed, (0, None, None, None, None))):
        with pytest.raises(NotImplementedError, match="kv_dtype"):
            method(*args)
    with pytest.raises(NotImplementedError, match="kv_dtype"):
        c.attend_packed(0, None, None, None, None, workspace=torch.zeros(1))
    for bad in (torch.float8_e5m2, torch.float16):
        with pytest.raises(ValueError, match="kv_dtype"):
            PagedKVCache(**SHAPE, device="cpu", kv_dtype=bad)
    with pytest.raises(ValueError, match="head_dim % 32"):
        PagedKVCache(10, 16, 3, 4, 48, device="cpu", kv_dtype=MX)
