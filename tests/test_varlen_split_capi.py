"""The split-K packed entry points of include/pli.h (pli_attn_varlen_paged_ws,
pli_attn_varlen_paged_fp8_ws, pli_attn_varlen_paged_split_plan,
pli_attn_varlen_paged_workspace_size) without a GPU: every argument check
answers PLI_EINVAL with its message before any HIP call, empty calls return
PLI_OK with NULL operands, the plan and the size agree, and the Python
wrappers and ch07.PagedKVCache refuse a bad workspace."""
from __future__ import annotations

import ctypes

import pytest
import torch

EINVAL, OK = 1000, 0
BF16 = 2
NAMES = {False: b"pli_attn_varlen_paged_ws", True: b"pli_attn_varlen_paged_fp8_ws"}


def _ws(L, fp8=False, **kw):
    """the _ws call on never-dereferenced pointers, one argument changed at a time; the defaults are a fast-path
    shape whose plan has 4 chunks of 64 keys"""
    p = ctypes.c_void_p(16)
    a = dict(q=p, k=p, v=p, o=p, cu=p, table=p, lens=p, batch=2, max_tokens=5, heads=8, kv_heads=2, head_dim=128,
             block_size=16, num_blocks=32, max_blocks=16, max_kv=256, strides=(ctypes.c_int64 * 10)(*([16] * 10)),
             scale=0.1, causal=1, dtype=BF16, split_keys=64, ws=p, ws_bytes=1 << 30)
    a.update(kw)
    head = (a["q"], a["k"], a["v"], a["o"], a["cu"], a["table"], a["lens"])
    tail = (a["batch"], a["max_tokens"], a["heads"], a["kv_heads"], a["head_dim"], a["block_size"], a["num_blocks"],
            a["max_blocks"], a["max_kv"], a["strides"], a["scale"], a["causal"], a["dtype"], a["split_keys"], a["ws"],
            a["ws_bytes"], None)
    if fp8:
        return L.pli_attn_varlen_paged_fp8_ws(*head, None, None, *tail)
    return L.pli_attn_varlen_paged_ws(*head, *tail)


@pytest.mark.parametrize("fp8", [False, True])
def test_ws_argument_validation_without_gpu(built_lib, fp8):
    import pli_hip
    L = pli_hip.lib()
    err = lambda: L.pli_last_error()  # noqa: E731
    name = NAMES[fp8]
    call = lambda **kw: _ws(L, fp8, **kw)  # noqa: E731
    # everything the plain calls reject, under this call's name
    for kw in (dict(batch=-1), dict(max_tokens=-1), dict(heads=0), dict(kv_heads=0), dict(head_dim=0), dict(max_kv=-1),
               dict(num_blocks=-1), dict(max_blocks=-1)):
        assert call(**kw) == EINVAL and name + b": bad shape" in err(), kw
    assert call(heads=6, kv_heads=4) == EINVAL and b"multiple of kv_heads" in err()
    assert call(dtype=7) == EINVAL and b"dtype" in err()
    for s in (float("nan"), float("inf")):
        assert call(scale=s) == EINVAL and b"non-finite scale" in err()
    for bs in (0, -16):
        assert call(block_size=bs) == EINVAL and b"block_size" in err()
    assert call(max_kv=257) == EINVAL and b"max_kv" in err()  # 16 blocks of 16 hold 256
    assert call(block_size=1 << 20, max_blocks=1 << 11) == EINVAL and b"2^31" in err()
    for arg in ("q", "k", "v", "o", "cu", "table", "lens", "strides"):
        assert call(**{arg: None}) == EINVAL and b"null" in err(), arg
    assert call(num_blocks=0) == EINVAL and b"empty pool" in err()
    assert call(max_blocks=0, max_kv=0) == EINVAL and b"empty pool or table" in err()
    # the generic path's limits are the plain call's (it runs the generic kernels as they are)
    assert call(head_dim=264) == EINVAL and b"head_dim" in err()
    assert call(head_dim=80, max_tokens=1 << 28) == EINVAL and b"grid too large" in err()
    # split_keys: negative, or not a multiple of 64
    for k in (-64, -1, 1, 32, 96, 100):
        assert call(split_keys=k) == EINVAL and name + b": split_keys" in err(), k
    # the workspace: NULL, short, misaligned -- only when the plan needs one
    need = L.pli_attn_varlen_paged_workspace_size(2, 5, 8, 2, 256, 128, 64)
    assert need == 4 * 5 * 8 * 130 * 4
    assert call(ws=None) == EINVAL and b"workspace of %d bytes needed" % need in err()
    assert call(ws_bytes=need - 1) == EINVAL and b"workspace of %d bytes needed, %d given" % (need, need - 1) in err()
    assert call(ws_bytes=0) == EINVAL and b"workspace of" in err()
    assert call(ws=ctypes.c_void_p(24)) == EINVAL and b"16-byte aligned" in err()
    # the split grid alone: (2^16 + 2) tiles x 2^14 chunks x 2 kv heads; the plain call's grid is small
    assert call(max_tokens=1 << 22, heads=2, kv_heads=2, block_size=1 << 10, max_blocks=1 << 10, max_kv=1 << 20,
                ) == EINVAL and name + b": grid too large" in err()
    assert L.pli_last_route() == b""  # nothing was launched


@pytest.mark.parametrize("fp8", [False, True])
def test_ws_empty_calls_without_gpu(built_lib, fp8):
    """an empty call returns PLI_OK before any HIP call; its operands and workspace may be NULL"""
    import pli_hip
    L = pli_hip.lib()
    none = dict(q=None, k=None, v=None, o=None, cu=None, table=None, lens=None, strides=None, ws=None, ws_bytes=0)
    assert _ws(L, fp8, batch=0, **none) == OK
    assert _ws(L, fp8, max_tokens=0, **none) == OK
    assert _ws(L, fp8, batch=0, max_tokens=0, num_blocks=0, max_blocks=0, max_kv=0, **none) == OK
    assert L.pli_last_route() == b""
    # the argument checks still come first
    assert _ws(L, fp8, batch=0, block_size=0, **none) == EINVAL
    assert _ws(L, fp8, batch=0, split_keys=65, **none) == EINVAL and b"split_keys" in L.pli_last_error()


def test_plan_call_and_workspace_size(built_lib):
    import pli_hip
    L = pli_hip.lib()
    span, splits = ctypes.c_int(-1), ctypes.c_int(-1)
    plan = lambda *a: L.pli_attn_varlen_paged_split_plan(*a, ctypes.byref(span), ctypes.byref(splits))  # noqa: E731
    assert plan(8, 1032, 32, 8, 32768, 128, 256) == OK and (span.value, splits.value) == (256, 128)
    assert L.pli_attn_varlen_paged_workspace_size(8, 1032, 32, 8, 32768, 128, 256) == 128 * 1032 * 32 * 130 * 4
    # the plan's own choice: a multiple of 64, a bounded number of chunks, the same whatever the batch is
    assert plan(8, 1032, 32, 8, 32768, 128, 0) == OK
    assert span.value % 64 == 0 and splits.value == -(-32768 // span.value) > 1
    chosen = (span.value, splits.value)
    assert pli_hip.attn_varlen_paged_split_plan(300, 1032, 32, 8, 32768, 128) == chosen
    assert pli_hip.attn_varlen_paged_workspace_bytes(8, 1032, 32, 8, 32768, 128) == chosen[1] * 1032 * 32 * 130 * 4
    # one chunk: no workspace
    assert plan(2, 5, 8, 2, 64, 128, 64) == OK and splits.value == 1
    assert L.pli_attn_varlen_paged_workspace_size(2, 5, 8, 2, 64, 128, 64) == 0
    assert plan(2, 5, 8, 2, 64, 128, 0) == OK and splits.value == 1
    # NULL outputs are allowed; bad arguments are PLI_EINVAL with the call's name
    assert L.pli_attn_varlen_paged_split_plan(2, 5, 8, 2, 64, 128, 64, None, None) == OK
    for bad in ((-1, 5, 8, 2, 64, 128, 64), (2, 5, 8, 3, 64, 128, 64), (2, 5, 8, 2, 64, 128, 63),
                (2, 5, 8, 2, 64, 128, -64), (2, 5, 8, 2, -1, 128, 0)):
        assert plan(*bad) == EINVAL and b"pli_attn_varlen_paged_split_plan" in L.pli_last_error(), bad
        assert L.pli_attn_varlen_paged_workspace_size(*bad) == 0


def test_wrappers_refuse_a_bad_workspace(built_lib):
    import pli_hip
    q = torch.zeros(5, 8, 128, dtype=torch.bfloat16)
    pool = torch.zeros(8, 2, 16, 2, 128, dtype=torch.bfloat16)
    pool8 = torch.zeros(8, 2, 16, 2, 128, dtype=torch.uint8)
    table = torch.zeros(2, 16, dtype=torch.int32)
    lens = torch.zeros(2, dtype=torch.int32)
    cu = torch.zeros(3, dtype=torch.int32)
    need = pli_hip.attn_varlen_paged_workspace_bytes(2, 5, 8, 2, 256, 128, 64)
    assert need == 4 * 5 * 8 * 130 * 4
    for fn, p in ((pli_hip.attn_varlen_paged, pool), (pli_hip.attn_varlen_paged_fp8, pool8)):
        args = (q, p[:, 0], p[:, 1], table, lens, cu)
        with pytest.raises(pli_hip.PliError, match="float32"):  # wrong dtype
            fn(*args, workspace=torch.zeros(need // 2, dtype=torch.bfloat16), split_keys=64)
        with pytest.raises(pli_hip.PliError, match="float32"):
            fn(*args, workspace=[0.0] * 8, split_keys=64)
        with pytest.raises(pli_hip.PliError, match=f"workspace of {need} bytes needed, {need - 4} given"):  # short
            fn(*args, workspace=torch.zeros(need // 4 - 1), split_keys=64)
        with pytest.raises(pli_hip.PliError, match="split_keys"):
            fn(*args, workspace=torch.zeros(need // 4), split_keys=100)
        with pytest.raises(pli_hip.PliError, match="workspace is a CPU tensor"):  # big enough, but on the host
            fn(*args, workspace=torch.zeros(need // 4), split_keys=64)
        with pytest.raises(pli_hip.PliError, match="CPU tensor"):  # workspace=None: today's call and today's refusal
            fn(*args)


@pytest.mark.parametrize("fp8", [False, True])
def test_paged_kv_cache_workspace_size_and_cpu_refusal(built_lib, fp8):
    import pli_hip
    from ch07 import PagedKVCache
    kw = dict(kv_dtype=torch.float8_e4m3fn) if fp8 else {}
    c = PagedKVCache(num_blocks=4096, block_size=16, num_layers=2, num_heads=8, head_dim=128, dtype=torch.bfloat16,
                     device="cpu", **kw)
    L = pli_hip.lib()
    assert c.packed_workspace_bytes(8, 1032, 32) == L.pli_attn_varlen_paged_workspace_size(8, 1032, 32, 8, 4096 * 16,
                                                                                          128, 0) > 0
    assert c.packed_workspace_bytes(8, 1032, 32, max_blocks=2048) == L.pli_attn_varlen_paged_workspace_size(
        8, 1032, 32, 8, 32768, 128, 0) > 0
    assert c.packed_workspace_bytes(8, 1032, 32, max_blocks=4) == 0  # 64 keys: one chunk
    with pytest.raises(pli_hip.PliError, match="no device pools"):
        c.packed_workspace(8, 1032, 32)
    c.allocate_blocks(1, 4)
    table, lens, cu = c.tables_packed([1], [4])
    x = torch.zeros(4, 32, 128, dtype=torch.bfloat16)
    with pytest.raises(pli_hip.PliError, match="no device pools"):  # as without a workspace
        c.attend_packed(0, x, table, lens, cu)
    with pytest.raises(pli_hip.PliError, match="no device pools"):
        c.attend_packed(0, x, table, lens, cu, workspace=torch.zeros(16))
    with pytest.raises(pli_hip.PliError, match="no device pools"):
        c.attend_packed(0, x, table, lens, cu, causal=False, workspace=torch.zeros(16))
