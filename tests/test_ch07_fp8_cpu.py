"""ch07.PagedKVCache(kv_dtype=...) without a GPU: kv_dtype=None is the cache
as it was, an fp8 cache reports 1 byte per element and carries its scales,
construction works off-device, and set_scales checks what it is given."""
from __future__ import annotations

import pytest
import torch

FP8 = torch.float8_e4m3fn
SHAPE = dict(num_blocks=10, block_size=16, num_layers=3, num_heads=4, head_dim=64)


def make(**kw):
    from ch07 import PagedKVCache
    return PagedKVCache(**SHAPE, device="cpu", **kw)


def test_kv_dtype_none_is_the_cache_as_it_was():
    from ch07 import PagedKVCache
    old, new = PagedKVCache(10, 16, 3, 4, 64, torch.float16, "cpu"), make(kv_dtype=None)
    for c in (old, new):
        c.allocate_blocks(1, 40)
        assert c.kv_dtype is None and c.k_scale is None and c.v_scale is None and c.k_cache is None
    assert old.get_memory_usage() == new.get_memory_usage()
    u = new.get_memory_usage()
    assert u["bytes_per_block"] == 2 * 3 * 16 * 4 * 64 * 2 and u["used_blocks"] == 3 and u["free_blocks"] == 7
    assert u["total_mb"] == 10 * u["bytes_per_block"] / (1024 * 1024)
    with pytest.raises(ValueError, match="fp8 cache"):
        new.set_scales(0, [1.0] * 4, [1.0] * 4)
    with pytest.raises(TypeError):
        PagedKVCache(10, 16, 3, 4, 64, torch.float16, "cpu", FP8)  # keyword only


def test_kv_dtype_is_a_keyword_of_the_class_call_not_of_init():
    """the reference's constructor keeps its parameter list (tests/test_ch07_packed_cpu.py pins it); kv_dtype is
    taken where the class is called, for subclasses too"""
    import inspect

    from ch07 import PagedKVCache
    assert "kv_dtype" not in inspect.signature(PagedKVCache.__init__).parameters
    assert PagedKVCache.kv_dtype is None

    class Sub(PagedKVCache):
        pass

    c = Sub(**SHAPE, device="cpu", kv_dtype=FP8)
    assert type(c) is Sub and c.kv_dtype is FP8 and c.k_scale.shape == (3, 4) and Sub.kv_dtype is None
    assert make().kv_dtype is None  # one instance's choice is not the next one's


def test_fp8_cache_halves_the_bytes():
    ref, c = make(), make(kv_dtype=FP8)
    for x in (ref, c):
        x.allocate_blocks(1, 40)
    a, b = ref.get_memory_usage(), c.get_memory_usage()
    assert b["bytes_per_block"] * 2 == a["bytes_per_block"] and b["total_mb"] * 2 == a["total_mb"]
    assert b["used_mb"] * 2 == a["used_mb"]
    assert {k: v for k, v in a.items() if "bytes" not in k and "mb" not in k} == \
           {k: v for k, v in b.items() if "bytes" not in k and "mb" not in k}
    with pytest.raises(ValueError, match="kv_dtype"):
        make(kv_dtype=torch.float8_e5m2)
    with pytest.raises(ValueError, match="kv_dtype"):
        make(kv_dtype=torch.float16)


def test_off_device_construction_and_the_allocator():
    import pli_hip
    c = make(kv_dtype=FP8, dtype=torch.bfloat16)
    assert c.kv_dtype is FP8 and c.dtype is torch.bfloat16 and c.k_cache is None and c.v_cache is None
    for s in (c.k_scale, c.v_scale):
        assert s.shape == (3, 4) and s.dtype == torch.float32 and s.device.type == "cpu" and bool((s == 1).all())
    t = c.allocate_blocks(7, 33)
    assert t.num_blocks() == 3 and c.get_num_free_blocks() == 7
    c.extend_blocks(7, 16)
    assert c.block_tables[7].num_blocks() == 4 and c.free_blocks_for_request(7) == 4
    c.allocate_blocks(1, 4)
    table, lens, cu = c.tables_packed([1], [4])
    x = torch.zeros(4, 4, 64, dtype=torch.bfloat16)
    with pytest.raises(pli_hip.PliError, match="no device pools"):
        c.append_packed(0, x, x, table, lens, cu)
    with pytest.raises(pli_hip.PliError, match="no device pools"):
        c.attend(0, x[None], table, lens)


def test_set_scales_checks_its_arguments():
    c = make(kv_dtype=FP8)
    c.set_scales(1, [0.5, 1.5, 2.0, 3.0], torch.tensor([0.25, 0.75, 1.25, 1.75], dtype=torch.float64))
    assert c.k_scale[1].tolist() == [0.5, 1.5, 2.0, 3.0] and c.v_scale[1].tolist() == [0.25, 0.75, 1.25, 1.75]
    assert bool((c.k_scale[0] == 1).all()) and bool((c.v_scale[2] == 1).all())  # the other layers keep theirs
    before = (c.k_scale.clone(), c.v_scale.clone())
    good = [1.0] * 4
    for bad in ([1.0] * 3, [[1.0] * 4], 1.0):
        with pytest.raises(ValueError, match="shape"):
            c.set_scales(0, bad, good)
        with pytest.raises(ValueError, match="shape"):
            c.set_scales(0, good, bad)
    for bad in ([1.0, 0.0, 1.0, 1.0], [1.0, -2.0, 1.0, 1.0], [float("inf")] + [1.0] * 3, [float("nan")] + [1.0] * 3):
        with pytest.raises(ValueError, match="finite and > 0"):
            c.set_scales(0, bad, good)
        with pytest.raises(ValueError, match="finite and > 0"):
            c.set_scales(0, good, bad)
    for layer in (-1, 3):
        with pytest.raises(IndexError):
            c.set_scales(layer, good, good)
    assert torch.equal(c.k_scale, before[0]) and torch.equal(c.v_scale, before[1])  # a refused call changes nothing


def test_the_explanation_names_the_one_byte_cache():
    from ch07.paged_memory import explain_paged_memory
    text = explain_paged_memory()
    assert "float8_e4m3fn" in text and "twice the tokens" in text and "pli_attn_decode_paged" in text
