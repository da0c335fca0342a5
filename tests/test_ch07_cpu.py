"""ch07.PagedKVCache: the allocator half, on device="cpu" (the behaviour of the
reference's ch07/paged_memory.py:53-137; which free block a request gets is
unspecified there -- it pops from a set -- and here)."""
from __future__ import annotations

import subprocess
import sys

import pytest
import torch

from conftest import PKG


def make(num_blocks=10, block_size=16, num_layers=2, num_heads=4, head_dim=64, **kw):
    from ch07 import PagedKVCache
    return PagedKVCache(num_blocks=num_blocks, block_size=block_size, num_layers=num_layers, num_heads=num_heads,
                        head_dim=head_dim, device="cpu", **kw)


def test_public_names_and_attributes():
    import ch07
    from ch07.paged_memory import BlockTable, PagedKVCache, explain_paged_memory
    assert ch07.PagedKVCache is PagedKVCache and ch07.BlockTable is BlockTable
    c = make(num_blocks=6, block_size=8, num_layers=3, num_heads=2, head_dim=32, dtype=torch.bfloat16)
    assert (c.num_blocks, c.block_size, c.num_layers, c.num_heads, c.head_dim, c.dtype, c.device) == (
        6, 8, 3, 2, 32, torch.bfloat16, "cpu")
    assert c.free_blocks == set(range(6)) and c.block_tables == {}
    assert c.k_cache is None and c.v_cache is None  # the pools exist only on a device
    assert make().dtype == torch.float16          # the reference's default
    t = BlockTable(request_id=3)
    assert (t.request_id, t.block_indices, t.num_tokens, t.num_blocks()) == (3, [], 0, 0)
    assert isinstance(explain_paged_memory(), str) and len(explain_paged_memory()) > 200


@pytest.mark.parametrize("tokens,blocks", [(1, 1), (16, 1), (17, 2), (50, 4)])
def test_block_counts(tokens, blocks):
    c = make()
    t = c.allocate_blocks(request_id=1, num_tokens=tokens)
    assert t.request_id == 1 and t.num_tokens == tokens and t.num_blocks() == blocks
    assert len(set(t.block_indices)) == blocks and set(t.block_indices) <= set(range(10))
    assert c.block_tables[1] is t
    assert c.get_num_free_blocks() == 10 - blocks and c.free_blocks.isdisjoint(t.block_indices)


def test_extend_takes_a_page_only_across_a_boundary():
    c = make()
    c.allocate_blocks(1, 15)
    first = list(c.block_tables[1].block_indices)
    c.extend_blocks(1, 1)   # 16 tokens: still one page
    assert c.block_tables[1].block_indices == first and c.block_tables[1].num_tokens == 16
    c.extend_blocks(1, 1)   # 17: the boundary
    assert c.block_tables[1].num_blocks() == 2 and c.block_tables[1].block_indices[:1] == first
    c.extend_blocks(1, 30)  # 47: three pages
    assert c.block_tables[1].num_blocks() == 3 and c.block_tables[1].num_tokens == 47
    c.extend_blocks(1, 0)
    assert c.block_tables[1].num_blocks() == 3 and c.get_num_free_blocks() == 7
    assert len(set(c.block_tables[1].block_indices)) == 3


def test_free_returns_the_pages_for_reuse():
    c = make(num_blocks=4)
    a = c.allocate_blocks(1, 33)  # 3 pages
    held = set(a.block_indices)
    c.allocate_blocks(2, 5)
    assert c.get_num_free_blocks() == 0
    assert c.free_blocks_for_request(1) == 3
    assert 1 not in c.block_tables and c.free_blocks == held
    assert c.free_blocks_for_request(1) == 0 and c.free_blocks_for_request(99) == 0  # unknown: nothing freed
    b = c.allocate_blocks(3, 48)
    assert set(b.block_indices) == held and c.get_num_free_blocks() == 0


def test_exhaustion_and_unknown_request():
    c = make(num_blocks=3)
    c.allocate_blocks(1, 32)
    with pytest.raises(RuntimeError, match="Not enough free blocks"):
        c.allocate_blocks(2, 33)
    assert 2 not in c.block_tables and c.get_num_free_blocks() == 1  # a refused request takes nothing
    c.extend_blocks(1, 16)
    with pytest.raises(RuntimeError, match="Not enough free blocks"):
        c.extend_blocks(1, 1)
    assert c.block_tables[1].num_tokens == 48 and c.block_tables[1].num_blocks() == 3
    with pytest.raises(KeyError):
        c.extend_blocks(7, 1)


def test_memory_usage_arithmetic():
    c = make(num_blocks=100, block_size=16, num_layers=32, num_heads=32, head_dim=128)
    c.allocate_blocks(1, 50)   # 4 pages
    c.allocate_blocks(2, 100)  # 7 pages
    u = c.get_memory_usage()
    per_block = 2 * 32 * 16 * 32 * 128 * 2  # K and V x layers x tokens x heads x dim x 2 bytes
    assert u == {"total_blocks": 100, "used_blocks": 11, "free_blocks": 89, "block_size_tokens": 16,
                 "bytes_per_block": per_block, "total_mb": 100 * per_block / 1024 / 1024,
                 "used_mb": 11 * per_block / 1024 / 1024, "utilization": 0.11}
    assert list(u) == ["total_blocks", "used_blocks", "free_blocks", "block_size_tokens", "bytes_per_block", "total_mb",
                       "used_mb", "utilization"]
    assert make(num_blocks=0).get_memory_usage()["utilization"] == 0


def test_tables_on_the_host():
    """the packed table: int32, padded with a valid page, lengths = num_tokens"""
    c = make()
    c.allocate_blocks(5, 40)
    c.allocate_blocks(6, 3)
    c.allocate_blocks(7, 0)
    table, lens = c.tables([6, 5, 7])
    assert table.dtype == lens.dtype == torch.int32 and table.shape == (3, 3) and lens.tolist() == [3, 40, 0]
    assert table[1].tolist() == c.block_tables[5].block_indices
    assert table[0].tolist() == c.block_tables[6].block_indices * 3 and table[2].tolist() == [0, 0, 0]
    assert c.tables([5], max_blocks=8)[0].shape == (1, 8)
    with pytest.raises(ValueError):
        c.tables([5], max_blocks=2)
    with pytest.raises(KeyError):
        c.tables([42])


def test_device_half_needs_device_pools():
    import pli_hip
    c = make()
    c.allocate_blocks(1, 4)
    table, lens = c.tables([1])
    x = torch.zeros(1, 1, 4, 64, dtype=torch.float16)
    with pytest.raises(pli_hip.PliError):
        c.attend(0, x, table, lens)
    with pytest.raises(pli_hip.PliError):
        c.append(0, x, x, table, lens)


def test_import_does_not_reach_the_oracle():
    code = "import sys, ch07; assert 'oracle' not in sys.modules, 'ch07 imported the oracle'; print(ch07.__all__)"
    r = subprocess.run([sys.executable, "-c", code], cwd=PKG, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "PagedKVCache" in r.stdout
