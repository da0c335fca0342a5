"""ch07.PagedKVCache.tables_packed on device="cpu": the three tensors of a
packed (mixed) step, its errors, and the allocator interface it leaves
unchanged."""
from __future__ import annotations

import inspect

import pytest
import torch


def make(num_blocks=12, block_size=16, num_layers=2, num_heads=4, head_dim=64, **kw):
    from ch07 import PagedKVCache
    return PagedKVCache(num_blocks=num_blocks, block_size=block_size, num_layers=num_layers, num_heads=num_heads,
                        head_dim=head_dim, device="cpu", **kw)


def test_tables_packed_contents_and_shapes():
    c = make()
    for rid, n in ((1, 30), (2, 17), (3, 9)):
        c.allocate_blocks(rid, n)
    grow = [40, 1, 0]
    for rid, n in zip((1, 2, 3), grow):
        c.extend_blocks(rid, n)
    table, lens, cu = c.tables_packed([1, 2, 3], grow)
    assert all(t.dtype == torch.int32 and t.is_contiguous() for t in (table, lens, cu))
    assert table.shape == (3, 5) and lens.shape == (3,) and cu.shape == (4,)
    assert lens.tolist() == [70, 18, 9], "seq_lens already counts the step's tokens"
    assert cu.tolist() == [0, 40, 41, 41], "a request with no new token owns no packed row"
    t2, l2 = c.tables([1, 2, 3])
    assert torch.equal(table, t2) and torch.equal(lens, l2)  # the same table and lengths tables() gives
    for i, rid in enumerate((1, 2, 3)):
        pages = c.block_tables[rid].block_indices
        assert table[i, :len(pages)].tolist() == pages and set(table[i, len(pages):].tolist()) <= {pages[-1]}
    # the order given, a fixed width, counts that need not be what was extended (a chunk of a longer prompt)
    table, lens, cu = c.tables_packed([3, 1], [2, 16], max_blocks=7)
    assert table.shape == (2, 7) and lens.tolist() == [9, 70] and cu.tolist() == [0, 2, 18]
    table, lens, cu = c.tables_packed([], [])
    assert table.shape[0] == 0 and lens.shape == (0,) and cu.tolist() == [0]


def test_tables_packed_errors():
    c = make()
    c.allocate_blocks(1, 40)
    with pytest.raises(KeyError):
        c.tables_packed([1, 99], [1, 1])  # an unknown request
    with pytest.raises(ValueError, match="narrower"):
        c.tables_packed([1], [1], max_blocks=2)  # 40 tokens hold 3 blocks
    with pytest.raises(ValueError, match="new_tokens"):
        c.tables_packed([1], [1, 2])
    with pytest.raises(ValueError, match="new_tokens"):
        c.tables_packed([1], [-1])


def test_packed_methods_need_device_pools():
    import pli_hip
    c = make()
    c.allocate_blocks(1, 4)
    table, lens, cu = c.tables_packed([1], [4])
    x = torch.zeros(4, 4, 64, dtype=torch.float16)
    with pytest.raises(pli_hip.PliError, match="no device pools"):
        c.append_packed(0, x, x, table, lens, cu)
    with pytest.raises(pli_hip.PliError, match="no device pools"):
        c.attend_packed(0, x, table, lens, cu)


def test_allocator_interface_is_unchanged():
    from ch07 import PagedKVCache
    from ch07.paged_memory import explain_paged_memory
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(PagedKVCache.__init__) == ["self", "num_blocks", "block_size", "num_layers", "num_heads", "head_dim",
                                          "dtype", "device"]
    assert sig(PagedKVCache.allocate_blocks) == ["self", "request_id", "num_tokens"]
    assert sig(PagedKVCache.extend_blocks) == ["self", "request_id", "new_tokens"]
    assert sig(PagedKVCache.free_blocks_for_request) == ["self", "request_id"]
    assert sig(PagedKVCache.tables) == ["self", "request_ids", "max_blocks"]
    assert sig(PagedKVCache.append) == ["self", "layer", "k_new", "v_new", "block_table", "seq_lens"]
    assert sig(PagedKVCache.attend) == ["self", "layer", "q", "block_table", "seq_lens", "n_kv_add", "causal"]
    assert sig(PagedKVCache.tables_packed) == ["self", "request_ids", "new_tokens", "max_blocks"]
    assert sig(PagedKVCache.append_packed) == ["self", "layer", "k_new", "v_new", "block_table", "seq_lens",
                                               "cu_seqlens_q"]
    assert sig(PagedKVCache.attend_packed) == ["self", "layer", "q", "block_table", "seq_lens", "cu_seqlens_q", "causal"]
    # tables_packed allocates and frees nothing
    c = make()
    c.allocate_blocks(1, 20)
    before = (set(c.free_blocks), list(c.block_tables[1].block_indices), c.block_tables[1].num_tokens, c.get_memory_usage())
    c.tables_packed([1], [5])
    assert before == (set(c.free_blocks), list(c.block_tables[1].block_indices), c.block_tables[1].num_tokens,
                      c.get_memory_usage())
    assert "pli_attn_varlen_paged" in explain_paged_memory() and "cu_seqlens_q" in explain_paged_memory()
