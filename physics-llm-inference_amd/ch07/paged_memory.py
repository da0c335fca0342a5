"""Paged KV cache -- mirror of ``ch07/paged_memory.py``.

The allocator half keeps the reference's interface: ``BlockTable`` and
``PagedKVCache`` with the pools ``k_cache`` / ``v_cache`` laid out
[num_blocks, num_layers, block_size, num_heads, head_dim]
(``ch07/paged_memory.py:16-51``), a free set, one block table per request,
``allocate_blocks`` / ``extend_blocks`` / ``free_blocks_for_request`` and the
``get_memory_usage`` report (``:53-137``).

The reference stops at the bookkeeping: its text describes an attention
kernel that "reads from scattered blocks / uses block table for indirection"
(``:171-175``) and never writes one.  Here the pools can be written and
attended over in place, through ``pli_kv_append_paged`` and
``pli_attn_decode_paged`` (csrc/paged_attn.hip):

* ``tables(request_ids)`` packs the requests' block tables and lengths into
  device int32 tensors,
* ``append(layer, k_new, v_new, block_table, seq_lens)`` stores the newest
  tokens of every sequence,
* ``attend(layer, q, block_table, seq_lens)`` runs decode attention over each
  sequence's own pages and length,
* ``tables_packed`` / ``append_packed`` / ``attend_packed`` do the same for a
  mixed step -- every request brings its own number of new tokens, packed
  behind a ``cu_seqlens_q`` -- through ``pli_kv_append_varlen_paged`` and
  ``pli_attn_varlen_paged`` (csrc/varlen_attn.hip), one launch each.

No page is gathered into a contiguous tensor on the way.

``PagedKVCache(..., kv_dtype=torch.float8_e4m3fn)`` keeps the pools as 1-byte
OCP fp8 e4m3 codes with one fp32 scale per (layer, kv head) for K and for V
(``k_scale`` / ``v_scale``, ones until ``set_scales``): the same four methods
then quantise on append and attend through the ``*_fp8`` entry points, and the
same memory holds twice the tokens.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import torch

import pli_hip


@dataclass
class BlockTable:
    request_id: int
    block_indices: list[int] = field(default_factory=list)
    num_tokens: int = 0

    def num_blocks(self) -> int:
        return len(self.block_indices)


class _CacheOptions(type):
    """Construction options the reference's constructor does not have.
    ``PagedKVCache.__init__`` keeps the reference's parameter list exactly
    (tests/test_ch07_packed_cpu.py pins it), so the trailing keyword
    ``kv_dtype`` of ``PagedKVCache(..., kv_dtype=...)`` is taken here, at the
    call of the class, and is on the instance before ``__init__`` runs."""

    def __call__(cls, *args, kv_dtype: torch.dtype | None = None, **kwargs):
        if kv_dtype not in (None, torch.float8_e4m3fn):
            raise ValueError(f"kv_dtype must be None or torch.float8_e4m3fn, got {kv_dtype}")
        self = cls.__new__(cls)
        self.kv_dtype = kv_dtype
        self.__init__(*args, **kwargs)
        return self


def _workspace_keyword(method):
    """``attend_packed`` keeps its parameter list too (the same test pins it),
    so its trailing keyword ``workspace=`` is taken here, as ``kv_dtype`` is
    above: None (the default) is the method as written, a tensor goes to
    ``_attend_packed_ws`` with the method's own arguments."""
    @functools.wraps(method)
    def call(self, *args, workspace: torch.Tensor | None = None, **kwargs):
        if workspace is None:
            return method(self, *args, **kwargs)
        return self._attend_packed_ws(*args, workspace=workspace, **kwargs)
    return call


class PagedKVCache(metaclass=_CacheOptions):
    # None: the pools hold `dtype`; torch.float8_e4m3fn: 1-byte codes, `dtype` is q's (keyword of the class call)
    kv_dtype: torch.dtype | None = None

    def __init__(self, num_blocks: int, block_size: int, num_layers: int, num_heads: int, head_dim: int,
                 dtype: torch.dtype = torch.float16, device: str = "cuda"):
        kv_dtype = self.kv_dtype
        self.num_blocks = num_blocks
        self.block_size = block_size
        self.num_layers = num_layers
        self.num_heads = num_heads
        self.head_dim = head_dim
        self.dtype = dtype
        self.device = device

        self.free_blocks: set[int] = set(range(num_blocks))
        self.block_tables: dict[int, BlockTable] = {}

        # the pools exist only on a device (None otherwise, as in the reference)
        self.k_cache = self.v_cache = None
        on_device = torch.cuda.is_available() and torch.device(device).type == "cuda"
        if on_device:
            shape = (num_blocks, num_layers, block_size, num_heads, head_dim)
            self.k_cache = torch.zeros(shape, dtype=kv_dtype or dtype, device=device)
            self.v_cache = torch.zeros(shape, dtype=kv_dtype or dtype, device=device)
        # fp8 pools: value = code * scale[layer, kv head]; the scales live where the pools do (host copies off-device)
        self.k_scale = self.v_scale = None
        if kv_dtype is not None:
            self.k_scale = torch.ones(num_layers, num_heads, dtype=torch.float32, device=device if on_device else "cpu")
            self.v_scale = torch.ones_like(self.k_scale)

    # ------------------------------------------------------------ allocator --
    def _blocks_for(self, num_tokens: int) -> int:
        return -(-num_tokens // self.block_size)

    def _take(self, count: int, what: str) -> list[int]:
        if count > len(self.free_blocks):
            raise RuntimeError(f"Not enough free blocks{what}: need {count}, have {len(self.free_blocks)}")
        return [self.free_blocks.pop() for _ in range(count)]

    def allocate_blocks(self, request_id: int, num_tokens: int) -> BlockTable:
        pages = self._take(self._blocks_for(num_tokens), "")
        table = BlockTable(request_id=request_id, block_indices=pages, num_tokens=num_tokens)
        self.block_tables[request_id] = table
        return table

    def extend_blocks(self, request_id: int, new_tokens: int) -> None:
        if request_id not in self.block_tables:
            raise KeyError(f"Request {request_id} not found")
        table = self.block_tables[request_id]
        total = table.num_tokens + new_tokens
        # a page is taken only when the new tokens cross a block boundary
        grow = self._blocks_for(total) - self._blocks_for(table.num_tokens)
        table.block_indices.extend(self._take(grow, " for extension"))
        table.num_tokens = total

    def free_blocks_for_request(self, request_id: int) -> int:
        table = self.block_tables.pop(request_id, None)
        if table is None:
            return 0
        self.free_blocks.update(table.block_indices)
        return len(table.block_indices)

    def get_num_free_blocks(self) -> int:
        return len(self.free_blocks)

    def get_memory_usage(self) -> dict:
        free = len(self.free_blocks)
        used = self.num_blocks - free
        # K and V, every layer, 2 bytes per element (the reference's fp16 figure), 1 for an fp8 cache
        elem_bytes = 2 if self.kv_dtype is None else 1
        bytes_per_block = 2 * self.num_layers * self.block_size * self.num_heads * self.head_dim * elem_bytes
        mb = 1024 * 1024
        return {
            "total_blocks": self.num_blocks,
            "used_blocks": used,
            "free_blocks": free,
            "block_size_tokens": self.block_size,
            "bytes_per_block": bytes_per_block,
            "total_mb": self.num_blocks * bytes_per_block / mb,
            "used_mb": used * bytes_per_block / mb,
            "utilization": used / self.num_blocks if self.num_blocks > 0 else 0,
        }

    # ---------------------------------------------------------- device half --
    def _pools(self, layer: int):
        if self.k_cache is None:
            raise pli_hip.PliError("PagedKVCache has no device pools (created off-device)")
        if not 0 <= layer < self.num_layers:
            raise IndexError(f"layer {layer} outside [0, {self.num_layers})")
        # [num_blocks, block_size, heads, head_dim] views: the layer is in the page stride
        return self.k_cache[:, layer], self.v_cache[:, layer]

    def set_scales(self, layer: int, k_scale, v_scale) -> None:
        """Set an fp8 cache's per-kv-head scales of one layer, in place (so a
        captured graph sees them): each a tensor or sequence of num_heads
        finite values > 0.  Tokens already in the pool keep the codes they were
        stored with."""
        if self.kv_dtype is None:
            raise ValueError("set_scales needs an fp8 cache (kv_dtype=torch.float8_e4m3fn)")
        if not 0 <= layer < self.num_layers:
            raise IndexError(f"layer {layer} outside [0, {self.num_layers})")
        new = [torch.as_tensor(s, dtype=torch.float32).detach().cpu() for s in (k_scale, v_scale)]
        for name, t in zip(("k_scale", "v_scale"), new):
            if tuple(t.shape) != (self.num_heads,):
                raise ValueError(f"{name} needs shape ({self.num_heads},), got {tuple(t.shape)}")
            if not bool((torch.isfinite(t) & (t > 0)).all()):
                raise ValueError(f"{name} must be finite and > 0")
        self.k_scale[layer].copy_(new[0])
        self.v_scale[layer].copy_(new[1])

    def tables(self, request_ids, max_blocks: int | None = None):
        """(block_table int32 [B, max_blocks], seq_lens int32 [B]) of the given
        requests on the cache's device, in the order given.  seq_lens holds each
        request's ``num_tokens``.  Entries past a request's blocks repeat its last
        page (page 0 for a request without blocks), so every entry is a valid page
        index.  max_blocks: the table width, default the longest request's (at
        least 1); a fixed width keeps the tensors' shapes stable across steps."""
        rows = [self.block_tables[r] for r in request_ids]  # KeyError for an unknown request
        width = max([1] + [t.num_blocks() for t in rows]) if max_blocks is None else int(max_blocks)
        if any(t.num_blocks() > width for t in rows) or width < 1:
            raise ValueError(f"max_blocks {width} is narrower than a request's block table")
        host = torch.tensor([t.block_indices + [t.block_indices[-1] if t.block_indices else 0] *
                             (width - t.num_blocks()) for t in rows], dtype=torch.int32).reshape(len(rows), width)
        lens = torch.tensor([t.num_tokens for t in rows], dtype=torch.int32)
        dev = self.device if self.k_cache is None else self.k_cache.device
        return host.to(dev), lens.to(dev)

    def append(self, layer: int, k_new: torch.Tensor, v_new: torch.Tensor, block_table: torch.Tensor,
               seq_lens: torch.Tensor) -> None:
        """Store k_new / v_new [B, T, heads, head_dim] as the LAST T tokens of
        every sequence: token t of sequence b goes to position
        seq_lens[b] - T + t.  The order of a step is therefore extend_blocks(rid,
        T), tables(...), append, attend -- the lengths ``tables`` returns already
        count the new tokens."""
        k_pool, v_pool = self._pools(layer)
        start = seq_lens - k_new.shape[1]
        if self.kv_dtype is not None:
            pli_hip.kv_append_paged_fp8(k_new, v_new, k_pool, v_pool, block_table, start, self.k_scale[layer],
                                        self.v_scale[layer])
            return
        pli_hip.kv_append_paged(k_new, v_new, k_pool, v_pool, block_table, start)

    def attend(self, layer: int, q: torch.Tensor, block_table: torch.Tensor, seq_lens: torch.Tensor,
               n_kv_add: int = 0, causal: bool = True) -> torch.Tensor:
        """Attention of q [B, Sq, Hq, head_dim] over each sequence's first
        seq_lens[b] + n_kv_add tokens of this layer's pages, read in place;
        causal masks bottom-right per sequence.  Returns [B, Sq, Hq, head_dim]."""
        k_pool, v_pool = self._pools(layer)
        if self.kv_dtype is not None:
            return pli_hip.attn_decode_paged_fp8(q, k_pool, v_pool, block_table, seq_lens, self.k_scale[layer],
                                                 self.v_scale[layer], causal=causal, n_kv_add=n_kv_add)
        return pli_hip.attn_decode_paged(q, k_pool, v_pool, block_table, seq_lens, causal=causal,
                                         n_kv_add=n_kv_add)

    # ------------------------------------------- packed (mixed) steps --
    def tables_packed(self, request_ids, new_tokens, max_blocks: int | None = None):
        """(block_table, seq_lens, cu_seqlens_q) of a step in which request i
        brings ``new_tokens[i]`` tokens (any count, 0 for a request that sits the
        step out): ``tables(request_ids, max_blocks)`` plus cu_seqlens_q int32
        [B + 1], the running sum of new_tokens, so request i owns packed rows
        cu[i] .. cu[i+1] - 1.  seq_lens already counts the new tokens: the
        order of a step is extend_blocks(rid, n), tables_packed, append_packed,
        attend_packed."""
        new_tokens = [int(n) for n in new_tokens]
        if len(new_tokens) != len(request_ids) or any(n < 0 for n in new_tokens):
            raise ValueError("new_tokens needs one non-negative count per request")
        table, lens = self.tables(request_ids, max_blocks)
        cu = torch.tensor([0] + new_tokens, dtype=torch.int64).cumsum(0).to(torch.int32)
        return table, lens, cu.to(table.device)

    def append_packed(self, layer: int, k_new: torch.Tensor, v_new: torch.Tensor, block_table: torch.Tensor,
                      seq_lens: torch.Tensor, cu_seqlens_q: torch.Tensor) -> None:
        """Store packed k_new / v_new [tokens, heads, head_dim] as the LAST
        tokens of their sequences: row cu[b] + i goes to position
        seq_lens[b] - (cu[b+1] - cu[b]) + i."""
        k_pool, v_pool = self._pools(layer)
        if self.kv_dtype is not None:
            pli_hip.kv_append_varlen_paged_fp8(k_new, v_new, k_pool, v_pool, block_table, seq_lens, cu_seqlens_q,
                                               self.k_scale[layer], self.v_scale[layer])
            return
        pli_hip.kv_append_varlen_paged(k_new, v_new, k_pool, v_pool, block_table, seq_lens, cu_seqlens_q)

    def packed_workspace_bytes(self, batch: int, max_tokens: int, q_heads: int, max_blocks: int | None = None) -> int:
        """Bytes ``attend_packed(..., workspace=)`` needs for a step of
        ``batch`` requests and ``max_tokens`` packed rows of ``q_heads`` heads
        over tables ``max_blocks`` wide (default: the whole pool): the size
        pli_attn_varlen_paged_workspace_size reports, 0 when the keys are too
        few to split."""
        width = self.num_blocks if max_blocks is None else int(max_blocks)
        return pli_hip.attn_varlen_paged_workspace_bytes(batch, max_tokens, q_heads, self.num_heads,
                                                         width * self.block_size, self.head_dim)

    def packed_workspace(self, batch: int, max_tokens: int, q_heads: int, max_blocks: int | None = None):
        """A float32 device tensor of ``packed_workspace_bytes(...)`` bytes (at
        least one element) for ``attend_packed``; it need not be initialised
        and can be reused by every layer and step of the same sizes."""
        if self.k_cache is None:
            raise pli_hip.PliError("PagedKVCache has no device pools (created off-device)")
        need = self.packed_workspace_bytes(batch, max_tokens, q_heads, max_blocks)
        return torch.empty(max(need // 4, 1), dtype=torch.float32, device=self.k_cache.device)

    def _attend_packed_ws(self, layer: int, q: torch.Tensor, block_table: torch.Tensor, seq_lens: torch.Tensor,
                          cu_seqlens_q: torch.Tensor, causal: bool = True, *, workspace: torch.Tensor) -> torch.Tensor:
        """attend_packed through the split-K calls (pli_attn_varlen_paged_ws /
        _fp8_ws) with the plan's own span"""
        k_pool, v_pool = self._pools(layer)
        if self.kv_dtype is not None:
            return pli_hip.attn_varlen_paged_fp8(q, k_pool, v_pool, block_table, seq_lens, cu_seqlens_q,
                                                 self.k_scale[layer], self.v_scale[layer], causal=causal,
                                                 workspace=workspace)
        return pli_hip.attn_varlen_paged(q, k_pool, v_pool, block_table, seq_lens, cu_seqlens_q, causal=causal,
                                         workspace=workspace)

    @_workspace_keyword
    def attend_packed(self, layer: int, q: torch.Tensor, block_table: torch.Tensor, seq_lens: torch.Tensor,
                      cu_seqlens_q: torch.Tensor, causal: bool = True) -> torch.Tensor:
        """Attention of packed q [tokens, Hq, head_dim] over each sequence's
        own pages and length in one launch, prompt chunks and decode rows
        mixed; causal masks bottom-right per sequence.  Returns [tokens, Hq,
        head_dim].  The keyword ``workspace=`` (a ``packed_workspace(...)``
        tensor; default None, this call as it is) makes the split-K call, which
        gives a long sequence's tile several workgroups."""
        k_pool, v_pool = self._pools(layer)
        if self.kv_dtype is not None:
            return pli_hip.attn_varlen_paged_fp8(q, k_pool, v_pool, block_table, seq_lens, cu_seqlens_q,
                                                 self.k_scale[layer], self.v_scale[layer], causal=causal)
        return pli_hip.attn_varlen_paged(q, k_pool, v_pool, block_table, seq_lens, cu_seqlens_q, causal=causal)


def explain_paged_memory() -> str:
    return """
Paged KV cache on MI355X

Why pages: a contiguous cache reserves max_seq_len rows per request, so short
requests strand memory that no other request can use.

How it works here:
  - The pool is cut into blocks of block_size tokens (16 is typical).
  - A free set hands blocks out; a request's block table lists its blocks in
    logical order; freeing a request returns them to the set.
  - A prompt of N tokens takes ceil(N / block_size) blocks; decoding takes one
    more block each time a boundary is crossed.  Nothing is copied or
    pre-reserved, and equal-sized blocks do not fragment.

Attention over pages:
  - pli_attn_decode_paged reads K and V rows straight from the scattered
    blocks: row j of sequence b lives in page table[b][j // block_size] at
    slot j % block_size.
  - The table entries a step needs are fetched two steps ahead, so the extra
    indirection stays off the critical path; every sequence attends over its
    own length, read on the device, so the step replays in a captured graph.

Mixed steps (prompt chunks and decode rows in one launch):
  - pli_attn_varlen_paged takes the step's new tokens packed, sequence b
    owning rows cu_seqlens_q[b] .. cu_seqlens_q[b+1] - 1, however many each
    has (none for a request that sits the step out).
  - 64 rows of one kv head (token-major, the kv head's query heads minor) form
    a tile; the four waves of a workgroup share each 32-key K/V image, loaded
    once through the block table, and a tile stops at its last row's causal
    limit.  tables_packed / append_packed / attend_packed drive it.
  - With a workspace (packed_workspace, attend_packed(..., workspace=ws)) a
    tile's keys are cut into chunks that run as workgroups of their own and
    are merged by a second kernel (pli_attn_varlen_paged_ws): a decode row at
    long context no longer walks all its keys in one workgroup.

A 1-byte cache (kv_dtype=torch.float8_e4m3fn):
  - The pools hold OCP fp8 e4m3 codes, value = code * scale[layer, kv head];
    the same HBM holds twice the tokens and decode reads half the bytes.
  - The appends quantise (x / scale, clamped to +-448, round to nearest even);
    the attention kernels widen each code exactly to q's type between the
    global load and the LDS write, so the MFMA loop and the softmax are those of
    the 16-bit kernels, with k_scale folded into the softmax constant and
    v_scale into the final 1/l.
"""


if __name__ == "__main__":
    print(explain_paged_memory())
    cache = PagedKVCache(num_blocks=100, block_size=16, num_layers=32, num_heads=32, head_dim=128, device="cpu")
    print("empty:", cache.get_memory_usage())
    first = cache.allocate_blocks(request_id=1, num_tokens=50)
    print(f"request 1, 50 tokens: blocks {first.block_indices}, {cache.get_num_free_blocks()} free")
    second = cache.allocate_blocks(request_id=2, num_tokens=100)
    print(f"request 2, 100 tokens: blocks {second.block_indices}, {cache.get_num_free_blocks()} free")
    cache.extend_blocks(request_id=1, new_tokens=30)
    print(f"request 1 grown to {cache.block_tables[1].num_tokens} tokens: blocks {cache.block_tables[1].block_indices}")
    print(f"request 2 freed: {cache.free_blocks_for_request(request_id=2)} blocks back, "
          f"{cache.get_num_free_blocks()} free")
    for key, value in cache.get_memory_usage().items():
        print(f"  {key}: {value:.2f}" if isinstance(value, float) else f"  {key}: {value}")
