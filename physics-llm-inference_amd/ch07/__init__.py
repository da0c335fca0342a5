"""Chapter 07 on MI355X: the paged KV cache (the part with device work).

``PagedKVCache`` mirrors the reference's allocator and adds the device half it
describes but does not write: paged append and decode attention over the block
pool (csrc/paged_attn.hip).  The batchers, the scheduler and the radix cache
of the reference's ch07 are CPU bookkeeping (SURVEY.md §8 out of scope) and
are not mirrored.
"""

from .paged_memory import BlockTable, PagedKVCache, explain_paged_memory

__all__ = ["BlockTable", "PagedKVCache", "explain_paged_memory"]
