"""The parity cases of paged decode attention, shared by the GPU tests
(tests/test_gpu_paged.py) and the CPU plan test (tests/test_paged_plan.py,
which proves on the CPU which of them split and which take the generic
kernel).

Each case: B, Hq, Hkv, Sq, block size, D, dtype, per-sequence lengths, the
table width max_blocks, max_kv (None: max_blocks * block size), the route
pli_last_route must name, and whether the plan splits.
"""
from __future__ import annotations

from collections import namedtuple

Case = namedtuple("Case", "B H Hkv Sq bs D dt lens max_blocks max_kv route splits")

FAST, COMBINE, GENERIC = "attn_decode_paged", "attn_decode_paged+attn_decode_paged_combine", "attn_decode_paged_generic"

# lengths of case 8: 128 sequences between 0 and 512 keys, every residue mod 16 and mod 32
LENS8 = [(37 * i + 11) % 513 for i in range(126)] + [512, 0]

CASES = {
    # one token, exactly one page, a ragged last page, an empty sequence (its row must be 0)
    "1": Case(4, 8, 2, 1, 16, 128, "bf16", [1, 16, 47, 0], 3, None, FAST, 1),
    # G = 16: a full 16-row tile
    "2": Case(2, 32, 2, 1, 16, 64, "fp16", [200, 33], 13, None, COMBINE, 2),
    # G = 1
    "3": Case(2, 4, 4, 1, 64, 128, "bf16", [129, 64], 3, None, COMBINE, 2),
    # split-K with chunks that are empty for the short sequences
    "4": Case(3, 8, 2, 1, 16, 128, "bf16", [1000, 130, 5], 64, 1024, COMBINE, 8),
    # 128-key chunks inside one 256-token page, page boundaries between chunks
    "5": Case(2, 8, 2, 1, 256, 128, "bf16", [700, 300], 3, None, COMBINE, 6),
    # causal multi-token chunk, bottom-right mask per sequence; length == n_q
    "6": Case(2, 8, 2, 3, 16, 128, "bf16", [50, 3], 4, None, FAST, 1),
    # the generic kernel: fp32, head_dim 80, block size 24, 32 rows per kv head
    "7a": Case(1, 8, 2, 1, 16, 128, "fp32", [77], 5, None, GENERIC, 0),
    "7b": Case(1, 4, 2, 1, 16, 80, "bf16", [77], 5, None, GENERIC, 0),
    "7c": Case(1, 4, 2, 1, 24, 64, "bf16", [50], 3, None, GENERIC, 0),
    "7d": Case(1, 64, 2, 1, 16, 128, "bf16", [40], 3, None, GENERIC, 0),
    # many steps per wave (none of the cases above runs more than one 32-key
    # step per wave, so none reaches the kernel's steady state: table entries
    # fetched two steps ahead, K/V one step ahead).  128 (batch, kv head) pairs
    # and <= 1024 keys take one chunk: 512 keys = 4 steps per wave, page
    # boundaries inside every wave's range, every length residue
    "8": Case(128, 4, 1, 1, 16, 64, "fp16", LENS8, 32, None, FAST, 1),
}


def max_kv_of(c: Case) -> int:
    return c.max_blocks * c.bs if c.max_kv is None else c.max_kv
