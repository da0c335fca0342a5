"""The parity cases of packed variable-length paged attention
(pli_attn_varlen_paged), shared by the GPU tests
(tests/test_gpu_varlen_paged.py) and the CPU plan test
(tests/test_varlen_plan.py, which proves on the CPU which kernel each takes).

Each case: Hq, Hkv, block size, D, dtype, the new tokens per sequence
(q_lens), the kv lengths after the step (kv_lens), the table width
max_blocks, whether the mask is causal, and the route pli_last_route must
name.
"""
from __future__ import annotations

from collections import namedtuple

from paged_cases import LENS8

VCase = namedtuple("VCase", "H Hkv bs D dt q_lens kv_lens max_blocks causal route")

FAST, GENERIC, APPEND = "attn_varlen_paged", "attn_varlen_paged_generic", "kv_append_varlen_paged"

MIXED = dict(q_lens=[1, 1, 37, 0, 70], kv_lens=[513, 16, 37, 40, 200])

CASES = {
    # decode rows, a pure prompt, a chunk with history that spans several tiles (70 tokens x G 4 = 5 tiles), and
    # a sequence that sits the step out
    "1": VCase(8, 2, 16, 128, "bf16", MIXED["q_lens"], MIXED["kv_lens"], 33, True, FAST),
    # G = 1: 64 tokens per tile
    "2": VCase(2, 2, 64, 64, "fp16", [130, 3], [130, 259], 5, True, FAST),
    # G = 16: one token per wave
    "3": VCase(32, 2, 16, 64, "bf16", [5, 1], [100, 33], 7, True, FAST),
    # n_kv < q_len: the first 8 tokens see nothing
    "4": VCase(8, 2, 16, 128, "bf16", [20], [12], 2, True, FAST),
    # steady state: 35 key steps, page boundaries inside the walk
    "5": VCase(8, 2, 256, 128, "bf16", [64], [1100], 5, True, FAST),
    # many sequences: the tile lookup over 128 of them, zero-length ones among them
    "6": VCase(4, 1, 16, 64, "fp16", [(7 * i) % 5 for i in range(128)], LENS8, 33, True, FAST),
    # the generic kernel: fp32, head_dim 80, block size 24, G = 3
    "7a": VCase(8, 2, 16, 128, "fp32", [3, 1, 9], [40, 17, 9], 3, True, GENERIC),
    "7b": VCase(4, 2, 16, 80, "bf16", [3, 1, 9], [40, 17, 9], 3, True, GENERIC),
    "7c": VCase(4, 2, 24, 64, "bf16", [3, 1, 9], [40, 17, 9], 2, True, GENERIC),
    "7d": VCase(6, 2, 16, 128, "bf16", [3, 1, 9], [40, 17, 9], 3, True, GENERIC),
    # case 1 without the causal mask
    "8": VCase(8, 2, 16, 128, "bf16", MIXED["q_lens"], MIXED["kv_lens"], 33, False, FAST),
}


def max_kv_of(c: VCase) -> int:
    return c.max_blocks * c.bs
