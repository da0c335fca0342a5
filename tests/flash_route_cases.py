"""The flash dispatch table that DESIGN.md §0 / §3 and include/pli.h state,
as cases: tests/test_flash_plan.py asks the planner (csrc/flash_plan.h
plan_flash, on the CPU) for each route, tests/test_gpu_routes.py the device."""
from __future__ import annotations

import torch


def v13(dtype, D, causal, ragged):
    return ("attn_fwd_v13" + ("h" if dtype == torch.float16 else "") +
            ("rc" if ragged and causal else "r" if ragged else "c" if causal else "") + ("_d64" if D == 64 else ""))


BF, FP = torch.bfloat16, torch.float16
# (B, H, Hkv, Nq, Nk, D, dtype, causal, expected route)
FLASH = [
    *[(2, 4, 2, 256, 256, D, dt, c, v13(dt, D, c, False)) for D in (128, 64) for dt in (BF, FP) for c in (False, True)],
    *[(2, 4, 2, 200, 200, D, dt, c, v13(dt, D, c, True)) for D in (128, 64) for dt in (BF, FP) for c in (False, True)],
    (1, 8, 8, 128, 1024, 128, BF, True, "attn_fwd_v13c"),      # chunked prefill, offset 896
    (1, 8, 8, 100, 1000, 128, BF, True, "attn_fwd_v13rc"),     # offset 900, ragged
    (1, 8, 2, 1, 777, 64, FP, True, "attn_fwd_v13hrc_d64"),    # one query row
    (2, 4, 4, 64, 64, 128, BF, False, "attn_fwd_v12"),          # Nk = 64: v12
    (2, 4, 4, 64, 64, 128, BF, True, "attn_fwd_v12"),
    (2, 4, 4, 64, 64, 128, FP, False, "attn_fwd_v7"),           # v12 is bf16 only
    (2, 4, 4, 40, 40, 128, BF, False, "attn_fwd_v7"),           # Nk < 64
    (2, 4, 4, 300, 200, 128, BF, True, "attn_fwd_v7"),          # causal Nq > Nk
    (2, 4, 4, 128, 256, 96, BF, False, "attn_fwd_generic"),     # head dim 96
    (2, 4, 4, 128, 256, 128, torch.float32, False, "attn_fwd_generic"),
    (2, 4, 4, 128, 0, 128, BF, False, "attn_fwd_generic"),      # no keys: O = 0
]

# Forced variants (pli_flash_attn_fwd_variant) and the edges of the chain pp64
# -> v13 -> v12 -> v7 / v10 -> v2, written out from include/pli.h:
# (variant, B, H, Hkv, Nq, Nk, D, dtype, causal, scale or None for D^-1/2, route).
# Every variant number at a shape where it applies and at one where it falls
# through; small enough (a few heads of <= 256 rows) to run on the device too.
A128 = (2, 4, 2, 256, 256, 128)   # bf16 non-causal: every D = 128 family applies
A64 = (2, 4, 2, 256, 256, 64)     # every D = 64 family, pp64 too
FORCED = [
    (21, *A128, BF, False, None, "attn_fwd_v2"),
    *[(var, *A128, BF, False, None, "attn_fwd_v7") for var in (50, 51, 54, 55, 60)],
    *[(var, *A128, BF, True, None, "attn_fwd_v7") for var in (50, 51, 54, 55, 60)],
    *[(var, *A128, BF, False, None, "attn_fwd_v12") for var in (70, 71, 72)],
    *[(var, *A128, BF, True, None, "attn_fwd_v12") for var in (73, 74)],
    *[(var, *A128, BF, False, None, "attn_fwd_v13") for var in (80, 81, 82)],
    *[(var, *A128, BF, True, None, "attn_fwd_v13c") for var in (83, 84, 85)],
    *[(var, *A128, FP, False, None, "attn_fwd_v13h") for var in (80, 82)],
    *[(var, *A64, BF, False, None, "attn_fwd_pp64") for var in (86, 87)],
    *[(var, *A64, FP, False, None, "attn_fwd_pp64h") for var in (86, 87)],
    (86, *A64, BF, True, None, "attn_fwd_pp64c"),
    (86, *A64, FP, True, None, "attn_fwd_pp64hc"),
    (86, 2, 4, 2, 64, 1024, 64, BF, False, None, "attn_fwd_pp64"),         # Nk >= 256: pp64's persistent rule
    (88, *A128, BF, False, None, "attn_fwd_v13"),
    (88, *A64, BF, False, None, "attn_fwd_v13_d64"),      # 8 blocks of 512 rows do not fill a chip
    (88, *A64, BF, True, None, "attn_fwd_v13c_d64"),      # causal D 64 stays on v13c
    # falling through
    *[(var, *A128, BF, False, None, "attn_fwd_v13") for var in (86, 87)],  # pp64 is D 64 only
    (86, 2, 4, 2, 200, 200, 64, BF, False, None, "attn_fwd_v13r_d64"),     # ragged Nk
    (86, 2, 4, 2, 100, 256, 64, BF, True, None, "attn_fwd_v13c_d64"),      # causal pp64 needs Nq % 64 == 0
    (87, 2, 4, 2, 100, 256, 64, FP, True, None, "attn_fwd_v13hc_d64"),
    *[(var, *A128, BF, True, None, "attn_fwd_v12") for var in (80, 81, 82)],   # non-causal form, causal call -> 74
    *[(var, *A128, BF, False, None, "attn_fwd_v12") for var in (83, 84, 85)],  # causal form, plain call -> 71
    *[(var, 2, 4, 4, 64, 64, 128, BF, False, None, "attn_fwd_v12") for var in (80, 86, 88)],  # Nk = 64 -> v12
    (83, 2, 4, 4, 64, 64, 128, BF, True, None, "attn_fwd_v12"),
    *[(var, 2, 4, 4, 64, 64, 128, FP, False, None, "attn_fwd_v7") for var in (70, 71, 72, 80)],  # fp16 -> not v12
    *[(var, 2, 4, 4, 64, 64, 128, FP, True, None, "attn_fwd_v7") for var in (73, 74, 83)],
    *[(var, 2, 4, 4, 64, 64, 64, BF, False, None, "attn_fwd_v7") for var in (70, 71, 72, 80, 86, 88)],  # D 64 -> not v12
    *[(var, 2, 4, 4, 64, 64, 64, BF, True, None, "attn_fwd_v7") for var in (73, 74, 83)],
    *[(var, *A128, BF, True, None, "attn_fwd_v7") for var in (70, 71, 72)],     # v12's plain forms are non-causal
    *[(var, *A128, BF, False, None, "attn_fwd_v7") for var in (73, 74)],        # and its causal forms causal
    *[(var, 2, 4, 4, 300, 200, 128, BF, True, None, "attn_fwd_v7") for var in (73, 74, 83, 84, 85)],  # causal Nq > Nk
    *[(var, 2, 4, 4, 40, 40, 128, BF, False, None, "attn_fwd_v7") for var in (70, 80, 86)],  # Nk < 64
    # c = scale log2(e) > 1: the prescaled 50 / 54 -> v2, the exact ones stay
    *[(var, *A128, BF, False, 1.0, "attn_fwd_v2") for var in (50, 54)],
    *[(var, *A128, BF, False, 1.0, "attn_fwd_v7") for var in (51, 55, 60)],
    (71, *A128, BF, False, 1.0, "attn_fwd_v12"),
    (80, *A128, BF, False, 1.0, "attn_fwd_v13"),
    # scale <= 0 never reaches an MFMA kernel, whatever the variant
    *[(var, *A128, BF, False, sc, "attn_fwd_generic") for var in (-1, 21, 50, 71, 80, 88) for sc in (0.0, -0.125)],
]


def forced_id(c):
    return "v{}-b{}h{}kv{}q{}k{}d{}-{}-causal{}-scale{}".format(*c[:7], str(c[7]).split(".")[-1], int(c[8]), c[9])
