"""The flash dispatch and the v13 / pp64 argument block, on the CPU.

csrc/flash_plan.h is pure host C++: plan_flash picks the kernel family of a
call and pack_v13 fills the 64-dword block the generated programs read.
tests/host/flash_plan_check.cpp (built here with the host compiler, under
AddressSanitizer + UBSan where the compiler has them) prints both for a list
of calls, and this file checks
 (a) the route table of tests/flash_route_cases.py FLASH (what
     tests/test_gpu_routes.py demands of the device) at 256 CUs,
 (b) every variant number and the edges of the chain (FORCED, and the rules
     below that launch nothing), and
 (c) the block word for word against tools/v13/run.py args_for (with
     tools/v14/pp64_run.py's for pp64) -- the block the emulator tests prove
     drives the programs correctly -- fed the planner's grid.
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
from flash_route_cases import BF, FLASH, FORCED, FP, forced_id

sys.path.insert(0, os.path.join(ROOT, "tools"))

from v13 import run as R  # noqa: E402
from v13.kernel import AI  # noqa: E402
from v14 import pp64_run as P  # noqa: E402

CUS = 256
PTRS = (0x7F0000001000, 0x7F0100002000, 0x7F0200003000, 0x7F0300004000)
DT = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}


def _cxx():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("c++"), shutil.which("g++")):
        if cand and os.path.exists(cand):
            return cand
    pytest.fail("no host C++ compiler")


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("flash_plan") / "flash_plan_check")
    cmd = [_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "host", "flash_plan_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(cmd + san, capture_output=True, text=True)
    if r.returncode != 0:  # a compiler without the sanitizer runtimes: the plain build
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def bhsd(B, H, Hkv, Nq, Nk, D):
    """element strides of contiguous [B, H, N, D] tensors: qb qh qn kb kh kn vb vh vn ob oh on"""
    q, kv = (H * Nq * D, Nq * D, D), (Hkv * Nk * D, Nk * D, D)
    return [*q, *kv, *kv, *q]


def bshd(B, H, Hkv, Nq, Nk, D):
    """[B, S, H, D] storage: strided heads"""
    q, kv = (Nq * H * D, D, H * D), (Nk * Hkv * D, D, Hkv * D)
    return [*q, *kv, *kv, *q]


def call(B, H, Hkv, Nq, Nk, D, dtype, causal, variant=-1, scale=None, cus=CUS, strides=None, ptrs=PTRS):
    scale = D ** -0.5 if scale is None else scale
    return dict(B=B, H=H, Hkv=Hkv, Nq=Nq, Nk=Nk, D=D, dtype=DT.get(dtype, dtype), causal=bool(causal), variant=variant,
                scale=float(np.float32(scale)), cus=cus, strides=strides or bhsd(B, H, Hkv, Nq, Nk, D), ptrs=ptrs)


def plan(checker, calls):
    """the driver's answer for each call"""
    text = "".join("{B} {H} {Hkv} {Nq} {Nk} {D} {dtype} {c} {s} {scale!r} {variant} {cus} {p}\n".format(
        c=int(k["causal"]), s=" ".join(map(str, k["strides"])), p=" ".join(map(str, k["ptrs"])), **k) for k in calls)
    r = subprocess.run([checker], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert len(out) == len(calls)
    return out


# ---- (a) the route table ---------------------------------------------------
def test_route_table(checker):
    got = plan(checker, [call(*c[:8]) for c in FLASH])
    assert [g["route"] for g in got] == [c[8] for c in FLASH]


# ---- (b) forced variants and edges -----------------------------------------
def test_forced_variants(checker):
    got = plan(checker, [call(*c[1:9], variant=c[0], scale=c[9]) for c in FORCED])
    bad = [(forced_id(c), g["route"]) for c, g in zip(FORCED, got) if g["route"] != c[10]]
    assert not bad, bad
    covered = {c[0] for c in FORCED}
    assert covered >= {21, 50, 51, 54, 55, 60, *range(70, 75), *range(80, 89)}


def test_plan_parameters(checker):
    """what each variant number asks of its family (include/pli.h)"""
    a128, a64 = (2, 4, 2, 256, 256, 128), (2, 4, 2, 256, 256, 64)
    want = [  # (call, family, {parameter: value})
        *[(call(*a128, BF, False, v), "v7", {"sub": v - 50}) for v in (50, 51, 54, 55, 60)],
        (call(*a128, BF, False, 70), "v12", {"persistent": False, "thr": 64}),
        (call(*a128, BF, False, 71), "v12", {"persistent": True, "thr": 64}),
        (call(*a128, BF, False, 72), "v12", {"persistent": True, "thr": 0}),
        (call(*a128, BF, True, 73), "v12", {"persistent": False, "thr": 64}),
        (call(*a128, BF, True, 74), "v12", {"persistent": True, "thr": 64}),
        (call(*a128, BF, False, 80), "v13", {"persistent": True, "muoff": 62}),
        (call(*a128, BF, False, 81), "v13", {"persistent": False, "muoff": 62}),
        (call(*a128, BF, True, 83), "v13", {"persistent": True, "muoff": 62}),
        (call(*a128, BF, True, 84), "v13", {"persistent": False, "muoff": 62}),
        (call(*a64, BF, False, 86), "pp64", {"persistent": True, "muoff": 62}),
        (call(*a128, BF, False, -1), "v13", {"variant": 80, "persistent": True}),  # the defaults: 88 -> 80 / 86, 83
        (call(*a128, BF, True, -1), "v13", {"variant": 83, "persistent": True}),
        (call(8, 32, 32, 4096, 4096, 64, BF, False, -1), "pp64", {"variant": 86}),
        (call(*a128, BF, False, 16), "unknown", {"variant": 16, "route": ""}),   # not a variant: an error at launch
        (call(*a128, BF, False, 89), "unknown", {"variant": 89}),
        # the rare-path sweeps: mu = max c (bf16), max c - 1 (fp16)
        *[(call(*a128, dt, v == 85, v), "v13", {"muoff": m}) for v in (82, 85) for dt, m in ((BF, 0), (FP, -1))],
        *[(call(*a64, dt, False, 87), "pp64", {"muoff": m}) for dt, m in ((BF, 0), (FP, -1))],
        # the fp16 mu offset falls by one per doubling of Nk past 4096 (floor 1); bf16 keeps 62
        *[(call(1, 4, 4, 256, nk, 128, FP, c, -1), "v13", {"muoff": m})
          for nk, m in ((256, 4), (4096, 4), (8192, 3), (32768, 1), (65536, 1)) for c in (False, True)],
        *[(call(1, 256, 256, 512, nk, 64, FP, False, -1), "pp64", {"muoff": m}) for nk, m in ((4096, 4), (8192, 3))],
        *[(call(1, 4, 4, 256, nk, 128, BF, False, -1), "v13", {"muoff": 62}) for nk in (4096, 65536)],
    ]
    got = plan(checker, [w[0] for w in want])
    for (k, family, params), g in zip(want, got):
        assert g["family"] == family, (k, g)
        assert {p: g[p] for p in params} == params, (k, g)


def test_fill_rule(checker):
    """88, D 64 non-causal: pp64 where B H ceil(Nq / 512) >= the CU count"""
    cases = [  # (B, H, Nq, CUs, route)
        (1, 256, 64, 256, "attn_fwd_pp64"), (1, 255, 64, 256, "attn_fwd_v13_d64"),
        (1, 256, 512, 256, "attn_fwd_pp64"), (1, 128, 513, 256, "attn_fwd_pp64"), (1, 128, 512, 256, "attn_fwd_v13_d64"),
        (4, 76, 64, 304, "attn_fwd_pp64"), (4, 76, 64, 305, "attn_fwd_v13_d64"), (3, 101, 64, 304, "attn_fwd_v13_d64"),
    ]
    got = plan(checker, [call(B, H, H, Nq, 128, 64, BF, False, cus=cus) for B, H, Nq, cus, _ in cases])
    assert [g["route"] for g in got] == [c[4] for c in cases]
    # causal D 64 stays on v13c however full the chip; D 128 never takes pp64
    got = plan(checker, [call(8, 256, 256, 512, 512, 64, BF, True), call(8, 256, 256, 512, 512, 64, FP, True),
                         call(8, 256, 256, 512, 512, 128, BF, False)])
    assert [g["route"] for g in got] == ["attn_fwd_v13c_d64", "attn_fwd_v13hc_d64", "attn_fwd_v13"]


def test_v13_range_edges(checker):
    """what v13's packed fields cannot hold leaves v13 (to v12 here: bf16, D 128, Nk % 64 == 0)"""
    D = 128
    neg = bhsd(1, 4, 4, 256, 256, D)
    neg[0] = -neg[0]  # a negative batch stride
    wide = bhsd(1, 1, 1, (1 << 20) + 1, 256, D)
    wide[2] = wide[11] = 2048  # q_ext = 2^20 rows * 4096 B + 256 >= 2^32
    below = list(wide)
    below[2] = below[11] = 2040
    cases = [
        (call(1, 4, 4, 256, 256, D, BF, False, strides=neg), "attn_fwd_v12"),
        (call(1, 1, 1, (1 << 20) + 1, 256, D, BF, False, strides=wide), "attn_fwd_v12"),
        (call(1, 1, 1, (1 << 20) + 1, 256, D, BF, False, strides=below), "attn_fwd_v13"),
        (call(1, 1, 1, 64, 64 * 0x10000, D, BF, True), "attn_fwd_v12"),    # causal: cdiv(Nk, 64) > 0xFFFF
        (call(1, 1, 1, 64, 64 * 0xFFFF, D, BF, True), "attn_fwd_v13c"),
        (call(1, 1, 1, 64, 64 * 0x10000, D, BF, False), "attn_fwd_v13"),   # the limit is the causal stream's
        (call(1, 65536, 65536, 64, 256, D, BF, False), "attn_fwd_v12"),    # H past the packed 16 bits
        (call(1, 65535, 65535, 64, 256, D, BF, False), "attn_fwd_v13"),
        (call(1, 65536, 65536, 64, 256, 64, BF, False, cus=8), "attn_fwd_v7"),  # pp64 packs H the same way
        # operands no MFMA kernel reads: an address off 16 bytes, a stride off 8 elements, rows closer than D
        (call(2, 4, 2, 256, 256, D, BF, False, ptrs=(PTRS[0] + 8, *PTRS[1:])), "attn_fwd_generic"),
        (call(2, 4, 2, 256, 256, D, BF, False, strides=[s + 4 * (i == 1) for i, s in enumerate(bhsd(2, 4, 2, 256, 256, D))]),
         "attn_fwd_generic"),
        (call(2, 4, 2, 256, 256, D, BF, False, strides=[64 if i == 5 else s for i, s in enumerate(bhsd(2, 4, 2, 256, 256, D))]),
         "attn_fwd_generic"),
    ]
    got = plan(checker, [c[0] for c in cases])
    assert [g["route"] for g in got] == [c[1] for c in cases]


# ---- (c) the argument block ------------------------------------------------
def _c_word(scale):
    """the block's c = scale log2(e), formed in fp32 as pack_v13 does (the mirror forms it in double)"""
    return int((np.float32(scale) * np.float32(1.4426950408889634)).view(np.uint32))


BLOCKS = {  # name: (call, family, walk -- the causal walk word's low byte, or None)
    "plain": (call(2, 4, 4, 512, 512, 128, BF, False), "v13", None),
    "plain-persistent": (call(8, 32, 32, 4096, 4096, 128, BF, False), "v13", None),
    "causal-pair-walk": (call(8, 32, 32, 4096, 4096, 128, BF, True), "v13", 1),
    "causal-remap-walk": (call(2, 4, 4, 768, 768, 128, BF, True), "v13", 2),
    "causal-remap-walk-full-chip": (call(3, 40, 40, 4096, 4096, 128, BF, True), "v13", 2),
    "chunked-prefill": (call(1, 8, 8, 128, 1024, 128, BF, True), "v13", 2),
    "ragged": (call(2, 4, 4, 300, 1000, 128, BF, False), "v13", None),
    "ragged-causal": (call(1, 8, 8, 100, 1000, 128, BF, True), "v13", 2),
    "ragged-causal-pair-walk": (call(8, 32, 32, 4000, 4072, 128, FP, True), "v13", 1),
    "one-row": (call(1, 8, 2, 1, 777, 64, FP, True), "v13", 2),
    "gqa4": (call(2, 8, 2, 256, 512, 128, BF, False), "v13", None),
    "bshd": (call(2, 4, 2, 384, 640, 128, BF, True, strides=bshd(2, 4, 2, 384, 640, 128)), "v13", 2),
    "d64": (call(2, 4, 2, 256, 256, 64, FP, False, scale=0.25), "v13", None),
    "d64-scale1": (call(2, 6, 3, 200, 328, 64, BF, False, scale=1.0), "v13", None),
    "sweep": (call(2, 4, 4, 512, 512, 128, FP, False, variant=82), "v13", None),
    "one-block-per-workgroup": (call(8, 32, 32, 4096, 4096, 128, BF, False, variant=81), "v13", None),
    "pp64": (call(2, 4, 2, 1024, 128, 64, BF, False, variant=86), "pp64", None),
    "pp64-persistent": (call(8, 64, 16, 512, 256, 64, BF, False), "pp64", None),
    "pp64-short-keys": (call(8, 64, 64, 512, 192, 64, FP, False), "pp64", None),   # Nk < 256: one block per workgroup
    "pp64-causal": (call(2, 4, 2, 512, 768, 64, FP, True, variant=86), "pp64", None),
    "pp64-bshd": (call(2, 4, 2, 600, 256, 64, BF, False, variant=86, strides=bshd(2, 4, 2, 600, 256, 64)), "pp64", None),
}


@pytest.mark.parametrize("name", BLOCKS)
def test_argument_block(checker, name):
    k, family, walk = BLOCKS[name]
    g = plan(checker, [k])[0]
    assert g["family"] == family and g["error"] == "", g
    mirror = (P if family == "pp64" else R).args_for(*k["ptrs"], k["B"], k["H"], k["Hkv"], k["Nq"], k["Nk"], k["strides"],
                                                     k["scale"], g["grid"], g["muoff"], k["causal"])
    mirror[AI["c"]] = _c_word(k["scale"])
    names = {i: n for n, i in AI.items()}
    diff = [(names.get(i, i), g["args"][i], int(mirror[i])) for i in range(64) if g["args"][i] != int(mirror[i])]
    assert not diff, diff
    rows = 512 if family == "pp64" else 256
    nqv = k["Nq"] + ((k["Nk"] - k["Nq"]) & 63 if k["causal"] else 0)
    nb = k["B"] * k["H"] * -(-nqv // rows)
    assert g["grid"] == (CUS if name in ("plain-persistent", "causal-pair-walk", "ragged-causal-pair-walk",
                                         "pp64-persistent") else nb)
    assert (g["D"], bool(g["fp16"]), bool(g["causal"]), bool(g["ragged"]), bool(g["pp64"])) == (
        k["D"], k["dtype"] == "f16", k["causal"], k["Nk"] % 64 != 0, family == "pp64")
    if walk is not None and family == "v13":
        assert g["args"][AI["cw"]] & 0xFF == walk
    p0 = (64 - k["Nk"] % 64) % 64  # ragged: in cw (non-causal) or the top byte of hx (causal)
    assert (g["args"][AI["hx"]] >> 24 if k["causal"] else g["args"][AI["cw"]] if p0 else 0) == p0

