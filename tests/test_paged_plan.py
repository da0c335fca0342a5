"""The paged decode plan and address arithmetic, on the CPU.

csrc/paged_plan.h is pure C++ whose functions the kernels of
csrc/paged_attn.hip call on the device: the split-K plan of a paged call (the
rule of csrc/decode_plan.h, shared with the contiguous kernel), the rule that
picks the MFMA kernel or the generic one, and the function that turns logical
key j of sequence b into the offset of its row through the block table.
tests/host/paged_plan_check.cpp (built here with the host compiler, under
AddressSanitizer + UBSan where the compiler has them; no Python code runs
under a sanitizer) prints them for a list of commands, and this file checks
 (a) the plan against pli_attn_decode_workspace_size (through the library, no
     GPU) for the shapes tests/test_capi.py pins and for the GPU cases of
     tests/paged_cases.py -- which proves which GPU cases really split,
 (b) every key of a few small pools against the offset numpy computes,
 (c) 64-bit offsets in a pool of more than 2^31 elements (nothing allocated),
 (d) the clamp of out-of-range table entries, and
 (e) the fast / generic rule.
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from paged_cases import CASES, GENERIC, max_kv_of

DT = {"fp32": 0, "fp16": 1, "bf16": 2}


def _cxx():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("c++"), shutil.which("g++")):
        if cand and os.path.exists(cand):
            return cand
    pytest.fail("no host C++ compiler")


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("paged_plan") / "paged_plan_check")
    cmd = [_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "host", "paged_plan_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(cmd + san, capture_output=True, text=True)
    if r.returncode != 0:  # a compiler without the sanitizer runtimes: the plain build
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def ask(checker, lines):
    r = subprocess.run([checker], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def strides_of(c, layers=2):
    """q_b q_h q_n, k / v {page, token, head}, o_b o_h o_n of contiguous [B, Sq, H, D] q / o and a layer view of
    the [num_blocks, layers, bs, Hkv, D] pools"""
    q = (c.Sq * c.H * c.D, c.D, c.H * c.D)
    kv = (layers * c.bs * c.Hkv * c.D, c.Hkv * c.D, c.D)
    return [*q, *kv, *kv, *q]


def fast_line(c, scale=None, aligned=1, strides=None):
    scale = c.D ** -0.5 if scale is None else scale
    return "fast {} {} {} {} {!r} {} {}".format(DT[c.dt], c.D, c.Sq * (c.H // c.Hkv), c.bs, float(scale), aligned,
                                                " ".join(map(str, strides or strides_of(c))))


# ---- (a) the plan -----------------------------------------------------------
PINNED = [  # tests/test_capi.py::test_decode_workspace_plan: B, H, Hkv, n_q, n_kv, D
    (64, 32, 8, 1, 4096, 128), (128, 32, 8, 1, 4096, 128), (1, 32, 8, 1, 32768, 128), (1, 32, 8, 1, 100, 128),
    (1, 64, 2, 1, 4096, 128), (1, 8, 8, 1, 4096, 80),
]


def test_plan_matches_the_library(checker, built_lib):
    import pli_hip
    shapes = PINNED + [(c.B, c.H, c.Hkv, c.Sq, max_kv_of(c), c.D) for c in CASES.values()]
    shapes += [(8, 32, 8, 1, 32768, 128), (3, 8, 2, 1, 1, 64), (200, 16, 8, 1, 1025, 64), (2, 8, 8, 2, 129, 128)]
    got = ask(checker, ["plan {} {} {} {} {}".format(B, Hkv, n, Sq * (H // Hkv), D) for B, H, Hkv, Sq, n, D in shapes])
    for (B, H, Hkv, Sq, n, D), g in zip(shapes, got):
        rows = Sq * (H // Hkv)
        assert g["chunk"] % 128 == 0 and g["chunk"] * g["splits"] >= n > g["chunk"] * (g["splits"] - 1)
        assert g["ws"] == (B * Hkv * g["splits"] * rows * (D + 2) * 4 if g["splits"] > 1 else 0)
        if rows <= 16 and D in (64, 128):  # the shapes the MFMA kernels take: the library sizes both the same way
            assert g["ws"] == pli_hip.attn_decode_workspace_bytes(B, H, Hkv, Sq, n, D), (B, H, Hkv, Sq, n, D)
            assert g["ws"] == pli_hip.attn_decode_paged_workspace_bytes(B, H, Hkv, Sq, n, D)
        else:
            assert pli_hip.attn_decode_paged_workspace_bytes(B, H, Hkv, Sq, n, D) == 0
    by = dict(zip(shapes, got))
    assert by[PINNED[0]]["splits"] == 2 and by[PINNED[1]]["splits"] == 1 and by[PINNED[2]]["splits"] == 128
    assert by[PINNED[3]] == {"chunk": 128, "splits": 1, "ws": 0}
    assert by[(8, 32, 8, 1, 32768, 128)]["splits"] == 16  # the timing tool's shape: 64 pairs -> 1024 workgroups


def test_gpu_cases_split_as_the_tests_claim(checker):
    """which GPU cases run the combine kernel (tests/test_gpu_paged.py asserts the route they name)"""
    fast = [c for c in CASES.values() if c.route != GENERIC]
    got = ask(checker, ["plan {} {} {} {} {}".format(c.B, c.Hkv, max_kv_of(c), c.Sq * (c.H // c.Hkv), c.D) for c in fast])
    assert [g["splits"] for g in got] == [c.splits for c in fast]
    assert all((g["splits"] > 1) == c.route.endswith("_combine") for c, g in zip(fast, got))
    assert CASES["4"].splits > 1  # the split-K case with empty chunks
    assert all(max_kv_of(c) <= c.max_blocks * c.bs and max(c.lens) <= max_kv_of(c) for c in CASES.values())
    assert got[fast.index(CASES["8"])]["chunk"] == 512  # 4 steps per wave


def test_empty_plan(checker):
    assert ask(checker, ["plan 4 2 0 4 128"]) == [{"chunk": 128, "splits": 1, "ws": 0}]


# ---- (b) the address function, key by key -----------------------------------
POOLS = [  # bs, num_blocks, max_blocks, B, layers, Hkv, D
    (16, 11, 3, 2, 2, 2, 128), (64, 7, 2, 3, 1, 4, 64), (24, 9, 4, 2, 3, 2, 80), (256, 5, 2, 2, 2, 1, 128), (1, 6, 5, 1, 1, 1, 8),
]


def numpy_offsets(table, bs, nb, b, hk, n, pool):
    j = np.arange(n, dtype=np.int64)
    page = np.clip(table[b, np.minimum(j // bs, table.shape[1] - 1)].astype(np.int64), 0, nb - 1)
    return page * pool[0] + (j % bs) * pool[1] + hk * pool[2]


@pytest.mark.parametrize("shape", POOLS, ids=lambda s: "bs{}_nb{}_mb{}_b{}_l{}_h{}_d{}".format(*s))
def test_every_key_of_a_small_pool(checker, shape):
    bs, nb, mb, B, layers, Hkv, D = shape
    rng = np.random.default_rng(bs * 1000 + nb)
    table = np.stack([rng.permutation(nb)[:mb] for _ in range(B)]).astype(np.int32)
    pool = (layers * bs * Hkv * D, Hkv * D, D)
    lines = ["table {} {} {} {} {}".format(bs, nb, mb, B, " ".join(map(str, table.ravel()))), "pool {} {} {}".format(*pool)]
    lines += ["range {} {} {}".format(b, hk, mb * bs) for b in range(B) for hk in range(Hkv)]
    got = ask(checker, lines)
    assert got[0]["log2_bs"] == (int(np.log2(bs)) if bs & (bs - 1) == 0 else -1)
    seen = set()
    for (b, hk), g in zip(((b, hk) for b in range(B) for hk in range(Hkv)), got[2:]):
        want = numpy_offsets(table, bs, nb, b, hk, mb * bs, pool)
        assert g["off"] == want.tolist() and g["pow2_agrees"]
        seen.update(g["off"])
    # distinct pages per sequence: every (page, slot, head) row at most once per sequence, all inside the layer view
    assert max(seen) <= (nb - 1) * pool[0] + (bs - 1) * pool[1] + (Hkv - 1) * pool[2]


# ---- (c) past 2^31 ------------------------------------------------------------
def test_offsets_past_2_31(checker):
    bs, nb, Hkv, D, layers = 16, 50_000, 8, 128, 3
    pool = (layers * bs * Hkv * D, Hkv * D, D)
    assert nb * pool[0] > 2 ** 31  # elements; never allocated
    entries = [49_999, 43_691, 43_690, 0]  # 43_691 * 49_152 is the first page offset >= 2^31
    lines = ["table {} {} {} 1 {}".format(bs, nb, len(entries), " ".join(map(str, entries))), "pool {} {} {}".format(*pool)]
    keys = [(j, hk) for j in (0, 15, 16, 17, 31, 32, 47, 63) for hk in (0, 7)]
    got = ask(checker, lines + ["addr 0 {} {}".format(j, hk) for j, hk in keys])[2:]
    for (j, hk), g in zip(keys, got):
        want = entries[j // bs] * pool[0] + (j % bs) * pool[1] + hk * pool[2]  # Python integers
        assert g["off"] == [want] and g["page"] == entries[j // bs] and g["pow2_agrees"]
    assert max(g["off"][0] for g in got) > 2 ** 31
    # the same pool in bytes (pli_kv_append_paged's unit): past 2^32
    got = ask(checker, [lines[0], "pool {} {} {}".format(*(2 * s for s in pool)), "addr 0 15 7"])[2]
    assert got["off"] == [2 * (49_999 * pool[0] + 15 * pool[1] + 7 * pool[2])] and got["off"][0] > 2 ** 32


# ---- (d) the clamp ------------------------------------------------------------
def test_out_of_range_entries_are_clamped(checker):
    bs, nb = 16, 10
    pool = (2 * bs * 2 * 64, 2 * 64, 64)
    entries = [-5, 10, 1_000_000, -(2 ** 31), 2 ** 31 - 1, 9]
    lines = ["table {} {} {} 1 {}".format(bs, nb, len(entries), " ".join(map(str, entries))), "pool {} {} {}".format(*pool)]
    got = ask(checker, lines + ["addr 0 {} 1".format(i * bs + 3) for i in range(len(entries))] + ["range 0 1 {}".format(8 * bs)])[2:]
    want_pages = [0, 9, 9, 0, 9, 9]
    for g, p in zip(got, want_pages):
        assert g["page"] == p and g["off"] == [p * pool[0] + 3 * pool[1] + pool[2]]
    # keys past the table row (a prefetch one step past the last block) use the row's last entry
    offs = got[-1]["off"]
    assert len(offs) == 8 * bs and got[-1]["pow2_agrees"]
    assert all(0 <= o <= (nb - 1) * pool[0] + (bs - 1) * pool[1] + pool[2] for o in offs)
    assert offs[6 * bs:7 * bs] == offs[5 * bs:6 * bs]


# ---- (e) fast or generic --------------------------------------------------------
def test_fast_or_generic_rule(checker):
    from paged_cases import Case
    base = Case(2, 8, 2, 1, 16, 128, "bf16", [40], 3, None, None, 0)
    odd = strides_of(base)
    odd[4] += 4  # a token stride off 16 bytes
    table = [
        (base, {}, True), (base._replace(dt="fp16"), {}, True), (base._replace(D=64), {}, True),
        (base._replace(bs=256), {}, True), (base._replace(bs=32), {}, True),
        (base._replace(H=32), {}, True),            # 16 rows per kv head
        (base._replace(H=34), {}, False),           # 17
        (base._replace(Sq=4), {}, True), (base._replace(Sq=5), {}, False),  # 16 / 20 rows
        (base._replace(bs=24), {}, False), (base._replace(bs=8), {}, False),
        (base._replace(D=80), {}, False), (base._replace(D=256), {}, False),
        (base._replace(dt="fp32"), {}, False),
        (base, {"scale": 0.0}, False), (base, {"scale": -0.1}, False),  # the MFMA kernel's max is of the raw scores
        (base, {"aligned": 0}, False), (base, {"strides": odd}, False),
    ]
    got = ask(checker, [fast_line(c, **kw) for c, kw, _ in table])
    assert [g["fast"] for g in got] == [w for _, _, w in table]
    # the GPU cases take the kernel their route names
    got = ask(checker, [fast_line(c) for c in CASES.values()])
    assert [g["fast"] for g in got] == [c.route != GENERIC for c in CASES.values()]
