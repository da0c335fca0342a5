"""The split-K plan of packed variable-length paged attention, on the CPU.

csrc/varlen_plan.h cuts a tile's key range [0, key_end) into chunks of `span`
keys; attn_varlen_paged_split (one workgroup per tile, chunk and kv head) and
attn_varlen_paged_combine (one thread per packed row and 16-byte chunk) both
count a tile's chunks with varlen_tile_chunks.  tests/host/varlen_split_check.cpp
(built here with the host compiler, under AddressSanitizer + UBSan where the
compiler has them; no Python code runs under a sanitizer) replays both kernels'
index arithmetic, and this file checks
 (i)   each tile's chunks partition [0, key_end) exactly, start on even steps
       and number at most splits_max,
 (ii)  the partial rows the tile workgroups write are exactly those the combine
       reads (so it never reads uninitialised workspace), each written once, and
       every stored output row is written by exactly one of the two kernels,
 (iii) under malformed device tensors every partial row and every K / V and
       table address stays inside its operand,
 (iv)  the plan: the workspace formula, splits_max == 1 <=> no workspace, an
       explicit split_keys honoured, split_keys == 0 bounded by the cap.
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

BM, STEP = 64, 32


def _cxx():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("c++"), shutil.which("g++")):
        if cand and os.path.exists(cand):
            return cand
    pytest.fail("no host C++ compiler")


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("varlen_split") / "varlen_split_check")
    cmd = [_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "host", "varlen_split_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(cmd + san, capture_output=True, text=True)
    if r.returncode != 0:  # a compiler without the sanitizer runtimes: the plain build
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def ask(checker, lines):
    r = subprocess.run([checker], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def state_lines(cu, lens, table, bs, nb, mb, pool):
    return ["cu {} {}".format(len(cu) - 1, " ".join(map(str, cu))),
            "lens {} {}".format(len(lens), " ".join(map(str, lens))),
            "table {} {} {} {} {}".format(bs, nb, mb, len(lens), " ".join(map(str, np.asarray(table).ravel()))),
            "pool {} {} {}".format(*pool)]


def key_end_of(n_kv, q_len, tile, tpt, causal):
    i_last = min(q_len, (tile + 1) * tpt) - 1
    if i_last < 0:
        return 0
    return max(0, min(n_kv, n_kv - q_len + i_last + 1)) if causal else n_kv


def random_batch(rng, batch):
    """q_lens (decode rows, chunks and zeros mixed) and kv lengths (zeros, n_kv < q_len and long ones among them)"""
    q_lens = rng.choice([0, 0, 1, 1, 1, 2, 17, 64, 65, 130], batch)
    kv = rng.choice([0, 1, 63, 64, 65, 127, 128, 129, 500, 1024, 1025, 1500], batch)
    kv = np.where(rng.random(batch) < 0.8, np.maximum(kv, q_lens), kv)  # mostly n_kv >= q_len, some blind rows
    return q_lens.astype(np.int64), kv.astype(np.int64)


# ---- (i) + (ii) -------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 4, 16])
@pytest.mark.parametrize("causal", [1, 0])
def test_chunks_partition_and_partials_match(checker, G, causal):
    rng = np.random.default_rng(100 * G + causal)
    bs, Hkv, D = 16, 2, 64
    H, tpt = Hkv * G, BM // G
    for batch in (1, 9, 300):
        q_lens, kv = random_batch(rng, batch)
        if batch == 1:
            q_lens[0], kv[0] = 70, 1500
        cu = np.concatenate([[0], np.cumsum(q_lens)])
        mb = 1500 // bs + 1
        nb = 64
        table = rng.integers(0, nb, (batch, mb))
        pool = (2 * bs * Hkv * D, Hkv * D, D)
        max_tokens, max_kv = int(cu[-1]) + 3, mb * bs
        base = state_lines(cu, kv, table, bs, nb, mb, pool)
        spans = (64, 128, 1024)
        plans = ask(checker, ["plan {} {} {} {} {} {}".format(max_tokens, H, Hkv, max_kv, D, s) for s in spans])
        got = ask(checker, base + ["split {} {} {} {} {} {} {} {}".format(max_tokens, H, Hkv, D, max_kv, causal, s,
                                                                         p["splits_max"]) for s, p in zip(spans, plans)])[4:]
        for span, p, g in zip(spans, plans, got):
            assert p["span"] == span and p["splits_max"] == -(-max_kv // span)
            want_tiles = [(b, t) for b, n in enumerate(q_lens) for t in range(-(-int(n) // tpt))]
            assert [(t["b"], t["tile"]) for t in g["tiles"]] == want_tiles
            partial_rows, stored, merged_rows = 0, 0, 0
            for t in g["tiles"]:
                b = t["b"]
                end = key_end_of(int(kv[b]), int(q_lens[b]), t["tile"], tpt, causal)
                assert t["key_end"] == end
                assert t["chunks"] == max(1, -(-end // span)) <= p["splits_max"]
                r = t["ranges"]
                assert len(r) == t["chunks"] and r[0][0] == 0 and r[-1][1] == end
                assert all(a[1] == b2[0] for a, b2 in zip(r, r[1:])), "chunks are contiguous"
                assert all(0 < hi - lo <= span and lo % 64 == 0 for lo, hi in r) or end == 0
                rows = (min(int(q_lens[b]), (t["tile"] + 1) * tpt) - t["tile"] * tpt) * H
                stored += rows
                if t["chunks"] > 1:
                    partial_rows += rows * t["chunks"]
                    merged_rows += rows
            assert g["bad_step"] == 0
            assert g["same_set"] and g["dup"] == 0
            assert g["written"] == g["read"] == partial_rows
            assert g["merged"] == merged_rows and g["direct"] == stored - merged_rows and g["direct_and_merged"] == 0
            assert stored == int(cu[-1]) * H
            if g["written"]:
                assert 0 <= g["partial_written"][0] and g["partial_written"][1] < g["partial_rows"]
            if span == 64 and batch == 1:
                assert g["merged"] > 0  # the long sequence is split


# ---- (iii) ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
def test_split_addresses_under_malformed_device_tensors(checker, D):
    """a non-monotone cu_seqlens_q, INT_MIN / INT_MAX entries, lengths past max_kv and below 0, table entries out of
    range: every partial-row index of both kernels and every K / V and table address stays inside its operand"""
    bs, nb, mb, H, Hkv, max_tokens = 16, 6, 16, 8, 2, 40
    rng = np.random.default_rng(D)
    bad_table = rng.choice([-5, 6, 1_000_000, 2, -(2 ** 31), 2 ** 31 - 1, 0, 5, 3, 7, -1, 9], (4, mb))
    pool = (2 * bs * Hkv * D, Hkv * D, D)
    for cu in ([0, 30, 10, 25, 90], [5, 2, 2 ** 31 - 1, -7, 33], [-(2 ** 31), 2 ** 31 - 1, 0, 17, 12],
               [0, 0, 0, 0, 2 ** 31 - 1], [60, 70, 80, 90, 100], [0, 1, 2, 20, 40]):
        for lens in ([1000, -4, 2 ** 31 - 1, 17], [256, 63, 65, 0], [-(2 ** 31), 5, 200, 129]):
            lines = state_lines(cu, lens, bad_table, bs, nb, mb, pool)
            cmds = []
            for max_kv in (mb * bs, 200, 0):
                for span in (64, 128):
                    splits = max(1, -(-max_kv // span))
                    for causal in (1, 0):
                        cmds.append((max_kv, span, splits, "split {} {} {} {} {} {} {} {}".format(
                            max_tokens, H, Hkv, D, max_kv, causal, span, splits)))
            got = ask(checker, lines + [c[-1] for c in cmds])[4:]
            for (max_kv, span, splits, _), g in zip(cmds, got):
                assert g["partial_rows"] == splits * max_tokens * H
                for name in ("partial_written", "partial_read"):
                    lo, hi = g[name]
                    assert lo > hi or (0 <= lo and hi < g["partial_rows"]), (name, cu, lens, max_kv, span)
                lo, hi = g["table"]
                assert lo > hi or (0 <= lo and hi <= 4 * mb - 1)
                lo, hi = g["kv"]
                assert lo > hi or (0 <= lo and hi <= (nb - 1) * pool[0] + (bs - 1) * pool[1] + (Hkv - 1) * pool[2])
                assert all(t["chunks"] <= splits for t in g["tiles"])


# ---- (iv) the plan ---------------------------------------------------------------------
def test_the_plan(checker):
    shapes = [(1032, 32, 8, 32768, 128), (8, 32, 8, 32768, 128), (5, 8, 2, 64, 64), (1, 2, 2, 1, 64),
              (300, 16, 1, 100_000, 128), (40, 8, 2, 2 ** 31 - 64, 128), (7, 4, 4, 513, 64)]
    cmds = [(s, k) for s in shapes for k in (0, 64, 128, 1024, 4096)]
    got = ask(checker, ["plan {} {} {} {} {} {}".format(T, H, Hkv, max_kv, D, k) for (T, H, Hkv, max_kv, D), k in cmds])
    for ((T, H, Hkv, max_kv, D), k), p in zip(cmds, got):
        span_min, cap = p["span_min"], p["splits_cap"]
        assert span_min % 64 == 0 and span_min > 0 and cap >= 1
        if k:
            assert p["span"] == k, "an explicit split_keys is the span"
        else:
            assert p["span"] == max(span_min, -(-(-(-max_kv // cap)) // 64) * 64)
            assert p["splits_max"] <= cap
        assert p["span"] % 64 == 0
        assert p["splits_max"] == max(1, -(-max_kv // p["span"]))
        assert p["bytes"] == (p["splits_max"] * T * H * (D + 2) * 4 if p["splits_max"] > 1 else 0)
        assert (p["splits_max"] == 1) == (p["bytes"] == 0)
        assert p["bytes"] % 16 == 0
    # a shape only the generic kernel takes is never split
    got = ask(checker, ["plan 40 8 2 4096 80 64", "plan 40 6 2 4096 128 64", "plan 40 64 2 4096 128 64"])
    assert all(p["splits_max"] == 1 and p["bytes"] == 0 for p in got)
