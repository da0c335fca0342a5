"""The packed variable-length paged attention plan, on the CPU.

csrc/varlen_plan.h is pure C++ whose functions the kernels of
csrc/varlen_attn.hip call on the device: the tile map (workgroup -> sequence
and tile, from cu_seqlens_q), a tile's key range and each row's causal limit,
the append position rule, the address clamps and the fast / generic rule.
tests/host/varlen_plan_check.cpp (built here with the host compiler, under
AddressSanitizer + UBSan where the compiler has them; no Python code runs
under a sanitizer) prints them for a list of commands, and this file checks
 (a) the tile map against numpy for random cu_seqlens_q, zeros included,
     batch up to 300,
 (b) key_end and the row limits against a brute-force bottom-right mask,
 (c) the append positions, dropped ones included,
 (d) every address the MFMA kernel forms under a non-monotone cu_seqlens_q,
     lengths past max_kv and out-of-range table entries,
 (e) 64-bit offsets in a pool of more than 2^31 elements, and
 (f) the fast / generic rule, condition by condition and for the GPU cases.
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from varlen_cases import CASES, FAST

DT = {"fp32": 0, "fp16": 1, "bf16": 2}
BM = 64


def _cxx():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("c++"), shutil.which("g++")):
        if cand and os.path.exists(cand):
            return cand
    pytest.fail("no host C++ compiler")


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("varlen_plan") / "varlen_plan_check")
    cmd = [_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "host", "varlen_plan_check.cpp"), "-o", exe]
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


def cu_line(cu):
    return "cu {} {}".format(len(cu) - 1, " ".join(map(str, cu)))


# ---- (a) the tile map -----------------------------------------------------------
def numpy_tiles(q_lens, G):
    """[(b, tile)] in workgroup order"""
    tpt = BM // G
    return [[b, t] for b, n in enumerate(q_lens) for t in range(-(-int(n) // tpt))]


@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
def test_tile_map_against_numpy(checker, G):
    rng = np.random.default_rng(G)
    lines, want = [], []
    for batch in (1, 2, 5, 63, 64, 65, 255, 256, 257, 300):
        for style in range(3):
            # decode-heavy with zeros, prompt-heavy, and all zeros but one
            q_lens = (rng.integers(0, 3, batch) if style == 0 else rng.integers(0, 200, batch) if style == 1
                      else np.eye(1, batch, int(rng.integers(batch)), dtype=np.int64)[0] * 77).astype(np.int64)
            cu = np.concatenate([[0], np.cumsum(q_lens)])
            spare = int(rng.integers(0, 9))  # max_tokens may exceed the tokens in use
            lines += [cu_line(cu), "tiles {} {}".format(int(cu[-1]) + spare, G)]
            want.append((q_lens, int(cu[-1]) + spare, batch))
    got = ask(checker, lines)[1::2]
    for (q_lens, max_tokens, batch), g in zip(want, got):
        tiles = numpy_tiles(q_lens, G)
        assert g["upper"] == -(-max_tokens * G // BM) + batch
        assert g["upper"] >= len(tiles), "tiles_upper is never smaller than the tiles in use"
        assert g["map"][:len(tiles)] == tiles
        assert all(m == [-1, 0] for m in g["map"][len(tiles):]), "workgroups past the last tile find nothing"
        assert len(g["map"]) == g["upper"] + 3


def test_owner_of_a_token(checker):
    q_lens = [3, 0, 0, 5, 1, 0, 2]
    cu = np.concatenate([[0], np.cumsum(q_lens)])
    got = ask(checker, [cu_line(cu), "owner -2 14"])[1]["owner"]
    want = [-1, -1] + [b for b, n in enumerate(q_lens) for _ in range(n)] + [-1, -1, -1]
    assert got == want
    # a non-monotone cu never yields an owner that does not own the token
    cu = [0, 9, 4, 6, 2, 12]
    got = ask(checker, [cu_line(cu), "owner 0 14"])[1]["owner"]
    for t, b in enumerate(got):
        assert b == -1 or cu[b] <= t < cu[b + 1]


# ---- (b) key range and mask -----------------------------------------------------
SMALL = [(n_kv, q_len) for n_kv in (0, 1, 12, 31, 32, 33, 70, 200) for q_len in (1, 3, 16, 17, 20, 64, 70)]


@pytest.mark.parametrize("G", [1, 4, 16])
@pytest.mark.parametrize("causal", [1, 0])
def test_key_end_and_limits_against_a_brute_force_mask(checker, G, causal):
    tpt = BM // G
    got = ask(checker, ["mask {} {} {} {}".format(n_kv, q_len, G, causal) for n_kv, q_len in SMALL])
    for (n_kv, q_len), g in zip(SMALL, got):
        i, j = np.arange(q_len)[:, None], np.arange(max(n_kv, 1))[None, :]
        visible = np.broadcast_to(j < n_kv, (q_len, j.shape[1])) & ((j <= n_kv - q_len + i) if causal else np.True_)  # bottom-right
        last = np.where(visible.any(1), visible.shape[1] - 1 - np.argmax(visible[:, ::-1], axis=1), -1)
        assert g["limit"] == last.tolist(), (n_kv, q_len)
        assert visible.sum(1).tolist() == (last + 1).tolist()  # the visible keys of a row are a prefix
        ends = g["key_end"]
        assert len(ends) == -(-q_len // tpt)
        for t, end in enumerate(ends):
            rows = visible[t * tpt:(t + 1) * tpt]
            assert not rows[:, end:].any(), "no visible key lies at or past key_end"
            assert end == 0 or rows[:, end - 1].any(), "key_end is tight"
        if causal and n_kv < q_len:
            assert g["limit"][:q_len - n_kv] == [-1] * (q_len - n_kv), "n_kv < q_len rows see nothing"


# ---- (c) the append positions -----------------------------------------------------
def test_append_positions(checker):
    cases = [(18, 5, 32), (32, 16, 32), (7, 0, 32), (35, 6, 32), (2, 4, 32), (-3, 2, 32), (2 ** 31 - 1, 3, 2 ** 31 - 1),
             (-(2 ** 31), 2, 64)]
    got = ask(checker, ["append {} {} {}".format(*c) for c in cases])
    for (seq_len, q_len, cap), g in zip(cases, got):
        want = [seq_len - q_len + i for i in range(q_len)]
        assert g["pos"] == [p if 0 <= p < cap else -1 for p in want]
    assert got[3]["pos"] == [29, 30, 31, -1, -1, -1] and got[4]["pos"] == [-1, -1, 0, 1]


# ---- (d) the address clamps ---------------------------------------------------------
def sweep(checker, cu, lens, table, bs, nb, mb, max_tokens, H, Hkv, D, max_kv, causal=1, layers=2):
    B = len(lens)
    pool = (layers * bs * Hkv * D, Hkv * D, D)
    q_t, q_h = H * D, D
    g = ask(checker, [cu_line(cu), "lens {} {}".format(B, " ".join(map(str, lens))),
                      "table {} {} {} {} {}".format(bs, nb, mb, B, " ".join(map(str, np.asarray(table).ravel()))),
                      "pool {} {} {}".format(*pool),
                      "sweep {} {} {} {} {} {} {} {}".format(max_tokens, H, Hkv, D, max_kv, causal, q_t, q_h)])[-1]
    # every row starts inside its operand with a whole row after it
    assert 0 <= g["q"][0] and g["q"][1] <= (max_tokens - 1) * q_t + (H - 1) * q_h
    assert 0 <= g["table"][0] and g["table"][1] <= B * mb - 1
    if g["steps"]:
        assert 0 <= g["kv"][0] and g["kv"][1] <= (nb - 1) * pool[0] + (bs - 1) * pool[1] + (Hkv - 1) * pool[2]
    assert g["visible_past_end"] == 0
    return g


def test_addresses_of_a_well_formed_step(checker):
    q_lens, lens = [1, 1, 37, 0, 70], [513, 16, 37, 40, 200]
    cu = np.concatenate([[0], np.cumsum(q_lens)])
    rng = np.random.default_rng(0)
    table = rng.permutation(5 * 33).reshape(5, 33)
    g = sweep(checker, cu, lens, table, 16, 5 * 33, 33, int(cu[-1]) + 3, 8, 2, 128, 33 * 16)
    assert g["rows"] == int(cu[-1]) * 8 and g["stored"] == [0, int(cu[-1]) - 1] and g["dup"] == 0  # each row once


@pytest.mark.parametrize("D", [64, 128])
def test_address_clamps_under_malformed_device_tensors(checker, D):
    """a non-monotone cu_seqlens_q, negative and huge entries of it, lengths past max_kv and below 0, table
    entries out of range: every address stays inside its operand, and only live packed rows are stored"""
    bs, nb, mb, H, Hkv, max_tokens = 16, 6, 4, 8, 2, 40
    bad_tables = np.array([[-5, 6, 1_000_000, 2], [-(2 ** 31), 2 ** 31 - 1, 0, 5], [3, 3, 3, 3], [7, -1, 6, 9]])
    for cu in ([0, 30, 10, 25, 90], [5, 2, 2 ** 31 - 1, -7, 33], [-(2 ** 31), 2 ** 31 - 1, 0, 17, 12],
               [0, 0, 0, 0, 2 ** 31 - 1], [60, 70, 80, 90, 100]):
        for lens in ([1000, -4, 2 ** 31 - 1, 17], [64, 63, 65, 0], [-(2 ** 31), 5, 48, 49]):
            for max_kv in (mb * bs, 40, 0):
                g = sweep(checker, cu, lens, bad_tables, bs, nb, mb, max_tokens, H, Hkv, D, max_kv)
                live = max(0, min(cu[-1], max_tokens))
                if g["rows"]:
                    assert 0 <= g["stored"][0] and g["stored"][1] <= live - 1
                else:
                    assert g["stored"][0] > g["stored"][1]  # the empty range


# ---- (e) past 2^31 ----------------------------------------------------------------------
def test_offsets_past_2_31(checker):
    bs, nb, Hkv, D, layers = 16, 50_000, 8, 128, 3
    pool = (layers * bs * Hkv * D, Hkv * D, D)
    assert nb * pool[0] > 2 ** 31  # elements; never allocated
    lines = ["table {} {} 1 1 0".format(bs, nb), "pool {} {} {}".format(*pool)]
    probes = [(49_999, 15, 7), (43_691, 16, 0), (43_690, 31, 7), (0, 0, 0), (60_000, 3, 1), (-1, 3, 1)]
    got = ask(checker, lines + ["kvoff {} {} {}".format(*p) for p in probes])[2:]
    for (entry, key, hk), g in zip(probes, got):
        page = min(max(entry, 0), nb - 1)
        assert g["off"] == page * pool[0] + (key % bs) * pool[1] + hk * pool[2]  # Python integers
    assert got[0]["off"] > 2 ** 31 and got[1]["off"] >= 2 ** 31 > got[2]["off"]


# ---- (f) fast or generic ------------------------------------------------------------------
def strides_of(c, layers=2):
    """q_t q_h, k / v {page, token, head}, o_t o_h of packed contiguous q / o and a layer view of the pools"""
    kv = (layers * c.bs * c.Hkv * c.D, c.Hkv * c.D, c.D)
    return [c.H * c.D, c.D, *kv, *kv, c.H * c.D, c.D]


def fast_line(c, scale=None, aligned=1, strides=None):
    scale = c.D ** -0.5 if scale is None else scale
    return "fast {} {} {} {} {} {!r} {} {}".format(DT[c.dt], c.D, c.H, c.Hkv, c.bs, float(scale), aligned,
                                                   " ".join(map(str, strides or strides_of(c))))


def test_fast_or_generic_rule(checker):
    base = CASES["1"]
    odd = strides_of(base)
    odd[3] += 4  # a token stride off 16 bytes
    table = [
        (base, {}, True), (base._replace(dt="fp16"), {}, True), (base._replace(D=64), {}, True),
        (base._replace(bs=256), {}, True), (base._replace(bs=32), {}, True),
        *[(base._replace(H=2 * G), {}, True) for G in (1, 2, 4, 8, 16)],
        *[(base._replace(H=2 * G), {}, False) for G in (3, 5, 6, 7, 12, 32)],
        (base._replace(bs=24), {}, False), (base._replace(bs=8), {}, False),
        (base._replace(D=80), {}, False), (base._replace(D=256), {}, False), (base._replace(D=32), {}, False),
        (base._replace(dt="fp32"), {}, False),
        (base, {"scale": 0.0}, False), (base, {"scale": -0.1}, False),  # the MFMA kernel's max is of the raw scores
        (base, {"aligned": 0}, False), (base, {"strides": odd}, False),
    ]
    got = ask(checker, [fast_line(c, **kw) for c, kw, _ in table])
    assert [g["fast"] for g in got] == [w for _, _, w in table]
    # the GPU cases take the kernel their route names
    got = ask(checker, [fast_line(c) for c in CASES.values()])
    assert [g["fast"] for g in got] == [c.route == FAST for c in CASES.values()]
