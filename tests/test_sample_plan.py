"""The host-replayable part of the sampling kernel (csrc/sample_plan.h) on the CPU.

tests/host/sample_plan_check.cpp (built here with the host compiler, under
AddressSanitizer + UBSan where the compiler has them, and run directly; no
Python code runs under a sanitizer) calls the functions the kernel calls:
 (i)   Philox4x32-10 against the three known-answer vectors;
 (ii)  the uniform u of (seed, offset, row) against the numpy oracle of
       tests/sample_cases.py over a sweep of seeds, offsets (negative and past
       2^32 among them) and rows;
 (iii) the key transform: strictly order-preserving over all 2^16 patterns of
       fp16 and of bf16 and over a sweep of fp32 patterns (denormals, +-0,
       +-inf), NaN at the lowest key, -0 on +0's key, the digits rebuilding the
       key from the top, the inverse giving the canonical value back;
 (iv)  the launch configuration: every element of a row taken exactly once, in
       index order, for every vocab of the case list and the limits;
 (v)   the fixed-point weight and the threshold product at their exact points.
"""
from __future__ import annotations

import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import sample_cases as sc
from conftest import PKG, ROOT


def _cxx():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("c++"), shutil.which("g++")):
        if cand and os.path.exists(cand):
            return cand
    pytest.fail("no host C++ compiler")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sample_plan") / "sample_plan_check")
    cmd = [_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "host", "sample_plan_check.cpp"), "-o", exe]
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


def f32_bits(x) -> int:
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


VECTORS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def test_philox_known_answers(checker):
    got = ask(checker, ["philox {} {} {} {} {} {}".format(*c, *k) for c, k, _ in VECTORS])
    for (c, k, want), g in zip(VECTORS, got):
        assert tuple(g["out"]) == want, (c, k)
        assert tuple(int(v) for v in sc.philox4x32_10(c, k)) == want, "the numpy oracle's Philox"


def test_uniform_equals_the_numpy_oracle_over_a_counter_sweep(checker):
    sweep = [(seed, off, row0) for seed in (0, 1, 0xFFFFFFFF, 0x1_0000_0000, 0x9E3779B97F4A7C15, 2 ** 64 - 1)
             for off in (0, 1, 255, 2 ** 31 - 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 2 ** 40 + 11, -1, -3)
             for row0 in (0, 31, 2 ** 32 - 40)]
    got = ask(checker, [f"u {s} {o} {r} 64" for s, o, r in sweep])
    seen = set()
    for (s, o, r), g in zip(sweep, got):
        rows = (np.arange(64, dtype=np.uint64) + np.uint64(r)) & np.uint64(0xFFFFFFFF)   # (the row word wraps too)
        want = sc.philox_u(s, o, rows)
        assert want.dtype == np.float32 and (want >= 0).all() and (want < 1).all()
        assert g["u_bits"] == [int(b) for b in want.view(np.uint32)], (s, o, r)
        seen.update(g["u_bits"])
    # offsets that agree mod 2^32 give one stream, and the streams are not degenerate
    assert got[sweep.index((1, 2 ** 32 + 7, 0))]["u_bits"] == ask(checker, ["u 1 7 0 64"])[0]["u_bits"]
    assert got[sweep.index((1, -1, 0))]["u_bits"] == got[sweep.index((1, 2 ** 32 - 1, 0))]["u_bits"]
    assert len(seen) > 0.5 * 64 * len(sweep)   # (offset pairs that coincide mod 2^32 and overlapping rows repeat values)


def test_key_transform_is_strictly_order_preserving(checker):
    f16, bf16, f32 = ask(checker, ["keys16 1", "keys16 2", "keys32 200000"])
    for name, g in (("fp16", f16), ("bf16", bf16), ("fp32", f32)):
        assert g["violations"] == 0, (name, "a pair of patterns ordered differently by key and by value")
        assert g["digit_mismatch"] == 0, (name, "the digits from the top do not rebuild the key")
        assert g["unkey_mismatch"] == 0, (name, "key -> value is not the inverse on canonical values")
        assert g["nan_not_lowest"] == 0, (name, "a NaN above -inf")
        assert 0 < g["lowest"] < g["highest"]
    # all patterns: 2 * (mantissas) NaNs fold onto -inf, -0 onto +0
    assert f16["n"] == bf16["n"] == 65536
    assert f16["distinct"] == 65536 - 2 * 1023 - 1 and bf16["distinct"] == 65536 - 2 * 127 - 1
    assert f32["n"] > 200000


def test_launch_configuration_takes_every_element_once_in_index_order(checker):
    vocabs = sorted(set(sc.VOCABS) | {sc.THREADS - 1, sc.THREADS, sc.THREADS + 1, 2 * sc.THREADS + 1,
                                      sc.MAX_VOCAB - 1, sc.MAX_VOCAB})
    got = ask(checker, [f"cover {v}" for v in vocabs])
    for v, g in zip(vocabs, got):
        assert g["missing"] == 0 and g["dup"] == 0 and g["disorder"] == 0, (v, g)
        assert (g["waves"], g["threads"], g["max_vocab"]) == (sc.WAVES, sc.THREADS, sc.MAX_VOCAB)
        assert g["steps"] == -(-v // sc.THREADS) and g["seg"] == 64 * g["steps"], (v, g)   # tight, whole steps
    assert all("error" in g for g in ask(checker, ["cover 0", f"cover {sc.MAX_VOCAB + 1}"]))
    assert sc.MAX_VOCAB * 2 ** sc.FRAC_BITS < 2 ** 64   # a row's weights cannot overflow their 64-bit sum


def test_fixed_point_weight_and_threshold(checker):
    one, ninf, inf = 2 ** sc.FRAC_BITS, f32_bits(-np.inf), f32_bits(np.inf)
    b = f32_bits
    got = ask(checker, [f"weight {b(1.5)} {b(1.5)} {b(0.25)}", f"weight {ninf} {b(1.5)} {b(1.0)}",
                        f"weight {ninf} {b(1.5)} {inf}", f"weight {b(-3.0)} {b(1.5)} {inf}",
                        f"weight {b(0.5)} {b(1.5)} {b(1.0)}", f"weight {b(-200.0)} {b(1.5)} {b(1.0)}",
                        f"scale {b(0.5)} {3 * one}", f"scale {b(0.0)} {one}", f"scale {b(float(sc.U_MAX))} {one}",
                        f"scale {b(0.9)} {2 ** 62 + 12345}"])
    assert [g.get("w") for g in got[:4]] == [one, 0, 0, one]
    w = got[4]["w"]   # exp(-1) to a few fp32 ulp, on the 2^-45 grid
    assert abs(w / one - np.exp(-1.0)) < 4 * 2.0 ** -24 and got[5]["w"] == 0
    assert [g["v"] for g in got[6:9]] == [3 * one // 2, 0, one - 2 ** (sc.FRAC_BITS - 24)]
    assert got[9]["v"] == int(float(np.float32(0.9)) * float(2 ** 62 + 12345))   # one fp64 product, then floor
