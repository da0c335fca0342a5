"""The plan of the fp8-activation kernels (csrc/fp8a_plan.h) on the CPU.

tests/host/fp8a_plan_check.cpp (built here with the host compiler, under AddressSanitizer + UBSan where the compiler
has them, and run directly; no Python code runs under a sanitizer) replays the tile map of gemm_fp8_mx and the
element map of quant_rows_fp8 from the same functions the kernels call.  Checked over the shapes of
tests/fp8a_cases.py:
 (i)   every (row, 16-byte k-chunk) of both operand images is staged exactly once per K-step, and every LDS offset
       lies inside the image,
 (ii)  every byte an MFMA operand slot reads is the k of the (clamped) row the slot stands for, and every staged
       chunk is read by exactly the two waves that share its block row / column,
 (iii) every clamped source address lies inside its operand [0, (rows - 1) ld + k),
 (iv)  every (r, j) of C is stored exactly once, none outside [m, n], every packed store 8-byte aligned,
 (v)   the route of every case and of every boundary of the rule,
 (vi)  the quantiser takes every element of a row once, and re-reads none up to its register-resident K.
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

import fp8a_cases as fc
from conftest import PKG, ROOT


def _cxx():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("c++"), shutil.which("g++")):
        if cand and os.path.exists(cand):
            return cand
    pytest.fail("no host C++ compiler")


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fp8a_plan") / "fp8a_plan_check")
    cmd = [_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "host", "fp8a_plan_check.cpp"), "-o", exe]
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
    assert not any("error" in o for o in out), out
    return out


def test_route_of_every_case(checker):
    cmds, want = [], []
    for c in fc.GEMM_CASES:
        ldx8, ldw, ldc = fc.leading_dims(c)
        w8 = 8192 + (1 if c.mode == "off1" else 0)
        cmds.append(f"route {c.m} {c.n} {c.k} {ldx8} {ldw} {ldc} 4096 {w8} 12288")
        want.append(fc.MX_R if c.kernel == fc.MX else fc.GENERIC_R)
    assert [g["route"] for g in ask(checker, cmds)] == want


def test_route_rule_boundaries(checker):
    def r(**kw):
        a = dict(m=64, n=128, k=256, ldx8=256, ldw=256, ldc=128, x8=4096, w8=8192, c=12288)
        a.update(kw)
        got = ask(checker, ["route {m} {n} {k} {ldx8} {ldw} {ldc} {x8} {w8} {c}".format(**a)])[0]["route"]
        assert got == fc.route(**a), (a, "the Python replay disagrees with the header")
        return got

    E, MX, G = fc.EMPTY_R, fc.MX_R, fc.GENERIC_R
    assert r() == MX
    assert r(m=0) == E and r(n=0, ldc=0) == E and r(k=0, ldx8=0, ldw=0) == E
    assert r(m=fc.MIN_M) == MX and r(m=fc.MIN_M - 1) == G and r(m=1) == G
    assert r(k=128, ldx8=128, ldw=128) == MX and r(k=192, ldx8=192, ldw=192) == G and r(k=40, ldx8=48, ldw=48) == G
    assert r(x8=4097) == G and r(w8=8200) == G and r(x8=4096 + 16) == MX
    assert r(ldx8=264) == G and r(ldx8=272) == MX and r(ldw=260) == G and r(ldw=304) == MX
    assert r(n=132, ldc=132) == MX and r(n=130, ldc=132) == G and r(ldc=130) == G and r(ldc=136) == MX
    assert r(c=12288 + 4) == G and r(c=12288 + 8) == MX
    assert r(m=1 << 20, n=4) == MX


def check_mx(g, what):
    assert g["stage_missing"] == 0 and g["stage_dup"] == 0, (what, "a chunk staged never or twice", g)
    assert g["lds_oob"] == 0, (what, "an LDS offset outside the image")
    assert g["frag_mismatch"] == 0, (what, "an operand slot reads a byte of another row or k")
    assert g["frag_count_bad"] == 0, (what, "a staged chunk is not read by exactly its two waves")
    assert 0 <= g["w"][0] and g["w"][1] < g["w_extent"], (what, "W load outside the operand", g)
    assert 0 <= g["x"][0] and g["x"][1] < g["x_extent"], (what, "X load outside the operand", g)
    assert g["c_missing"] == 0 and g["c_dup"] == 0 and g["c_oob"] == 0, (what, "C not stored exactly once", g)
    assert g["c_misaligned"] == 0, (what, "a packed store off its 8-byte boundary")
    assert g["lds_bytes"] == fc.STAGES * 2 * fc.TM * fc.KSTEP


def test_mx_tile_map_over_the_case_list(checker):
    shapes = []
    for c in fc.GEMM_CASES:
        if c.kernel == fc.MX:
            shapes.append((c.m, c.n, c.k) + fc.leading_dims(c))
    # the lane-map tests' shapes, and one with several tiles both ways
    shapes += [(256, 256, 128, 128, 128, 256), (fc.TM + 3, fc.TN + fc.STORE_N, 256, 256, 256, fc.TN + fc.STORE_N),
               (3 * fc.TM + 5, 2 * fc.TN + 8, 128, 144, 176, 2 * fc.TN + 12),
               # two full bands of m-tiles and a short one, three n-tiles
               ((2 * fc.GROUP_M + 4) * fc.TM + 5, 2 * fc.TN + 8, 128, 128, 128, 2 * fc.TN + 8)]
    shapes = sorted(set(shapes))
    got = ask(checker, ["mx {} {} {} {} {} {}".format(*s) for s in shapes])
    for s, g in zip(shapes, got):
        check_mx(g, s)
        assert g["tiles"] == -(-s[0] // fc.TM) * -(-s[1] // fc.TN)


def test_mx_replay_refuses_other_shapes(checker):
    r = subprocess.run([checker], input="mx 16 128 128 128 128 128\nmx 64 128 40 48 48 128\n", capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0 and all("error" in json.loads(ln) for ln in r.stdout.splitlines())


def test_quantiser_takes_every_element_once(checker):
    ks = sorted(set(fc.QUANT_KS) | {8, 24, 2040, 2056, fc.QUANT_REG_K - 8, 2 * fc.QUANT_REG_K + 16, 255, 257, 513})
    cmds = [(k, vec) for k in ks for vec in ((0, 1) if k % 8 == 0 else (0,))]
    got = ask(checker, [f"quant {k} {vec}" for k, vec in cmds])
    for (k, vec), g in zip(cmds, got):
        assert g["missing"] == 0 and g["dup"] == 0 and g["oob"] == 0, (k, vec, g)
        assert g["reg_k"] == fc.QUANT_REG_K
        if vec:  # held in registers up to the limit; past it only the excess is read again
            assert g["reread"] == max(0, k - fc.QUANT_REG_K), (k, g)
        else:
            assert g["reread"] == k
