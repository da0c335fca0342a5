"""The plan of the weight-only fp8 linear (csrc/fp8w_plan.h) on the CPU.

tests/host/fp8w_plan_check.cpp (built here with the host compiler, under
AddressSanitizer + UBSan where the compiler has them, and run directly; no
Python code runs under a sanitizer) replays the index arithmetic of
linear_fp8w_vec and linear_fp8w_smallm from the same functions the kernels
call.  Checked over a shape grid:
 (i)   every code of every row is consumed exactly once, and every row is
       stored by exactly one wave,
 (ii)  the X element paired with a code has the code's k,
 (iii) no load leaves the W operand [0, (n-1) ldw + k) or the X operand
       [0, (m-1) ldx + k),
 (iv)  the (ROWS, CPL) choice keeps 8 KiB per wave in flight,
 (v)   the route rule returns what include/pli.h says at each boundary, and the
       workspace sizes.
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

EMPTY, SMALLM, VEC, WIDEN, GENERIC, BAD_WS = 0, 1, 2, 3, 4, -1


def _cxx():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("c++"), shutil.which("g++")):
        if cand and os.path.exists(cand):
            return cand
    pytest.fail("no host C++ compiler")


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fp8w_plan") / "fp8w_plan_check")
    cmd = [_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "host", "fp8w_plan_check.cpp"), "-o", exe]
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
    assert not any("error" in o for o in out)
    return out


def check_replay(g, what):
    assert g["missing"] == 0, (what, "a code was never consumed")
    assert g["dup"] == 0, (what, "a code was consumed twice or lies outside its row")
    assert g["xk_mismatch"] == 0, (what, "an X element paired with a code of another k")
    assert g["unstored"] == 0, (what, "a row stored by no wave or by two")
    assert 0 <= g["w"][0] and g["w"][1] < g["w_extent"], (what, "W load outside the operand")
    assert 0 <= g["x"][0] and g["x"][1] < g["x_extent"], (what, "X load outside the operand")


def vec_cfg(k, swiglu):
    short = k <= 2048
    return ((2, 2) if short else (1, 4)) if swiglu else ((4, 2) if short else (2, 4))


@pytest.mark.parametrize("swiglu", [0, 1])
def test_vec_consumes_every_code_once(checker, swiglu):
    """K from one chunk to past two trips of 64 * CPL chunks on both sides of each boundary (every multiple of 16 the
    rule admits near them), N with 1 .. ROWS - 1 tail rows, M in {1, 2, 15, 16}, ldw > k, ldx > k"""
    ks = {16, 32, 16 * 63, 16 * 64, 16 * 65}
    for cpl in (2, 4):
        trip = 16 * 64 * cpl
        if cpl == 2:  # the short-row configuration ends at K = 2048 = one trip
            ks |= {trip - 16, trip}
        else:         # the long-row one starts past 2048
            ks |= {2048 + 16, trip - 16, trip, trip + 16, 2 * trip - 16, 2 * trip, 2 * trip + 16, 2 * trip + 16 * 65}
    cmds = []
    for k in sorted(ks):
        rows, _ = vec_cfg(k, swiglu)
        for n in sorted({1, 3, 4 * rows, 4 * rows + 1, 4 * rows + rows - 1, 4 * rows * 2 + rows + 1} | set(range(1, rows))):
            for m in ((1, 16) if k > 4096 else (1, 2, 15, 16)):
                for pad in (0, 48):
                    cmds.append((m, n, k, k + pad, k + (8 if pad else 0), swiglu))
    got = ask(checker, ["vec {} {} {} {} {} {}".format(*c) for c in cmds])
    for c, g in zip(cmds, got):
        check_replay(g, c)
        assert (g["rows"], g["cpl"]) == vec_cfg(c[2], swiglu)
        assert g["bytes_in_flight"] == 8192


def test_smallm_consumes_every_code_once(checker):
    """K = 1, 2, U, U + 1, 2 U + 1 body steps of 256; N = one and three 16-row groups; M on both sides of every
    batch-group count; ldw > k, ldx > k"""
    cmds = []
    for k in (256, 512, 256 * 8, 256 * 9, 256 * 17):
        for n in (16, 48):
            for m in (2, 15, 16, 17, 32, 33, 64, 65, 128):
                for pad in (0, 32):
                    cmds.append((m, n, k, k + pad, k + (8 if pad else 0)))
    got = ask(checker, ["smallm {} {} {} {} {}".format(*c) for c in cmds])
    for c, g in zip(cmds, got):
        check_replay(g, c)
        assert g["cpl"] == (1 if c[0] <= 16 else 2 if c[0] <= 32 else 4 if c[0] <= 64 else 8)
        assert g["bytes_in_flight"] >= 8192, "at least the bf16 small-M kernel's 8 KiB per wave"


def route(checker, **kw):
    a = dict(m=4, n=64, k=512, ldx=512, ldw=512, ldc=64, w=4096, x=8192, c=12288, bias=0, ws=0, ws_bytes=0, swiglu=0)
    a.update(kw)
    return ask(checker, ["route {m} {n} {k} {ldx} {ldw} {ldc} {w} {x} {c} {bias} {ws} {ws_bytes} {swiglu}".format(**a)])[0]


def test_route_rule(checker):
    r = lambda **kw: route(checker, **kw)["route"]  # noqa: E731
    # 1. empty
    assert r(k=0, ldx=0, ldw=0) == EMPTY and r(m=0) == EMPTY and r(n=0, ldc=0) == EMPTY
    # 2. smallm: 1 < m <= 128, k % 256 == 0, n % 16 == 0, aligned W / X / C, ldw % 16, ldx / ldc % 8
    assert r() == SMALLM and r(m=2) == SMALLM and r(m=128) == SMALLM and r(k=256, ldx=256, ldw=256) == SMALLM
    assert r(m=1) == VEC, "one row is the GEMV"
    assert r(k=384, ldx=384, ldw=384) == VEC, "k is not a multiple of the 256 step"
    assert r(n=24, ldc=24) == VEC and r(c=12288 + 8) == VEC and r(ldc=68) == VEC
    assert r(m=128, ldw=520) == GENERIC and r(w=4097) == GENERIC and r(ldx=516) == GENERIC and r(x=8200) == GENERIC
    # 3. vec: m <= 16, k % 16 == 0
    assert r(m=16, n=24, ldc=24) == VEC and r(m=17, n=24, ldc=24) == GENERIC
    assert r(m=1, k=40, ldx=40, ldw=48) == GENERIC and r(m=1, k=48, ldx=48, ldw=48) == VEC
    assert r(m=1, ldw=513) == GENERIC and r(m=1, w=4097) == GENERIC and r(m=1, ldx=516) == GENERIC
    # 4. widen + gemm: m > 16, no fast route, a workspace, pli_gemm's vector class
    big = dict(m=17, n=24, ldc=24, k=40, ldx=40, ldw=40)
    need = route(checker, **big)["need"]
    assert need == (24 * 40 * 2 + 15) // 16 * 16
    assert r(**big) == GENERIC, "no workspace"
    assert r(ws=1 << 20, ws_bytes=need, **big) == WIDEN
    assert r(ws=1 << 20, ws_bytes=need - 1, **big) == BAD_WS and r(ws=(1 << 20) + 8, ws_bytes=need, **big) == BAD_WS
    assert r(ws=1 << 20, ws_bytes=need, swiglu=1, **big) == BAD_WS and r(ws=1 << 20, ws_bytes=2 * need, swiglu=1, **big) == WIDEN
    assert r(ws=1 << 20, ws_bytes=need, **dict(big, k=36, ldx=40, ldw=40)) == GENERIC, "k % 8 != 0: not pli_gemm's class"
    assert r(ws=1 << 20, ws_bytes=need, **dict(big, x=8194)) == GENERIC and r(ws=1 << 20, ws_bytes=need, bias=4, **big) == GENERIC
    assert r(m=129, ws=1 << 20, ws_bytes=1 << 20) == WIDEN and r(m=129) == GENERIC
    assert r(m=16, ws=1 << 20, ws_bytes=0, n=24, ldc=24) == VEC, "a fast route ignores the workspace"


def test_workspace_sizes(checker):
    al = lambda b: (b + 15) // 16 * 16  # noqa: E731
    shapes = [(1, 64, 512), (16, 24, 40), (17, 64, 512), (128, 4096, 4096), (17, 24, 40), (128, 48, 384), (129, 64, 512),
              (4096, 32000, 2048), (64, 33, 256), (0, 64, 512), (64, 0, 512), (64, 64, 0)]
    got = ask(checker, ["wsize {} {} {} {}".format(m, n, k, s) for m, n, k in shapes for s in (0, 1)])
    it = iter(got)
    for m, n, k in shapes:
        fast = m <= 16 or (m <= 128 and k % 256 == 0 and n % 16 == 0) or n == 0 or k == 0
        for s in (0, 1):
            assert next(it)["bytes"] == (0 if fast else (1 + s) * al(n * k * 2)), (m, n, k, s)
