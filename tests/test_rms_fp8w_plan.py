"""The plan of the fused RMSNorm + fp8-weight projection (csrc/rms_fp8w_plan.h) on
the CPU.

tests/host/rms_fp8w_plan_check.cpp (built here with the host compiler, under
AddressSanitizer + UBSan where the compiler has them, and run directly; no
Python code runs under a sanitizer) replays the index arithmetic of
rms_gemm_fp8w from the same functions the kernel and its launcher call.
Checked over K x group widths x SwiGLU x ldw:
 (i)   every code of every (group, row) is consumed exactly once and paired
       with the LDS X element of its own k,
 (ii)  every (group, row) is stored by exactly one wave,
 (iii) no weight load leaves its group's operand [0, (n_g - 1) ldw + k) and no
       X load the m * k LDS image,
 (iv)  the grid is the launcher's and is tight, the (ROWS, CPL) form is
       fp8w_vec_cfg's, the norm's RPT covers the row.
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

KS = (16, 32, 1008, 1024, 1040, 2032, 2048, 2064, 4080, 4096, 4112, 6160, 8176, 8192)
WIDTHS = ((1,), (10,), (5, 3, 2), (16, 16, 16), (17, 1, 1))


def _cxx():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("c++"), shutil.which("g++")):
        if cand and os.path.exists(cand):
            return cand
    pytest.fail("no host C++ compiler")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rms_fp8w_plan") / "rms_fp8w_plan_check")
    cmd = [_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "host", "rms_fp8w_plan_check.cpp"), "-o", exe]
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


def vec_cfg(k, swiglu):
    short = k <= 2048
    return ((2, 2) if short else (1, 4)) if swiglu else ((4, 2) if short else (2, 4))


@pytest.mark.parametrize("swiglu", [0, 1])
def test_every_code_once_every_row_once_nothing_out_of_bounds(checker, swiglu):
    cmds = []
    for k in KS:
        for widths in WIDTHS:
            for pad in (0, 48):
                for m in ((1, 4) if k in (16, 2048, 2064, 8192) else (3,)):
                    n = list(widths) + [0] * (3 - len(widths))
                    cmds.append((m, k, swiglu, k + pad, len(widths), *n))
    got = ask(checker, ["rms {} {} {} {} {} {} {} {}".format(*c) for c in cmds])
    for c, g in zip(cmds, got):
        assert "error" not in g, c
        m, k = c[0], c[1]
        ntot = sum(c[5:])
        rows, cpl = vec_cfg(k, swiglu)
        assert (g["rows"], g["cpl"]) == (rows, cpl), c
        assert g["missing"] == 0, (c, "a code was never consumed")
        assert g["dup"] == 0, (c, "a code was consumed twice or lies outside its row")
        assert g["xk_mismatch"] == 0, (c, "an X element paired with a code of another k")
        assert g["unstored"] == 0, (c, "a (group, row) stored by no wave or by two")
        assert g["w_oob"] == 0, (c, "a weight load outside its group's operand")
        assert g["x_oob"] == 0, (c, "an X load outside the LDS image")
        assert g["clamp_mismatch"] == 0, (c, "a stored row was loaded from another row")
        assert g["grid"] == -(-ntot // (4 * rows)) and g["grid_tight"] == 1, (c, g["grid"])
        assert g["active_waves"] == -(-ntot // rows), c
        assert g["lds_bytes"] == m * k * 2 <= 65536, c
        assert g["rpt"] == (1 if k <= 2048 else 2 if k <= 4096 else 4) and g["norm_cover"] == 1, c


def test_checker_refuses_what_the_entry_point_refuses(checker):
    bad = ["rms 5 64 0 64 1 4 0 0", "rms 1 24 0 32 1 4 0 0", "rms 1 8208 0 8208 1 4 0 0", "rms 1 64 0 48 1 4 0 0",
           "rms 1 64 0 64 4 4 4 4", "rms 1 64 0 64 2 4 0 0", "rms 0 64 0 64 1 4 0 0"]
    assert all("error" in g for g in ask(checker, bad))
