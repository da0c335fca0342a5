"""Inputs and host oracles shared by the fp8 e4m3 KV-cache tests
(tests/test_fp8_codec.py on the CPU, tests/test_gpu_fp8_kv.py on the GPU).

The host oracle of the quantising append is torch's own cast behind an explicit
clamp: ``x.clamp(-448, 448).to(torch.float8_e4m3fn)``.  torch alone does not
saturate (500 -> NaN), hence the clamp; NaN passes through a clamp unchanged.
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import numpy as np
import torch

from conftest import PKG, ROOT

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def decode_table() -> torch.Tensor:
    """fp32 [256]: the value of every code (NaN at 127 and 255)"""
    return torch.arange(256, dtype=torch.int32).to(torch.uint8).view(FP8).float()


def edge_values() -> np.ndarray:
    """fp32 values that probe every rounding decision of the encoder: every representable value, every midpoint
    between neighbours (ties to even) and the fp32 neighbours of each midpoint, the subnormal range (multiples of
    2^-9, their midpoints, the tie at 2^-10 that rounds to zero, fp32 subnormals), +-0, +-448, the would-be midpoint
    464 and beyond, +-inf and NaN of both signs"""
    pos = decode_table()[:127].numpy().astype(np.float32)  # codes 0 .. 0x7E: 0 .. 448, ascending
    assert (np.diff(pos) > 0).all() and pos[-1] == FP8_MAX
    mids = ((pos[:-1].astype(np.float64) + pos[1:]) / 2).astype(np.float32)
    assert (mids.astype(np.float64) * 2 == pos[:-1].astype(np.float64) + pos[1:]).all()  # exact in fp32
    inf = np.float32(np.inf)
    around = [np.nextafter(mids, -inf), np.nextafter(mids, inf), np.nextafter(pos, inf), np.nextafter(pos[1:], -inf)]
    extra = np.array([2.0 ** -10, 2.0 ** -11, 1e-40, 1.4e-45, 464.0, 480.0, 500.0, 1e4, 3e38, np.inf], dtype=np.float32)
    extra = np.concatenate([extra, np.nextafter(extra[:5], inf), np.nextafter(extra[:5], -inf)])
    mag = np.concatenate([pos, mids, *around, extra]).astype(np.float32)
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    return np.concatenate([mag, -mag, nan]).astype(np.float32)


def torch_codes(x: torch.Tensor) -> torch.Tensor:
    """uint8 codes of fp32 x by torch: clamp to +-448, then the e4m3fn cast (round to nearest even)"""
    return x.float().clamp(-FP8_MAX, FP8_MAX).to(FP8).view(torch.uint8)


def spacing_of(codes: torch.Tensor) -> torch.Tensor:
    """fp32 spacing of the e4m3 grid at each (non-NaN) code: 2^-9 for subnormals and the first binade"""
    e = ((codes.to(torch.int32) >> 3) & 15).clamp(min=1)
    return torch.ldexp(torch.ones_like(e, dtype=torch.float32), e - 7 - 3)


def quantise(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """host model of the quantising append: x [..., heads, D] (any float dtype), scale fp32 [heads] ->
    uint8 codes of clamp(x * (1.0f / scale)), the reciprocal and the product in fp32"""
    inv = (torch.ones_like(scale, dtype=torch.float32) / scale.float())[:, None]
    return torch_codes(x.float() * inv)


def dequantise(codes: torch.Tensor, scale: torch.Tensor) -> np.ndarray:
    """float64 values of uint8 codes [..., heads, D]: exact decode times the fp32 scale"""
    return (decode_table().double()[codes.long()] * scale.double()[:, None]).numpy()


# ---- tests/host/fp8_codec_check.cpp: csrc/fp8_codec.h on the host ------------------------
def host_compiler():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("c++"), shutil.which("g++")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("no host C++ compiler")


def build_checker(directory, sanitize: bool) -> str:
    """build the driver into `directory`; with sanitize, under AddressSanitizer + UBSan where the compiler has them"""
    exe = os.path.join(str(directory), "fp8_codec_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "host", "fp8_codec_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(cmd + san if sanitize else cmd, capture_output=True, text=True)
    if r.returncode != 0 and sanitize:  # a compiler without the sanitizer runtimes: the plain build
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def ask(checker: str, lines):
    r = subprocess.run([checker], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def codec_codes(checker: str, x: np.ndarray) -> np.ndarray:
    """uint8 codes of fp32 x by fp8_e4m3_encode of csrc/fp8_codec.h, same shape"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    bits = x.reshape(-1).view(np.uint32)
    codes = ask(checker, ["encode " + " ".join(map(str, bits.tolist()))])[0]["codes"]
    return np.array(codes, dtype=np.uint8).reshape(x.shape)
