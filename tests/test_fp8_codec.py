"""The fp8 e4m3fn codec and the fp8 fast / generic rules, on the CPU.

csrc/fp8_codec.h is pure C++ that the generic fp8 kernels run on the device
and that the hardware conversions of the fast kernels and the quantising
appends are compared against (tests/test_gpu_fp8_kv.py).
tests/host/fp8_codec_check.cpp (built here with the host compiler, under
AddressSanitizer + UBSan where the compiler has them; no Python code runs
under a sanitizer) prints it, and this file checks
 (a) the decode of all 256 codes against torch's float8_e4m3fn,
 (b) the encode of every representable value, every tie, the fp32 neighbours
     of every tie, the subnormal range, +-0, saturation, +-inf and NaN against
     torch's cast behind a clamp (tests/fp8_cases.py), and
 (c) the fp8 fast / generic rules of paged_plan.h / varlen_plan.h: the verdict
     of the 16-bit rule for every GPU case, and their own rejections.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import paged_cases
import varlen_cases
from fp8_cases import ask, build_checker, codec_codes, decode_table, edge_values, torch_codes

DT = {"fp32": 0, "fp16": 1, "bf16": 2}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("fp8_codec"), sanitize=True)


def encode(checker, x: np.ndarray) -> np.ndarray:
    return codec_codes(checker, x)


# ---- (a) decode -------------------------------------------------------------------
def test_decode_of_every_code(checker):
    got = np.array(ask(checker, ["decode"])[0]["bits"], dtype=np.uint32).view(np.float32)
    want = decode_table().numpy()
    nan = np.isnan(want)
    assert np.flatnonzero(nan).tolist() == [127, 255] and np.flatnonzero(np.isnan(got)).tolist() == [127, 255]
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))  # bitwise: -0 is 0x80
    assert got[0x7E] == 448.0 and got[0xFE] == -448.0 and got[1] == 2.0 ** -9 and got[8] == 2.0 ** -6
    # every value is a bf16 and an fp16 value: the fast kernels' widening is exact
    t = torch.from_numpy(got[~nan])
    assert torch.equal(t.bfloat16().float(), t) and torch.equal(t.half().float(), t)


# ---- (b) encode -------------------------------------------------------------------
def test_round_trip_of_every_code(checker):
    vals = decode_table().numpy()
    assert encode(checker, vals).tolist() == list(range(256))


def test_encode_of_the_edge_values_against_torch(checker):
    x = edge_values()
    got = encode(checker, x)
    want = torch_codes(torch.from_numpy(x)).numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(x[i]), int(got[i]), int(want[i])) for i in bad[:10]]
    nan = np.isnan(x)
    assert nan.sum() == 4 and set(got[nan].tolist()) == {0x7F, 0xFF}
    assert (got[nan] >> 7).tolist() == (x[nan].view(np.uint32) >> 31).tolist()  # a NaN keeps its sign
    assert not np.isin(got[~nan], (0x7F, 0xFF)).any()


def test_named_encodings(checker):
    x = np.array([0.0, -0.0, 448.0, -448.0, 464.0, -464.0, 500.0, 1e30, np.inf, -np.inf, 2.0 ** -10, 2.0 ** -10 * 1.0001,
                  3 * 2.0 ** -10, 0.0625 + 2.0 ** -8, 1e-40, -1e-40, 17.0, 19.0], dtype=np.float32)
    want = [0x00, 0x80, 0x7E, 0xFE, 0x7E, 0xFE, 0x7E, 0x7E, 0x7E, 0xFE, 0x00, 0x01,
            0x02, 0x18, 0x00, 0x80, 0x58, 0x5A]  # ties to even: 1.5 * 2^-9 -> 2 * 2^-9, 2^-4 + 2^-8 -> 2^-4, 17 -> 16, 19 -> 20
    got = encode(checker, x)
    assert got.tolist() == torch_codes(torch.from_numpy(x)).tolist()
    assert got.tolist() == want


# ---- (c) the fp8 fast / generic rules ---------------------------------------------------
def paged_strides(c, layers=2):
    q = (c.Sq * c.H * c.D, c.D, c.H * c.D)
    kv = (layers * c.bs * c.Hkv * c.D, c.Hkv * c.D, c.D)
    return [*q, *kv, *kv, *q]


def paged_line(c, aligned=1, strides=None):
    return "paged {} {} {} {} {!r} {} {}".format(DT[c.dt], c.D, c.Sq * (c.H // c.Hkv), c.bs, float(c.D ** -0.5), aligned,
                                                 " ".join(map(str, strides or paged_strides(c))))


def varlen_strides(c, layers=2):
    kv = (layers * c.bs * c.Hkv * c.D, c.Hkv * c.D, c.D)
    return [c.H * c.D, c.D, *kv, *kv, c.H * c.D, c.D]


def varlen_line(c, aligned=1, strides=None):
    return "varlen {} {} {} {} {} {!r} {} {}".format(DT[c.dt], c.D, c.H, c.Hkv, c.bs, float(c.D ** -0.5), aligned,
                                                     " ".join(map(str, strides or varlen_strides(c))))


def test_every_gpu_case_gets_the_verdict_of_its_16_bit_rule(checker):
    got = ask(checker, [paged_line(c) for c in paged_cases.CASES.values()])
    assert [g["fast_fp8"] for g in got] == [g["fast"] for g in got] == [c.route != paged_cases.GENERIC
                                                                        for c in paged_cases.CASES.values()]
    got = ask(checker, [varlen_line(c) for c in varlen_cases.CASES.values()])
    assert [g["fast_fp8"] for g in got] == [g["fast"] for g in got] == [c.route == varlen_cases.FAST
                                                                        for c in varlen_cases.CASES.values()]


def test_fp8_rule_rejections(checker):
    """a pool stride of 8 bytes (fine for 16-bit elements, half a 16-byte chunk of codes) and an unaligned pool"""
    for line, strides, pool in ((paged_line, paged_strides, range(3, 9)), (varlen_line, varlen_strides, range(2, 8))):
        c = (paged_cases if line is paged_line else varlen_cases).CASES["1"]
        base = strides(c)
        lines = [line(c), line(c, aligned=0)]
        for i in pool:
            s = list(base)
            s[i] += 8
            lines.append(line(c, strides=s))
        qo = list(base)
        qo[0] += 8  # q / o strides stay multiples of 8 elements
        odd_q = list(base)
        odd_q[0] += 4
        got = ask(checker, lines + [line(c, strides=qo), line(c, strides=odd_q)])
        assert got[0] == {"fast": True, "fast_fp8": True} and got[1] == {"fast": False, "fast_fp8": False}
        assert all(g == {"fast": True, "fast_fp8": False} for g in got[2:8])
        assert got[8] == {"fast": True, "fast_fp8": True} and got[9] == {"fast": False, "fast_fp8": False}
