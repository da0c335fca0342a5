"""The argument rules of pli_rms_gemm_nt_fp8w (include/pli.h) without a GPU: the
symbol is declared and exported, every rule returns PLI_EINVAL with its message
before any HIP call (the data pointers are made up and never dereferenced), and
the Python wrappers and the model's guard say the same thing."""
from __future__ import annotations

import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT

EINVAL = 1000
F32, F16, BF16 = 0, 1, 2
P = 4096        # never dereferenced: validation fails first
ODD = 4104      # 8 bytes past a 16-byte boundary
VP, I64, INT = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
NAME = b"pli_rms_gemm_nt_fp8w"


@pytest.fixture()
def L(built_lib):
    import pli_hip
    return pli_hip.lib()


def _call(L, **kw):
    a = dict(a=P, lda=64, r=P, ldr=64, g=P, eps=1e-6, h=P, ldh=64, m=2, k=64, tpb=1, w=P, ws=P, wu=None, wus=None, c=P,
             n=16, ldw=64, sb=16, st=16, cap=8, ng=3, dtype=BF16, null=())
    a.update(kw)
    a = SimpleNamespace(**a)
    rep = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * 3  # noqa: E731
    arr = dict(w=(VP * 3)(*rep(a.w)), ws=(VP * 3)(*rep(a.ws)) if a.ws is not None else None,
               wu=(VP * 3)(*rep(a.wu)) if a.wu is not None else None,
               wus=(VP * 3)(*rep(a.wus)) if a.wus is not None else None, c=(VP * 3)(*rep(a.c)),
               n=(INT * 3)(*rep(a.n)), ldw=(I64 * 3)(*rep(a.ldw)), sb=(I64 * 3)(*rep(a.sb)), st=(I64 * 3)(*rep(a.st)),
               ro=(VP * 3)(None, P, P), cap=(INT * 3)(*rep(a.cap)))
    for name in a.null:  # a NULL array
        arr[name] = None
    return L.pli_rms_gemm_nt_fp8w(a.a, a.lda, a.r, a.ldr, a.g, a.eps, a.h, a.ldh, a.m, a.k, a.tpb, arr["w"], arr["ws"],
                                  arr["wu"], arr["wus"], arr["c"], arr["n"], arr["ldw"], arr["sb"], arr["st"],
                                  arr["ro"], arr["cap"], a.ng, a.dtype, None)


def test_symbol_declared_and_exported(L, built_lib):
    header = open(os.path.join(ROOT, "include", "pli.h")).read()
    assert re.search(r"\bint\s+pli_rms_gemm_nt_fp8w\(", header)
    assert getattr(ctypes.CDLL(built_lib), "pli_rms_gemm_nt_fp8w") is not None
    doc = header[header.index("/* pli_rms_gemm_nt_fp8w:"):header.index("int pli_rms_gemm_nt_fp8w(")]
    doc = " ".join(re.sub(r"\n \*", " ", doc).split())
    for text in ("1 <= m <= 4 rows", "k % 16 == 0, k <= 8192", "m * k * 2 + 16 bytes", "65552", "rms_gemm_fp8w<swiglu>",
                 "ldw_g >= k and % 16 == 0", "A NaN code makes exactly its output column NaN"):
        assert text in doc, text


def test_argument_rules_without_gpu(L):
    err = L.pli_last_error
    for name in ("a", "g"):
        assert _call(L, **{name: None}) == EINVAL and NAME + b": null pointer" in err(), name
    for name in ("w", "c", "n", "ldw", "sb", "st", "ro", "cap"):
        assert _call(L, null=(name,)) == EINVAL and NAME + b": null pointer" in err(), name
    for ng in (0, 4, -1):
        assert _call(L, ng=ng) == EINVAL and NAME + b": 1..3 groups" in err(), ng
    for kw in (dict(m=0), dict(m=5), dict(m=-1), dict(tpb=0), dict(m=3, tpb=2), dict(m=4, tpb=3)):
        assert _call(L, **kw) == EINVAL and NAME + b": needs 1 <= m <= 4 rows" in err(), kw
    shape = (dict(k=0), dict(k=-16), dict(k=56), dict(k=72, lda=72, ldr=72, ldh=72, ldw=80),  # k % 8 == 0 is not enough
             dict(k=8208, lda=8208, ldr=8208, ldh=8208, ldw=8208),
             dict(lda=48), dict(lda=68), dict(ldr=48), dict(ldr=68), dict(ldh=48), dict(ldh=68),
             dict(a=ODD), dict(g=ODD), dict(r=ODD), dict(h=ODD))
    for kw in shape:
        assert _call(L, **kw) == EINVAL and NAME + b": needs k % 16 == 0, k <= 8192, 16-byte aligned rows" in err(), kw
    for dt in (F32, 7, -1):
        assert _call(L, dtype=dt) == EINVAL and NAME + b": bf16/fp16 only" in err(), dt
    for eps in (-1e-6, float("nan"), float("inf")):
        assert _call(L, eps=eps) == EINVAL and NAME + b": bad eps" in err(), eps
    bad = ((1, dict(w=[P, None, P])), (2, dict(c=[P, P, None])), (1, dict(n=[16, 0, 16])), (2, dict(n=[16, 16, -1])),
           (1, dict(ldw=[64, 48, 64])), (1, dict(ldw=[64, 72, 64])),  # below k; % 8 == 0 but not % 16
           (1, dict(w=[P, ODD, P])), (1, dict(wu=[P, None, P])), (2, dict(wu=[P, P, ODD])), (0, dict(ng=1, n=[0, 16, 16])))
    for g, kw in bad:
        assert _call(L, **kw) == EINVAL and NAME + b": bad group %d" % g in err(), kw
    assert L.pli_last_route() == b""  # nothing was launched


def test_largest_shape_and_optional_operands_pass_the_shape_rules(L):
    """m = 4 with k = 8192 (65536 + 16 bytes of LDS), no residual, no h_out (their strides are then not read), NULL
    scale arrays and entries: each reaches the group loop, where a made-up bad group stops the call"""
    err = L.pli_last_error
    big = dict(m=4, k=8192, lda=8192, ldr=8192, ldh=8192, ldw=8192)
    assert _call(L, n=[16, 0, 16], **big) == EINVAL and b"bad group 1" in err()
    assert _call(L, r=None, ldr=0, h=None, ldh=0, n=[16, 16, 0]) == EINVAL and b"bad group 2" in err()
    assert _call(L, ws=None, n=[16, 16, 0]) == EINVAL and b"bad group 2" in err()
    assert _call(L, ws=[P, None, P], wu=P, wus=[None, P, None], n=[16, 16, 0]) == EINVAL and b"bad group 2" in err()
    assert L.pli_last_route() == b""


def test_wrappers_refuse_cpu_tensors_and_bad_pos(built_lib):
    import pli_hip
    bf = torch.bfloat16
    x, g = torch.zeros(2, 64, dtype=bf), torch.ones(64, dtype=bf)
    codes, scale = pli_hip.quantize_weight_fp8(torch.ones(16, 64))
    kc = torch.zeros(2, 8, 2, 8, dtype=bf)
    q = torch.zeros(2, 1, 16, dtype=bf)
    pos = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.rms_linear_fp8w(x, g, 1e-6, codes, scale)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.rms_swiglu_fp8w(x, g, 1e-6, codes, scale, codes, None)
    for bad in (pos, pos.long()):
        with pytest.raises(pli_hip.PliError, match="pos must be an int32 device tensor"):
            pli_hip.rms_qkv_into_cache_fp8w(x.view(2, 1, 64), g, 1e-6, (codes, scale), (codes, scale), (codes, None), q,
                                            kc, kc, bad)


def test_model_guard_is_the_entry_points_rule():
    """Fp8WeightModel._fused_decode_ok: off by default; with fused_decode the 16-bit model's conditions plus
    hidden % 16 == 0"""
    from ch02 import CachedTransformerModel
    from ch02.fp8_weight_model import Fp8WeightModel

    def ok(B, S, hd, fused=True, heads=None):
        heads = heads or max(1, hd // 64)
        blk = SimpleNamespace(num_heads=heads, num_kv_heads=heads, head_dim=hd // heads)
        model = SimpleNamespace(fused_decode=fused, layers=[blk])
        x = torch.empty(B, S, hd, dtype=torch.bfloat16, device="meta")
        return Fp8WeightModel._fused_decode_ok(model, x, [SimpleNamespace(pos=object())])

    assert ok(4, 1, 8192) and ok(1, 4, 8192) and ok(2, 2, 8192) and ok(1, 1, 64)
    assert not ok(1, 1, 64, fused=False)
    assert not ok(5, 1, 64) and not ok(1, 1, 8192 + 64) and not ok(1, 5, 2048)
    # hidden 72 is % 8 == 0 but not % 16 == 0: the 16-bit guard takes it, the fp8 guard does not
    blk = SimpleNamespace(num_heads=1, num_kv_heads=1, head_dim=64)
    x = torch.empty(1, 1, 72, dtype=torch.bfloat16, device="meta")
    caches = [SimpleNamespace(pos=object())]
    assert not Fp8WeightModel._fused_decode_ok(SimpleNamespace(fused_decode=True, layers=[blk]), x, caches)
    sixteen = SimpleNamespace(layers=[SimpleNamespace(attn=blk)])
    assert CachedTransformerModel._fused_decode_ok(sixteen, x, caches), "the 16-bit rule alone takes k % 8 == 0"
    assert not Fp8WeightModel._fused_decode_ok(SimpleNamespace(fused_decode=True, layers=[blk]), x, None)
