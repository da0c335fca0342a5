"""The argument rules of the decode-step entry points of include/pli.h without
a GPU: each PLI_REQUIRE of pli_rms_gemm_nt, pli_gemm_multi_nt, pli_kv_append,
pli_rmsnorm and pli_attn_decode_dev returns its status with its message before
any HIP call (the data pointers are never dereferenced), the guards of the
fused path say the same thing in C, in Python and in the header, and the
Python wrappers refuse CPU tensors, a non-int32 pos and mismatched caches."""
from __future__ import annotations

import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT

EINVAL, EUNSUPPORTED, OK = 1000, 1001, 0
F32, F16, BF16 = 0, 1, 2
P = 4096        # never dereferenced: validation fails first
ODD = 4104      # 8 bytes past a 16-byte boundary
VP, I64, INT = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


@pytest.fixture()
def L(built_lib):
    import pli_hip
    return pli_hip.lib()


def _groups(ng, w, wu, c, n, ldw, sb, st, cap):
    rep = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * 3  # noqa: E731
    return dict(w=(VP * 3)(*rep(w)), wu=(VP * 3)(*rep(wu)) if wu is not None else None, c=(VP * 3)(*rep(c)),
                n=(INT * 3)(*rep(n)), ldw=(I64 * 3)(*rep(ldw)), sb=(I64 * 3)(*rep(sb)), st=(I64 * 3)(*rep(st)),
                ro=(VP * 3)(None, P, P), cap=(INT * 3)(*rep(cap)), ng=ng)


def _rms(L, **kw):
    a = dict(a=P, lda=64, r=P, ldr=64, g=P, eps=1e-6, h=P, ldh=64, m=2, k=64, tpb=1, w=P, wu=None, c=P, n=16, ldw=64,
             sb=16, st=16, cap=8, ng=3, dtype=BF16, arrays=True)
    a.update(kw)
    a = SimpleNamespace(**a)
    G = _groups(a.ng, a.w, a.wu, a.c, a.n, a.ldw, a.sb, a.st, a.cap)
    if not a.arrays:
        G = dict(G, w=None)
    return L.pli_rms_gemm_nt(a.a, a.lda, a.r, a.ldr, a.g, a.eps, a.h, a.ldh, a.m, a.k, a.tpb, G["w"], G["wu"], G["c"],
                             G["n"], G["ldw"], G["sb"], G["st"], G["ro"], G["cap"], a.ng, a.dtype, None)


def _multi(L, **kw):
    a = dict(x=P, ldx=128, m=4, k=128, tpb=1, w=P, c=P, n=16, ldw=128, sb=16, st=16, cap=8, ng=3, dtype=BF16)
    a.update(kw)
    a = SimpleNamespace(**a)
    G = _groups(a.ng, a.w, None, a.c, a.n, a.ldw, a.sb, a.st, a.cap)
    return L.pli_gemm_multi_nt(a.x, a.ldx, a.m, a.k, a.tpb, G["w"], G["c"], G["n"], G["ldw"], G["sb"], G["st"], G["ro"],
                               G["cap"], a.ng, a.dtype, None)


def _append(L, **kw):
    a = dict(kn=P, vn=P, kc=P, vc=P, B=2, T=1, Hkv=2, D=64, cap=8, strides=[128] * 12, pos=P, dtype=BF16)
    a.update(kw)
    a = SimpleNamespace(**a)
    return L.pli_kv_append(a.kn, a.vn, a.kc, a.vc, a.B, a.T, a.Hkv, a.D, a.cap, (I64 * 12)(*a.strides), a.pos, a.dtype,
                           None)


def _norm(L, **kw):
    a = dict(x=P, r=P, w=P, y=P, h=P, rows=2, n=64, ldx=64, ldr=64, ldy=64, ldh=64, eps=1e-6, dtype=BF16)
    a.update(kw)
    a = SimpleNamespace(**a)
    return L.pli_rmsnorm(a.x, a.r, a.w, a.y, a.h, a.rows, a.n, a.ldx, a.ldr, a.ldy, a.ldh, a.eps, a.dtype, None)


def _attn(L, **kw):
    a = dict(q=P, k=P, v=P, o=P, B=1, H=8, Hkv=2, nq=1, nmax=64, D=128, strides=[1024] * 12, scale=0.1, causal=0,
             ndev=P, add=1, ws=None, ws_bytes=0, dtype=BF16)
    a.update(kw)
    a = SimpleNamespace(**a)
    return L.pli_attn_decode_dev(a.q, a.k, a.v, a.o, a.B, a.H, a.Hkv, a.nq, a.nmax, a.D, (I64 * 12)(*a.strides), a.scale,
                                 a.causal, a.ndev, a.add, a.ws, a.ws_bytes, a.dtype, None)


def test_symbols_declared_and_exported(L):
    header = open(os.path.join(ROOT, "include", "pli.h")).read()
    for name in ("pli_rms_gemm_nt", "pli_gemm_multi_nt", "pli_kv_append", "pli_rmsnorm", "pli_attn_decode_dev"):
        assert re.search(r"\bint\s+" + name + r"\(", header), name
        assert getattr(L, name) is not None


def test_rms_gemm_nt_argument_rules_without_gpu(L):
    err = L.pli_last_error
    for name in ("a", "g"):
        assert _rms(L, **{name: None}) == EINVAL and b"pli_rms_gemm_nt: null pointer" in err(), name
    assert _rms(L, arrays=False) == EINVAL and b"null pointer" in err()
    for ng in (0, 4, -1):
        assert _rms(L, ng=ng) == EINVAL and b"1..3 groups" in err(), ng
    for kw in (dict(m=0), dict(m=5), dict(m=-1), dict(tpb=0), dict(m=3, tpb=2), dict(m=4, tpb=3)):
        assert _rms(L, **kw) == EINVAL and b"1 <= m <= 4 rows" in err(), kw
    shape = (dict(k=0), dict(k=-8), dict(k=60, lda=64), dict(k=8200, lda=8200, ldr=8200, ldh=8200, ldw=8200),
             dict(lda=56), dict(lda=68), dict(ldr=56), dict(ldr=68), dict(ldh=56), dict(ldh=68),
             dict(a=ODD), dict(g=ODD), dict(r=ODD), dict(h=ODD))
    for kw in shape:
        assert _rms(L, **kw) == EINVAL and b"k % 8 == 0, k <= 8192, 16-byte aligned rows" in err(), kw
    for dt in (F32, 7, -1):
        assert _rms(L, dtype=dt) == EINVAL and b"bf16/fp16 only" in err(), dt
    for eps in (-1e-6, float("nan"), float("inf")):
        assert _rms(L, eps=eps) == EINVAL and b"bad eps" in err(), eps
    bad = ((1, dict(w=[P, None, P])), (2, dict(c=[P, P, None])), (1, dict(n=[16, 0, 16])), (2, dict(n=[16, 16, -1])),
           (1, dict(ldw=[64, 56, 64])), (1, dict(ldw=[64, 68, 64])), (1, dict(w=[P, ODD, P])), (1, dict(wu=[P, None, P])),
           (2, dict(wu=[P, P, ODD])), (0, dict(ng=1, n=[0, 16, 16])))
    for g, kw in bad:
        assert _rms(L, **kw) == EINVAL and b"pli_rms_gemm_nt: bad group %d" % g in err(), kw
    assert L.pli_last_route() == b""  # nothing was launched


def test_fused_guards_agree_in_c_python_and_header(L):
    """1 <= m <= 4, k % 8 == 0, k <= 8192: the C guard (above: m = 5 and k = 8200 refused; m = 4 with k = 8192 passes
    every rule up to the group check), _fused_decode_ok and the text of include/pli.h"""
    err = L.pli_last_error
    # m = 4, k = 8192 reaches the group loop: the shape rules accept it (65536 + 16 bytes of LDS of gfx950's 160 KiB)
    big = dict(m=4, k=8192, lda=8192, ldr=8192, ldh=8192, ldw=8192)
    assert _rms(L, n=[16, 0, 16], **big) == EINVAL and b"bad group 1" in err()
    header = open(os.path.join(ROOT, "include", "pli.h")).read()
    doc = header[header.index("/* pli_rms_gemm_nt:"):header.index("int pli_rms_gemm_nt(")]
    doc = " ".join(re.sub(r"\n \*", " ", doc).split())
    assert "1 <= m <= 4 rows" in doc and "k % 8 == 0, k <= 8192" in doc and "m * k * 2 + 16 bytes" in doc

    import ch02.cached_generation as cg
    from ch02 import CachedTransformerModel

    def ok(B, S, hd):
        model = SimpleNamespace(layers=[SimpleNamespace(attn=SimpleNamespace(num_heads=hd // 64, num_kv_heads=hd // 64,
                                                                             head_dim=64))])
        x = torch.empty(B, S, hd, dtype=torch.bfloat16, device="meta")
        caches = [SimpleNamespace(pos=object())]
        return CachedTransformerModel._fused_decode_ok(model, x, caches)

    assert cg.FUSED_DECODE
    assert ok(4, 1, 8192) and ok(1, 4, 8192) and ok(2, 2, 8192) and ok(1, 1, 64)
    assert not ok(5, 1, 64) and not ok(1, 1, 8192 + 64) and not ok(1, 5, 2048)


def test_gemm_multi_nt_argument_rules_without_gpu(L):
    err = L.pli_last_error
    assert _multi(L, x=None) == EINVAL and b"pli_gemm_multi_nt: null pointer" in err()
    for ng in (0, 4):
        assert _multi(L, ng=ng) == EINVAL and b"1..3 groups" in err(), ng
    for kw in (dict(m=0), dict(m=129), dict(k=0), dict(k=100, ldx=104), dict(ldx=120), dict(ldx=132), dict(tpb=0),
               dict(m=4, tpb=3), dict(x=ODD)):
        assert _multi(L, **kw) == EINVAL and b"1 <= m <= 128 rows (whole batches)" in err(), kw
    assert _multi(L, m=17, k=192, ldx=192, ldw=192) == EINVAL and b"m > 16 needs k % 128 == 0" in err()
    assert _multi(L, m=16, k=192, ldx=192, ldw=192, n=[16, 0, 16]) == EINVAL and b"bad group 1" in err()  # m 16: k % 8 is enough
    for dt in (F32, 9):
        assert _multi(L, dtype=dt) == EINVAL and b"bf16/fp16 only" in err(), dt
    for kw in (dict(w=[P, None, P]), dict(c=[P, None, P]), dict(n=[16, 0, 16]), dict(ldw=[128, 120, 128]),
               dict(ldw=[128, 132, 128]), dict(w=[P, ODD, P])):
        assert _multi(L, **kw) == EINVAL and b"pli_gemm_multi_nt: bad group 1" in err(), kw
    # the m > 16 clauses one by one (each passes at m = 16 up to a later group's rule)
    for kw in (dict(n=[16, 24, 16]), dict(sb=[16, 18, 16]), dict(st=[16, 18, 16]), dict(c=[P, P + 4, P])):
        assert _multi(L, m=17, **kw) == EINVAL and b"m > 16 needs group widths % 16 == 0" in err(), kw
        assert b"(group 1)" in err()
        assert _multi(L, m=16, **dict(kw, w=[P, P, None])) == EINVAL and b"bad group 2" in err(), kw
    assert L.pli_last_route() == b""


def test_kv_append_argument_rules_without_gpu(L):
    err = L.pli_last_error
    for kw in (dict(B=-1), dict(T=-1), dict(Hkv=0), dict(D=0), dict(cap=-1)):
        assert _append(L, **kw) == EINVAL and b"pli_kv_append: bad shape" in err(), kw
    assert _append(L, B=0, kn=None, vn=None, kc=None, vc=None, pos=None) == OK
    assert _append(L, T=0, kn=None, vn=None, kc=None, vc=None, pos=None) == OK
    for name in ("kn", "vn", "kc", "vc", "pos"):
        assert _append(L, **{name: None}) == EINVAL and b"pli_kv_append: null pointer" in err(), name
    for dt in (F32, 5):
        assert _append(L, dtype=dt) == EINVAL and b"16-bit caches only" in err(), dt
    for kw in (dict(D=12), dict(D=4), dict(kn=ODD), dict(vn=ODD), dict(kc=ODD), dict(vc=ODD)):
        assert _append(L, **kw) == EINVAL and b"head_dim % 8 and 16-byte aligned operands" in err(), kw
    for i in range(12):
        st = [128] * 12
        st[i] = 132
        assert _append(L, strides=st) == EINVAL and b"stride %d not a multiple of 8" % i in err(), i
    assert L.pli_last_route() == b""


def test_rmsnorm_argument_rules_without_gpu(L):
    err = L.pli_last_error
    for kw in (dict(rows=-1), dict(n=0), dict(n=-8), dict(rows=1 << 31)):
        assert _norm(L, **kw) == EINVAL and b"pli_rmsnorm: bad shape" in err(), kw
    for kw in (dict(ldx=63), dict(ldy=63), dict(ldr=63), dict(ldh=63)):
        assert _norm(L, **kw) == EINVAL and b"leading dimension too small" in err(), kw
    assert _norm(L, ldr=0, ldh=0, r=None, h=None, rows=0) == OK  # without the operands their strides are not read
    assert _norm(L, eps=-1e-9) == EINVAL and b"negative eps" in err()
    assert _norm(L, rows=0, x=None, w=None, y=None, r=None, h=None) == OK
    for name in ("x", "w", "y"):
        assert _norm(L, **{name: None}) == EINVAL and b"pli_rmsnorm: null pointer" in err(), name
    for dt in (3, -1):
        assert _norm(L, dtype=dt) == EINVAL and b"pli_rmsnorm: bad dtype" in err(), dt
    assert L.pli_last_route() == b""


def test_attn_decode_dev_argument_rules_without_gpu(L):
    err = L.pli_last_error
    for kw in (dict(B=-1), dict(H=0), dict(Hkv=0), dict(nq=-1), dict(nmax=-1), dict(D=0), dict(H=8, Hkv=3)):
        assert _attn(L, **kw) == EINVAL and b"pli_attn_decode_dev: bad shape" in err(), kw
    for s in (float("nan"), float("inf")):
        assert _attn(L, scale=s) == EINVAL and b"non-finite scale" in err()
    assert _attn(L, B=0, q=None, k=None, v=None, o=None, ndev=None) == OK
    assert _attn(L, nq=0, q=None, k=None, v=None, o=None, ndev=None) == OK
    for name in ("q", "k", "v", "o", "ndev"):
        assert _attn(L, **{name: None}) == EINVAL and b"pli_attn_decode_dev: null pointer" in err(), name
    # off the fast path: fp32, head_dim 80, more than 16 rows per kv head, a stride % 8, an empty plan, alignment
    st = [1024] * 12
    st[5] = 1028
    for kw in (dict(dtype=F32), dict(D=80), dict(H=32, Hkv=1, nq=1), dict(nq=5), dict(strides=st), dict(nmax=0),
               dict(q=ODD), dict(k=ODD), dict(v=ODD), dict(o=ODD)):
        assert _attn(L, **kw) == EUNSUPPORTED and b"needs bf16/fp16, head_dim 64/128" in err(), kw
    # a short workspace: one (batch, kv head) pair over 4096 keys is split, the partials need room
    need = L.pli_attn_decode_workspace_size(1, 8, 1, 1, 4096, 128)
    assert need > 0
    big = dict(H=8, Hkv=1, nmax=4096)
    assert _attn(L, ws=P, ws_bytes=need - 1, **big) == EINVAL and b"workspace of" in err()
    assert _attn(L, ws=None, ws_bytes=need, **big) == EINVAL and b"workspace of" in err()
    assert L.pli_last_route() == b""


def test_wrappers_refuse_cpu_tensors_bad_pos_and_mismatched_caches(built_lib):
    import pli_hip
    bf = torch.bfloat16
    x, g = torch.zeros(2, 64, dtype=bf), torch.ones(64, dtype=bf)
    w = torch.zeros(16, 64, dtype=bf)
    kc = torch.zeros(2, 8, 2, 8, dtype=bf)
    q = torch.zeros(2, 1, 16, dtype=bf)
    pos = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.rmsnorm(x, g)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.rms_linear(x, g, 1e-6, w)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.rms_swiglu(x, g, 1e-6, w, w)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.kv_append(kc[:, :1], kc[:, :1], kc, kc, pos)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.attn_decode_dev(torch.zeros(2, 1, 4, 8, dtype=bf), kc, kc, pos)
    with pytest.raises(pli_hip.PliError, match="CPU tensor"):
        pli_hip.qkv_into_cache(x.view(2, 1, 64), w, w, w, q, kc, kc, pos)
    # pos: an int32 device tensor (a CPU one is refused before anything else in the fused form)
    for bad in (pos, pos.long()):
        with pytest.raises(pli_hip.PliError, match="pos must be an int32 device tensor"):
            pli_hip.rms_qkv_into_cache(x.view(2, 1, 64), g, 1e-6, w, w, w, q, kc, kc, bad)


@pytest.mark.gpu
def test_wrappers_refuse_bad_pos_and_mismatched_caches_on_the_device(built_lib):
    import pli_hip
    bf, dev = torch.bfloat16, "cuda:0"
    x, g = torch.zeros(2, 1, 64, dtype=bf, device=dev), torch.ones(64, dtype=bf, device=dev)
    w = torch.zeros(16, 64, dtype=bf, device=dev)
    kc = torch.zeros(2, 8, 2, 8, dtype=bf, device=dev)
    q = torch.zeros(2, 1, 16, dtype=bf, device=dev)
    pos = torch.zeros(1, dtype=torch.int32, device=dev)
    for bad in (pos.long(), pos.cpu()):
        with pytest.raises(pli_hip.PliError, match="pos must be an int32 device tensor"):
            pli_hip.qkv_into_cache(x, w, w, w, q, kc, kc, bad)
        with pytest.raises(pli_hip.PliError, match="pos must be an int32 device tensor"):
            pli_hip.rms_qkv_into_cache(x, g, 1e-6, w, w, w, q, kc, kc, bad)
        with pytest.raises(pli_hip.PliError, match="pos must be an int32 device tensor"):
            pli_hip.kv_append(kc[:, :1], kc[:, :1], kc, kc, bad)
    with pytest.raises(pli_hip.PliError, match="shape mismatch"):
        pli_hip.qkv_into_cache(x, w, w, w, q, kc, kc[:, :4], pos)
    with pytest.raises(pli_hip.PliError, match="must be \\[B, S_max, Hkv, D\\]"):
        pli_hip.qkv_into_cache(x, w, w, w, q, kc[:1], kc[:1], pos)
    with pytest.raises(pli_hip.PliError, match="do not match the cache"):
        pli_hip.qkv_into_cache(x, w, w[:8], w, q, kc, kc, pos)
    with pytest.raises(pli_hip.PliError, match="caches must be \\[B, S_max, Hkv, D\\]"):
        pli_hip.rms_qkv_into_cache(x, g, 1e-6, w, w, w, q, kc[:1], kc[:1], pos)
    with pytest.raises(pli_hip.PliError, match="q_out must be"):
        pli_hip.rms_qkv_into_cache(x, g, 1e-6, w, w, w, q[:, :, ::2], kc, kc, pos)
    with pytest.raises(pli_hip.PliError, match="kv_append shape mismatch"):
        pli_hip.kv_append(kc[:, :1], kc[:, :1], kc, kc[:, :, :1], pos)
    with pytest.raises(pli_hip.PliError, match="kv_append shape mismatch"):
        pli_hip.kv_append(kc[:, :1], kc[:1, :1], kc, kc, pos)
