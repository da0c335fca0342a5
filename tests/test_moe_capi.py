"""The argument rules of the MoE entry points of include/pli.h without a GPU:
each PLI_REQUIRE of pli_moe_route, pli_moe_combine and pli_gemm_grouped
returns its status with its message before any HIP call (the data pointers are
never dereferenced, nothing is launched), and pli.h, the comment above
grouped_dispatch and pli_hip.gemm_grouped state one rows_bound contract.  The
empty cases that return PLI_OK are in tests/test_capi.py."""
from __future__ import annotations

import os
import re

import pytest

from conftest import PKG, ROOT

EINVAL = 1000
F32, F16, BF16 = 0, 1, 2
P = 4096        # never dereferenced: validation fails first
ODD = 4104      # 8 bytes past a 16-byte boundary


@pytest.fixture()
def L(built_lib):
    import pli_hip
    return pli_hip.lib()


def _route(L, **kw):
    a = dict(logits=P, ld=8, tokens=4, experts=8, top_k=2, normalize=1, dtype=F32, weights=P, idx=P, pos=P, gather=P,
             offsets=P, ws=P)
    a.update(kw)
    return L.pli_moe_route(a["logits"], a["ld"], a["tokens"], a["experts"], a["top_k"], a["normalize"], a["dtype"],
                           a["weights"], a["idx"], a["pos"], a["gather"], a["offsets"], a["ws"], None)


def _combine(L, **kw):
    a = dict(y=P, ldy=64, pos=P, w=P, out=P, ldo=64, tokens=4, top_k=2, hidden=64, dtype=BF16)
    a.update(kw)
    return L.pli_moe_combine(a["y"], a["ldy"], a["pos"], a["w"], a["out"], a["ldo"], a["tokens"], a["top_k"],
                             a["hidden"], a["dtype"], None)


def _grouped(L, variant=None, **kw):
    a = dict(x=P, gather=P, w=P, wu=None, c=P, offsets=P, experts=4, rows=8, n=64, k=128, ldx=128, ldw=128, ldc=64,
             dtype=BF16)
    a.update(kw)
    args = (a["x"], a["gather"], a["w"], a["wu"], a["c"], a["offsets"], a["experts"], a["rows"], a["n"], a["k"],
            a["ldx"], a["ldw"], a["ldc"], a["dtype"], None)
    return L.pli_gemm_grouped(*args) if variant is None else L.pli_gemm_grouped_variant(*args, variant)


def test_symbols_declared_and_exported(L):
    header = open(os.path.join(ROOT, "include", "pli.h")).read()
    for name in ("pli_moe_route", "pli_moe_combine", "pli_gemm_grouped", "pli_gemm_grouped_variant"):
        assert re.search(r"\bint\s+" + name + r"\(", header), name
        assert getattr(L, name) is not None


def test_moe_route_argument_rules_without_gpu(L):
    err = L.pli_last_error
    for kw in (dict(experts=0), dict(experts=65, ld=65), dict(experts=-1), dict(top_k=0), dict(top_k=9, experts=16, ld=16),
               dict(top_k=3, experts=2), dict(top_k=8, experts=7), dict(ld=7), dict(ld=0), dict(tokens=-1)):
        assert _route(L, **kw) == EINVAL and b"pli_moe_route: bad shape" in err(), kw
    assert b"tokens=-1 experts=8 (<= 64) top_k=2 (<= 8)" in err()
    for dt in (3, 7, -1):
        assert _route(L, dtype=dt) == EINVAL and b"pli_moe_route: bad dtype" in err(), dt
    # offsets and workspace are always needed (tokens = 0 still writes the offsets)
    for name in ("offsets", "ws"):
        for tokens in (4, 0):
            assert _route(L, tokens=tokens, **{name: None}) == EINVAL and b"pli_moe_route: null pointer" in err(), name
    for name in ("logits", "weights", "idx", "pos", "gather"):
        assert _route(L, **{name: None}) == EINVAL and b"pli_moe_route: null pointer" in err(), name
    # (with tokens = 0 the per-token operands may be NULL: the next rule answers)
    assert _route(L, tokens=0, logits=None, weights=None, idx=None, pos=None, gather=None, experts=0) == EINVAL
    assert b"bad shape" in err()
    assert L.pli_last_route() == b""  # nothing was launched


def test_moe_combine_argument_rules_without_gpu(L):
    err = L.pli_last_error
    shape = (dict(hidden=60), dict(hidden=4), dict(hidden=0), dict(hidden=-8), dict(top_k=0), dict(tokens=-1),
             dict(ldy=68), dict(ldo=68), dict(ldy=56), dict(ldo=56), dict(hidden=72), dict(y=ODD), dict(out=ODD))
    for kw in shape:
        assert _combine(L, **kw) == EINVAL and b"pli_moe_combine: bad shape / alignment" in err(), kw
    assert b"hidden % 8 == 0, 16-byte rows" in err()
    for dt in (F32, 5, -1):
        assert _combine(L, dtype=dt) == EINVAL and b"pli_moe_combine: bf16/fp16 only" in err(), dt
    assert _combine(L, dtype=F32, tokens=0) == EINVAL  # the type rule comes before the empty return
    for name in ("y", "pos", "w", "out"):
        assert _combine(L, **{name: None}) == EINVAL and b"pli_moe_combine: null pointer" in err(), name
    assert L.pli_last_route() == b""


@pytest.mark.parametrize("variant", [None, 1, 2])
def test_gemm_grouped_argument_rules_without_gpu(L, variant):
    err = L.pli_last_error
    g = lambda **kw: _grouped(L, variant, **kw)  # noqa: E731
    for kw in (dict(experts=0), dict(experts=-1), dict(rows=-1), dict(n=0), dict(n=-16), dict(k=0), dict(k=-128)):
        assert g(**kw) == EINVAL and b"pli_gemm_grouped: bad shape E=" in err(), kw
    for name in ("x", "w", "c", "offsets"):
        assert g(**{name: None}) == EINVAL and b"pli_gemm_grouped: null pointer" in err(), name
    for dt in (F32, 4, -1):
        assert g(dtype=dt) == EINVAL and b"pli_gemm_grouped: bf16/fp16 only" in err(), dt
    align = (dict(k=64, ldx=64, ldw=64), dict(k=192, ldx=192, ldw=192), dict(k=8, ldx=8, ldw=8), dict(n=8), dict(n=72, ldc=72),
             dict(ldx=132), dict(ldw=132), dict(ldc=68), dict(x=ODD), dict(c=ODD))
    for kw in align:
        assert g(**kw) == EINVAL and b"needs k % 128 == 0, n % 16 == 0, 16-byte aligned rows" in err(), kw
    for kw in (dict(ldx=120), dict(ldw=120), dict(ldc=56), dict(ldx=0), dict(ldw=0), dict(ldc=0)):
        assert g(**kw) == EINVAL and b"pli_gemm_grouped: leading dimension too small" in err(), kw
    assert L.pli_last_route() == b""


def test_gemm_grouped_grid_guards_without_gpu(L):
    """the two "grid too large" rules, each on the route that owns it: the 256-row tile (slots x column tiles, here
    (2^23 + 2) x 256) and the weight-streaming kernel (experts x n / 16 = 2^20 x 2^11; 16 rows keep it off the LDS
    route)"""
    err = L.pli_last_error
    big = (1 << 31) - 1
    for variant in (None, 1):
        assert _grouped(L, variant, experts=2, rows=big, n=65536, ldc=65536) == EINVAL
        assert b"pli_gemm_grouped: grid too large" in err()
        assert _grouped(L, variant, experts=1 << 20, rows=16, n=32768, ldc=32768) == EINVAL
        assert b"pli_gemm_grouped: grid too large" in err()
    assert _grouped(L, 2, experts=1 << 20, rows=big, n=32768, ldc=32768) == EINVAL   # variant 2 past 1024 rows
    assert b"pli_gemm_grouped: grid too large" in err()
    assert L.pli_last_route() == b""


def test_gemm_grouped_lds_route_refuses_more_experts_than_grid_z_without_gpu(L):
    """the LDS-staged kernel indexes experts in blockIdx.z (<= 65535): forcing it (variant 2) with more experts is
    an argument error wherever it would have run; 65535 experts and the shapes it never took pass this rule (the
    replay of tests/moe_cases.py says the same); pli.h and the comment above grouped_dispatch state the limit"""
    import moe_cases as mc
    err = L.pli_last_error
    for kw in (dict(rows=8, n=128, ldc=128), dict(rows=20, n=128, ldc=128), dict(rows=1024, n=256, ldc=256),
               dict(rows=20, n=64, wu=P), dict(rows=1024, n=128, wu=P, ldc=128)):
        for E in (65536, 1 << 20):
            assert _grouped(L, 2, experts=E, **kw) == EINVAL, (kw, E)
            assert b"pli_gemm_grouped: the LDS-staged route takes at most 65535 experts (E=%d)" % E in err()
            with pytest.raises(ValueError):
                mc.grouped_route(E, kw["rows"], kw["n"], "wu" in kw, 2)
    # (where the route does not apply, variant 2 falls through as before: here onto the next rule)
    assert _grouped(L, 2, experts=1 << 20, rows=2048, n=32768, ldc=32768) == EINVAL and b"grid too large" in err()
    assert mc.grouped_route(1 << 20, 2048, 32768, False, 2) == "gemm_grouped_nt<NBG8,SW0>"
    # the default leaves the LDS route at 65536 experts, for the weight-streaming kernel
    assert mc.grouped_route(65535, 20, 128, False, None) == "gemm_grouped_lds_nt<MC1,SW0>"
    assert mc.grouped_route(65536, 20, 128, False, None) == "gemm_grouped_nt<NBG2,SW0>"
    assert mc.grouped_route(65536, 20, 128, True, None) == "gemm_grouped_nt<NBG2,SW1>"
    assert L.pli_last_route() == b""
    header = " ".join(open(os.path.join(ROOT, "include", "pli.h")).read().split())
    src = open(os.path.join(PKG, "csrc", "gemm.hip")).read()
    com = " ".join(src[src.index("// Grouped NT GEMM over experts"):src.index("static int grouped_dispatch(")].split())
    assert "blockIdx.z" in com and "65535" in com and "chosen only for experts <= 65535" in header


def test_rows_bound_contract_reads_the_same_everywhere():
    """rows_bound >= offsets[experts], the number of sorted rows (which also bounds every expert): pli.h, the comment
    above grouped_dispatch and pli_hip.gemm_grouped.  gemm_256g's grid is cdiv(rows_bound, 256) + experts slots,
    which covers sum_e cdiv(count_e, 256) only under that reading; (1100, 1100) at 2200 is the GPU case."""
    import pli_hip
    flat = lambda s: " ".join(re.sub(r"\n\s*(\*|//)", " ", s).split())  # noqa: E731
    header = open(os.path.join(ROOT, "include", "pli.h")).read()
    doc = flat(header[header.index("pli_gemm_grouped: for every expert"):header.index("pli_moe_combine: out[t]")])
    src = open(os.path.join(PKG, "csrc", "gemm.hip")).read()
    com = flat(src[src.index("// Grouped NT GEMM over experts"):src.index("static int grouped_dispatch(")])
    for text in (doc, com, " ".join(pli_hip.gemm_grouped.__doc__.split())):
        assert "rows_bound >= offsets[experts], the number of sorted rows" in text
        assert "every expert's row count" not in text
    # 10 real slots: 7 under the per-expert reading of the (1100, 1100) case, 11 under the documented one
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    assert 2 * cdiv(1100, 256) == 10 and cdiv(1100, 256) + 2 == 7 and cdiv(2200, 256) + 2 == 11
