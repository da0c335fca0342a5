"""The argument rules of pli_gemm / _variant / _ws / _ws_variant, pli_gemm_f32out
and pli_gemv / _variant without a GPU: each PLI_REQUIRE of gemm_dispatch,
pli_gemm_f32out, pli_gemv_variant and of the launchers reachable through them
(launch_mfma, launch_256, launch_gemm_w5, launch_gemm_w4v, gemv's launch)
returns its status with its message before any HIP call -- the data pointers are
never dereferenced and nothing is launched.

Rules with no failing input through these entry points:

* launch_gemm_w5 "fp32 output is NT without bias": pli_gemm_f32out, the only
  caller with f32out, passes trans_b = 1 and a null bias;
* launch_gemm_w5 / launch_gemm_w4v "shape ... not supported": the dispatch and
  pli_gemm_f32out test gemm_w5_ok / gemm_w4v_ok first and take another route
  when they fail (the replay's w5_ok / w4v_ok);
* launch_gemm_w5 "group_m must be >= 1": every caller passes 4;
* launch_gemm_w5 "persistent: M, N must be multiples of 256": the dispatch and
  pli_gemm_f32out ask for the walk only under that condition.

launch_skinny, launch_smallm, launch_midm, launch_splitk, launch_generic and
launch_gemm_f32_mfma have no rule of their own."""
from __future__ import annotations

import pytest

import gemm_cases as gc

EINVAL = 1000
F32, F16, BF16 = 0, 1, 2
P = 4096        # never dereferenced: validation fails first
ODD = 4104      # 8 bytes past a 16-byte boundary
BIG = (1 << 31) - 1
ENTRIES = ("gemm", "variant", "ws", "ws_variant")


@pytest.fixture()
def L(built_lib):
    import pli_hip
    return pli_hip.lib()


def _gemm(L, entry="gemm", variant=0, ws=None, ws_bytes=0, **kw):
    a = dict(a=P, b=P, c=P, bias=None, m=32, n=64, k=128, tb=1, dtype=BF16)
    a.update(kw)
    a.setdefault("lda", a["k"])
    a.setdefault("ldb", a["k"] if a["tb"] else a["n"])
    a.setdefault("ldc", a["n"])
    head = (a["a"], a["b"], a["c"], a["bias"], a["m"], a["n"], a["k"], a["lda"], a["ldb"], a["ldc"], a["tb"], a["dtype"])
    if entry == "gemm":
        return L.pli_gemm(*head, None)
    if entry == "variant":
        return L.pli_gemm_variant(*head, None, variant)
    if entry == "ws":
        return L.pli_gemm_ws(*head, ws, ws_bytes, None)
    return L.pli_gemm_ws_variant(*head, ws, ws_bytes, None, variant)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("tb", [1, 0])
def test_gemm_argument_rules_without_gpu(L, entry, tb):
    err = L.pli_last_error
    g = lambda **kw: _gemm(L, entry, tb=tb, **kw)  # noqa: E731
    for kw in (dict(m=-1), dict(n=-8), dict(k=-128), dict(m=-1, n=0)):
        assert g(**kw) == EINVAL and b"pli_gemm: bad shape m=" in err(), kw
    assert b"m=-1 n=0 k=128" in err()
    for name in ("a", "b", "c"):
        assert g(**{name: None}) == EINVAL and b"pli_gemm: null pointer" in err(), name
    assert g(k=0, a=None, b=None, c=None) == EINVAL and b"null pointer" in err()          # c is always needed
    for kw in (dict(lda=120), dict(ldc=63), dict(ldc=-64), dict(ldb=(127 if tb else 63)), dict(ldb=0)):
        assert g(**kw) == EINVAL and b"pli_gemm: leading dimension too small (lda=" in err(), kw
    assert g(lda=136, ldb=(120 if tb else 56), ldc=72) == EINVAL
    assert (b"lda=136 ldb=120 ldc=72" if tb else b"lda=136 ldb=56 ldc=72") in err()
    # ldb is measured against k (NT) or n (NN): 64 is enough for NN (n = 64), not for NT (k = 128)
    assert (g(ldb=64, dtype=7) == EINVAL) and (b"leading dimension" in err()) == bool(tb)
    # the type is looked at last: after the shape, the pointers and the leading dimensions, with K == 0 too
    for dt in (3, 7, -1):
        assert g(dtype=dt) == EINVAL and b"pli_gemm: bad dtype" in err(), dt
        assert g(dtype=dt, k=0, a=None, b=None, lda=0, ldb=(0 if tb else 64)) == EINVAL and b"pli_gemm: bad dtype" in err(), dt
    assert g(dtype=7, c=None) == EINVAL and b"null pointer" in err()
    assert L.pli_last_route() == b""  # nothing was launched


@pytest.mark.parametrize("entry", ENTRIES)
def test_gemm_empty_calls_return_ok_without_gpu(L, entry):
    """m == 0 or n == 0: OK after the shape rule and before the pointer, leading-dimension and type rules"""
    for kw in (dict(m=0), dict(n=0, ldc=0), dict(m=0, n=0), dict(m=0, a=None, c=None), dict(n=0, b=None, c=None, bias=None),
               dict(m=0, lda=0, ldb=0, ldc=0), dict(m=0, dtype=F32), dict(m=0, dtype=9), dict(m=0, k=0), dict(n=0, tb=0, ldb=0)):
        assert _gemm(L, entry, **kw) == 0, kw
        assert L.pli_last_error() == b"" and L.pli_last_route() == b""
    assert _gemm(L, entry, m=0, k=-1) == EINVAL                                # (the shape rule comes first)
    if "ws" in entry:
        assert _gemm(L, entry, ws=ODD, ws_bytes=1 << 20, m=0) == 0             # (nor is the workspace looked at)


def test_gemm_misaligned_workspace_is_refused_where_the_split_would_run(L):
    err = L.pli_last_error
    m, n, k = 64, 64, 4096
    need = L.pli_gemm_workspace_size(m, n, k, 1, BF16)
    assert need == gc.workspace_size(m, n, k, True, "bf16") == 16 * m * n * 4
    for entry, variant in (("ws", 0), ("ws_variant", 0), ("ws_variant", 22), ("ws_variant", 24), ("ws_variant", 25),
                           ("ws_variant", 28)):
        for dt in (BF16, F16):
            assert gc.gemm_route(m, n, k, "bf16", True, False, variant, need).kernel.startswith("gemm_splitk")
            assert _gemm(L, entry, variant, ws=ODD, ws_bytes=need, m=m, n=n, k=k, dtype=dt) == EINVAL
            assert b"pli_gemm_ws: workspace must be 16-byte aligned" in err()
            assert _gemm(L, entry, variant, ws=P + 4, ws_bytes=need + 64, m=m, n=n, k=k, dtype=dt) == EINVAL
    # one slice (K = 128 at 32 < M: not short K by N / 128 < 64) takes a workspace of any size: aligned all the same
    assert gc.gemm_route(64, 64, 128, "bf16", True, False, 25, 1).inst == "MC2,ks1,lds,NB2,direct-store"
    assert _gemm(L, "ws_variant", 25, ws=ODD, ws_bytes=1, m=64, n=64, k=128) == EINVAL and b"16-byte aligned" in err()
    assert L.pli_last_route() == b""


def test_gemm_grid_guards_without_gpu(L):
    """"grid too large" on each tile that owns one: gemm_mfma (k % 64 != 0 keeps the call off the others), gemm_256
    and gemm_256p (variants 2 / 3), gemm_w5 (41, 43 and the default) and gemm_w4v (40)"""
    err = L.pli_last_error
    n = (1 << 31) - 8
    for tb in (1, 0):
        for v in (0, 1, 2, 41):
            assert _gemm(L, "variant", v, m=BIG, n=n, k=8, tb=tb) == EINVAL and b"pli_gemm: grid too large" in err(), (tb, v)
            assert gc.gemm_route(BIG, n, 8, "bf16", tb, False, v, 0).kernel == gc.MFMA
        for v in (2, 3, 13):
            assert _gemm(L, "variant", v, m=BIG, n=n, k=64, tb=tb) == EINVAL and b"pli_gemm: grid too large" in err(), (tb, v)
            assert gc.gemm_route(BIG, n, 64, "bf16", tb, False, v, 0).kernel == gc.G256
        assert _gemm(L, "variant", 1, m=BIG, n=n, k=64, tb=tb) == EINVAL and b"pli_gemm: grid too large" in err()
        # (NN: ldb = n stays inside gemm_w5's 32-bit DMA offsets, n * 128 bytes < 2^31; past it the call is gemm_256's)
        nw = (1 << 24) - 256
        for v in (0, 41):
            assert _gemm(L, "variant", v, m=BIG, n=nw, k=64, tb=tb) == EINVAL and b"gemm_w5: grid too large" in err(), (tb, v)
        assert _gemm(L, "variant", 43, m=(1 << 31) - 256, n=nw, k=128, tb=tb) == EINVAL and b"gemm_w5: grid too large" in err()
        assert _gemm(L, "variant", 40, m=BIG, n=nw, k=32, tb=tb) == EINVAL and b"gemm_w4v: grid too large" in err()
        assert _gemm(L, "gemm", m=BIG, n=nw, k=64, tb=tb) == EINVAL and b"gemm_w5: grid too large" in err()     # the default
    # gemm_w5's leading-dimension limit (lda * 512 bytes < 2^31) fails: the default is the 256 x 256 tile again
    assert _gemm(L, "gemm", m=BIG, n=n, k=64, lda=1 << 22) == EINVAL and b"pli_gemm: grid too large" in err()
    assert gc.gemm_route(BIG, n, 64, "bf16", True, False, None, 0, lds=(1 << 22, 64, n)).kernel == gc.G256
    assert _gemm(L, "variant", 41, m=BIG, n=n, k=64, tb=0) == EINVAL and b"pli_gemm: grid too large" in err()
    assert gc.gemm_route(BIG, n, 64, "bf16", False, False, 41, 0).kernel == gc.G256
    assert L.pli_last_route() == b""


def _f32out(L, **kw):
    a = dict(a=P, b=P, c=P, m=32, n=64, k=128, dtype=BF16)
    a.update(kw)
    a.setdefault("lda", a["k"])
    a.setdefault("ldb", a["k"])
    return L.pli_gemm_f32out(a["a"], a["b"], a["c"], a["m"], a["n"], a["k"], a["lda"], a["ldb"], a["dtype"], None)


def test_gemm_f32out_argument_rules_without_gpu(L):
    err = L.pli_last_error
    for kw in (dict(m=-1), dict(n=-8), dict(k=-128), dict(lda=127), dict(ldb=0), dict(m=0, lda=120)):
        assert _f32out(L, **kw) == EINVAL and b"pli_gemm_f32out: bad shape m=" in err(), kw
    assert _f32out(L, lda=136, ldb=120) == EINVAL and b"m=32 n=64 k=128 lda=136 ldb=120" in err()
    for dt in (F32, 3, -1):
        assert _f32out(L, dtype=dt) == EINVAL and b"pli_gemm_f32out: bf16 / fp16 inputs only" in err(), dt
    assert _f32out(L, dtype=F32, m=0) == EINVAL                     # the type rule comes before the empty return
    for kw in (dict(m=0), dict(n=0), dict(m=0, a=None, b=None, c=None), dict(n=0, c=None), dict(m=0, k=0, dtype=F16)):
        assert _f32out(L, **kw) == 0 and err() == b"", kw
    for name in ("a", "b", "c"):
        assert _f32out(L, **{name: None}) == EINVAL and b"pli_gemm_f32out: null pointer" in err(), name
    assert _f32out(L, k=0, a=None, b=None, c=None) == EINVAL and b"null pointer" in err()
    # the one-thread-per-output kernel's grid, and gemm_w5's through the large-shape route
    assert gc.f32out_route(BIG, BIG, 8, "bf16").kernel == gc.F32OUT_GENERIC
    assert _f32out(L, m=BIG, n=BIG, k=8) == EINVAL and b"pli_gemm_f32out: grid too large" in err()
    n32 = (1 << 31) - 32
    assert gc.f32out_route(BIG, n32, 64, "bf16").kernel == gc.W5
    assert _f32out(L, m=BIG, n=n32, k=64) == EINVAL and b"gemm_w5: grid too large" in err()
    assert L.pli_last_route() == b""


def _gemv(L, variant=None, **kw):
    a = dict(w=P, x=P, y=P, m=32, k=128, dtype=BF16)
    a.update(kw)
    a.setdefault("ldw", a["k"])
    head = (a["w"], a["x"], a["y"], a["m"], a["k"], a["ldw"], a["dtype"], None)
    return L.pli_gemv(*head) if variant is None else L.pli_gemv_variant(*head, variant)


@pytest.mark.parametrize("variant", [None, -1, 0, 8, 16])
def test_gemv_argument_rules_without_gpu(L, variant):
    err = L.pli_last_error
    g = lambda **kw: _gemv(L, variant, **kw)  # noqa: E731
    for kw in (dict(m=-1), dict(k=-8), dict(ldw=127), dict(ldw=0), dict(m=0, ldw=8)):
        assert g(**kw) == EINVAL and b"pli_gemv: bad shape m=" in err(), kw
    assert g(m=3, k=16, ldw=8) == EINVAL and b"m=3 k=16 ldw=8" in err()
    for dt in (3, 7, -1):
        assert g(dtype=dt) == EINVAL and b"pli_gemv: bad dtype" in err(), dt
    assert g(dtype=3, m=0) == EINVAL                                # the type rule comes before the empty return
    for kw in (dict(m=0), dict(m=0, w=None, x=None, y=None), dict(m=0, k=0), dict(m=0, dtype=F32)):
        assert g(**kw) == 0 and err() == b"", kw
    for name in ("w", "x", "y"):
        assert g(**{name: None}) == EINVAL and b"pli_gemv: null pointer" in err(), name
    assert g(k=0, w=None, x=None, y=None) == EINVAL and b"null pointer" in err()           # y is always needed
    assert L.pli_last_route() == b""


def test_gemv_unknown_variant_without_gpu(L):
    """an unknown variant is refused in the vector class (before the launch); any negative one is the default rule"""
    err = L.pli_last_error
    for v in (17, 18, 99):
        for dt in (F32, F16, BF16):
            assert _gemv(L, v, dtype=dt) == EINVAL and b"pli_gemv: unknown variant" in err(), (v, dt)
    assert sorted(gc.GEMV_VARIANTS) == list(range(17))
    assert L.pli_last_route() == b""
