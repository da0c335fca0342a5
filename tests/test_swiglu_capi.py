"""The argument rules of pli_gemm_swiglu / _ws / _ws_variant without a GPU:
each PLI_REQUIRE of swiglu_dispatch, launch_swiglu and launch_gemm_w5_swiglu
returns its status with its message before any HIP call (the data pointers are
never dereferenced, nothing is launched), and pli_gemm_swiglu_workspace_size is
2 * ks * m * n * 4 with ks from the replay of tests/swiglu_cases.py.

launch_gemm_w5_swiglu's shape rule (k % 64, n % 8, the 32-bit DMA offsets) has
no failing input through these entry points: launch_swiglu sends a call there
only under the same conditions, and a call that misses them takes the phased
tile or the 128 x 64 tile instead (the replay's `w5_ld`); its grid rule is
reached with variant 3."""
from __future__ import annotations

import ctypes

import pytest

import swiglu_cases as sc

EINVAL = 1000
F32, F16, BF16 = 0, 1, 2
P = 4096        # never dereferenced: validation fails first
ODD = 4104      # 8 bytes past a 16-byte boundary
BIG = (1 << 31) - 1


@pytest.fixture()
def L(built_lib):
    import pli_hip
    return pli_hip.lib()


def _swiglu(L, variant=None, ws=None, ws_bytes=0, **kw):
    a = dict(x=P, wg=P, wu=P, h=P, m=32, n=64, k=128, dtype=BF16)
    a.update(kw)
    for name, dim in (("ldx", "k"), ("ldwg", "k"), ("ldwu", "k"), ("ldh", "n")):
        a.setdefault(name, a[dim])
    head = (a["x"], a["wg"], a["wu"], a["h"], a["m"], a["n"], a["k"], a["ldx"], a["ldwg"], a["ldwu"], a["ldh"],
            a["dtype"])
    if variant is not None:
        return L.pli_gemm_swiglu_ws_variant(*head, ws, ws_bytes, None, variant)
    if ws is not None or ws_bytes:
        return L.pli_gemm_swiglu_ws(*head, ws, ws_bytes, None)
    return L.pli_gemm_swiglu(*head, None)


@pytest.mark.parametrize("variant", [None, 0, 1, 2, 3, 4])
def test_swiglu_argument_rules_without_gpu(L, variant):
    err = L.pli_last_error
    g = lambda **kw: _swiglu(L, variant, **kw)  # noqa: E731
    for kw in (dict(m=-1), dict(n=-8), dict(k=-128), dict(m=-1, n=0)):
        assert g(**kw) == EINVAL and b"pli_gemm_swiglu: bad shape m=" in err(), kw
    assert b"m=-1 n=0 k=128" in err()
    for dt in (3, 7, -1):
        assert g(dtype=dt) == EINVAL and b"pli_gemm_swiglu: bad dtype" in err(), dt
    assert g(dtype=3, m=0) == EINVAL                     # the type rule comes before the empty return
    for name in ("x", "wg", "wu", "h"):
        assert g(**{name: None}) == EINVAL and b"pli_gemm_swiglu: null pointer" in err(), name
    assert g(k=0, x=None, wg=None, wu=None, h=None) == EINVAL and b"null pointer" in err()   # h is always needed
    for kw in (dict(ldx=120), dict(ldwg=127), dict(ldwu=0), dict(ldh=63), dict(ldh=-64), dict(ldwu=120, ldwg=136)):
        assert g(**kw) == EINVAL and b"pli_gemm_swiglu: leading dimension too small (ldx=" in err(), kw
    assert b"ldx=128 ldwg=136 ldwu=120 ldh=64" in err()
    assert L.pli_last_route() == b""  # nothing was launched


@pytest.mark.parametrize("variant", [None, 0, 1, 2, 3, 4])
def test_swiglu_empty_calls_return_ok_without_gpu(L, variant):
    """m == 0 or n == 0: OK before the pointer rule (empty operands may be NULL) and before the leading dimensions"""
    for kw in (dict(m=0), dict(n=0, ldh=0), dict(m=0, n=0, ldh=0), dict(m=0, x=None, h=None),
               dict(n=0, ldh=0, wg=None, wu=None, h=None), dict(m=0, ldx=0, ldwg=0, ldwu=0, ldh=0),
               dict(m=0, dtype=F32), dict(m=0, k=0)):
        assert _swiglu(L, variant, **kw) == 0, kw
        assert L.pli_last_error() == b"" and L.pli_last_route() == b""
    assert _swiglu(L, variant, ws=ODD, ws_bytes=1 << 20, m=0) == 0    # (nor is the workspace looked at)


def test_swiglu_misaligned_workspace_is_refused_where_the_split_would_run(L):
    err = L.pli_last_error
    need = L.pli_gemm_swiglu_workspace_size(32, 64, 128, BF16)
    assert need == 2 * 1 * 32 * 64 * 4
    for variant in (None, 0, 1):
        for dt in (BF16, F16):
            assert _swiglu(L, variant, ws=ODD, ws_bytes=need, dtype=dt) == EINVAL
            assert b"pli_gemm_swiglu_ws: workspace must be 16-byte aligned" in err()
            assert _swiglu(L, variant, ws=P + 4, ws_bytes=need + 64, dtype=dt) == EINVAL
    assert L.pli_last_route() == b""


def test_swiglu_grid_guards_without_gpu(L):
    """"grid too large" on each tile that owns one: gemm_w5 (variant 3), the phased tile (variant 4) and the
    128 x 64 tile (k % 64 != 0 keeps the call off the other two)"""
    err = L.pli_last_error
    n = (1 << 31) - 8
    assert _swiglu(L, 3, m=BIG, n=n, k=64) == EINVAL and b"gemm_w5 swiglu: grid too large" in err()
    assert _swiglu(L, 4, m=BIG, n=n, k=64) == EINVAL and b"pli_gemm_swiglu: grid too large" in err()
    for variant in (None, 2, 3, 4):
        assert _swiglu(L, variant, m=BIG, n=n, k=8) == EINVAL and b"pli_gemm_swiglu: grid too large" in err()
    assert _swiglu(L, None, m=BIG, n=n, k=64) == EINVAL and b"gemm_w5 swiglu: grid too large" in err()   # the default
    # gemm_w5's leading-dimension limit (ldx * 512 bytes < 2^31) fails: the default is the phased tile again
    assert _swiglu(L, None, m=BIG, n=n, k=64, ldx=1 << 22) == EINVAL and b"pli_gemm_swiglu: grid too large" in err()
    assert sc.swiglu_route(BIG, n, 64, "bf16", None, 0, lds=(1 << 22, 64, 64)).kernel == sc.P256
    assert sc.swiglu_route(BIG, n, 64, "bf16", None, 0).kernel == sc.W5
    assert L.pli_last_route() == b""


def _size(L, m, n, k, dt):
    return L.pli_gemm_swiglu_workspace_size(m, n, k, sc.DTYPE_CODE[dt])


def test_workspace_size_is_two_ks_planes_for_every_case(L):
    for c in sc.SWIGLU_CASES:
        for dt in c.dts:
            ks = sc.swiglu_slices(c.m, c.n, c.k, True) if dt != "fp32" else 0
            assert _size(L, c.m, c.n, c.k, dt) == 2 * ks * c.m * c.n * 4 == sc.workspace_size(c.m, c.n, c.k, dt), c
            if c.route == sc.SPLIT:
                assert ks == sc.split_ks(c) > 0   # (the default and the forced slices agree on every split case)


def test_workspace_size_at_the_boundaries(L):
    ks_of = lambda m, n, k: _size(L, m, n, k, "bf16") // (2 * m * n * 4)  # noqa: E731
    # m: 16 and 257 are outside the decode-batch range, 17 and 256 inside
    assert [ks_of(m, 64, 1024) for m in (16, 17, 256, 257)] == [0, 4, 4, 0]
    # n % 32
    assert [ks_of(64, n, 1024) for n in (32, 40, 48, 56, 64, 96)] == [4, 0, 0, 0, 4, 4]
    # k: % 64, and at least 64
    assert [ks_of(64, 64, k) for k in (56, 63, 64, 72, 120, 128)] == [0, 0, 1, 0, 0, 1]
    # slices stay >= 256: K / (2 ks) = 256 is the last doubling
    assert [ks_of(64, 64, k) for k in (256, 448, 512, 960, 1024, 2048, 4096)] == [1, 1, 2, 1, 4, 8, 16]
    # the 512-workgroup target: tiles * ks <= 512 (m 256 x n 4096: 64 tiles)
    assert ks_of(256, 4096, 1 << 16) == 8 and ks_of(128, 4096, 1 << 16) == 16 and ks_of(128, 128, 1 << 20) == 512
    # every variant's slices fit: m = 256 with >= 96 tiles splits under variant 1 only, and the size covers it
    assert sc.swiglu_slices(256, 12288, 4096) == 0 and ks_of(256, 12288, 4096) == sc.swiglu_slices(256, 12288, 4096, True) > 0
    for m, n, k in ((16, 64, 1024), (17, 64, 1024), (256, 64, 1024), (257, 64, 1024), (64, 40, 1024), (64, 64, 63),
                    (64, 64, 64), (64, 64, 512), (64, 64, 448), (256, 4096, 1 << 16), (256, 12288, 4096)):
        for dt in ("bf16", "fp16"):
            assert _size(L, m, n, k, dt) == sc.workspace_size(m, n, k, dt), (m, n, k, dt)
        assert _size(L, m, n, k, "fp32") == 0
    for bad in ((0, 64, 1024), (64, 0, 1024), (64, 64, 0), (-1, 64, 1024)):
        assert _size(L, *bad, "bf16") == 0
    assert L.pli_gemm_swiglu_workspace_size(64, 64, 1024, 5) == 0
    assert ctypes.sizeof(ctypes.c_size_t) == 8 and _size(L, 256, 1 << 20, 1 << 20, "bf16") == 2 * 1 * 256 * (1 << 20) * 4
