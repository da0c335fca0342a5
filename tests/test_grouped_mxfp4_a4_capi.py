"""pli_gemm_grouped_mxfp4_a4 without a GPU: the argument rules in the documented order, the empty calls, the grid guard"""
import ctypes

import pytest

EINVAL, OK, F32, BF16 = 1000, 0, 0, 2
P = ctypes.c_void_p(4096)  # never dereferenced: validation fails first


@pytest.fixture()
def call(built_lib):
    import pli_hip
    L = pli_hip.lib()

    def f(want, msg=b"", **kw):
        a = dict(x4=P, xe=P, xs=P, gather=P, w=P, we=P, wu=None, wue=None, c=P, offsets=P, experts=4, rows=64, n=64,
                 k=512, ldx4=256, ldxs=16, ldw=256, lds=16, ldc=64, dtype=BF16, stream=None)
        a.update(kw)
        assert L.pli_gemm_grouped_mxfp4_a4(*a.values()) == want and msg in L.pli_last_error(), (kw, L.pli_last_error())
        assert L.pli_last_route() == b""  # nothing is ever launched here
    return f


def test_argument_rules_in_order_and_empty_calls_without_gpu(call):
    rules = [(b"bad dtype", [dict(dtype=F32), dict(dtype=7), dict(dtype=-1)]),
             (b"bad shape", [dict(experts=0), dict(rows=-1), dict(n=-1), dict(k=-32)]),
             (b"MX block of 32", [dict(k=16), dict(k=48), dict(k=500)]),
             (b"leading dimension too small", [dict(ldx4=255), dict(ldxs=15), dict(ldw=255), dict(lds=15), dict(ldc=63)]),
             (b"null pointer", [{name: None} for name in ("x4", "xe", "w", "we", "c", "offsets")] +
              [dict(k=0, ldx4=0, ldxs=0, ldw=0, lds=0, x4=None, xe=None, w=None, we=None, c=None)]),  # k == 0 needs C
             (b"up tables come as a pair", [dict(wu=P), dict(wue=P)]),
             (b"grid too large", [dict(rows=1 << 30, n=1026, ldc=1026)])]  # n % 16 != 0: generic, 2^32 workgroups
    for i, (msg, cases) in enumerate(rules):
        for kw in cases:
            call(EINVAL, msg, **kw)
        for _, later in rules[i + 1:]:  # an earlier rule wins over every later one
            call(EINVAL, msg, **{**later[0], **cases[0]})
    none = dict(x4=None, xe=None, xs=None, gather=None, w=None, we=None, c=None, offsets=None)
    call(OK, rows=0, **none)
    call(OK, n=0, ldc=0, wu=P, **none)  # before any pointer rule, the pair included
    for kw in (dict(rows=0, k=-32), dict(n=0, dtype=9), dict(rows=0, k=48)):  # the argument checks still come first
        call(EINVAL, **kw)
