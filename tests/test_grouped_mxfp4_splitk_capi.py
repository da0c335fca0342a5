"""pli_gemm_grouped_mxfp4_ws and pli_gemm_grouped_mxfp4_workspace_size of include/pli.h without a GPU: the plain call's
argument rules in its order and then splits < 0, before any HIP call, and the workspace size against its closed form."""
import ctypes

EINVAL, OK, F32, BF16 = 1000, 0, 0, 2
P = ctypes.c_void_p(4096)  # never dereferenced: validation fails first


def call(want, msg=b"", **kw):
    import pli_hip
    L = pli_hip.lib()
    a = dict(x8=P, xs=P, gather=P, w=P, we=P, wu=None, wue=None, c=P, offsets=P, experts=4, rows=8, n=64, k=512,
             ldx8=512, ldw=256, lds=16, ldc=64, dtype=BF16, work=P, bytes=1 << 20, splits=0, stream=None)
    a.update(kw)
    assert L.pli_gemm_grouped_mxfp4_ws(*a.values()) == want and msg in L.pli_last_error(), (kw, L.pli_last_error())
    assert L.pli_last_route() == b"" and (want == OK or L.pli_last_error().startswith(b"pli_gemm_grouped_mxfp4_ws: "))


def test_argument_rules_in_order_without_gpu(built_lib):
    rules = [(b"bad dtype", [dict(dtype=F32), dict(dtype=7)]),
             (b"bad shape", [dict(experts=0), dict(rows=-1), dict(n=-1), dict(k=-32)]),
             (b"MX block of 32", [dict(k=16), dict(k=500)]),
             (b"leading dimension too small", [dict(ldx8=511), dict(ldw=255), dict(lds=15), dict(ldc=63)]),
             (b"null pointer", [{name: None} for name in ("x8", "w", "we", "c", "offsets")]),
             (b"up tables come as a pair", [dict(wu=P), dict(wue=P)]),
             (b"grid too large", [dict(rows=1 << 30, n=1026, ldc=1026)]),  # n % 16 != 0: the generic route, 2^32 workgroups
             (b"bad splits", [dict(splits=-1)])]
    for i, (msg, cases) in enumerate(rules):
        for kw in cases + [{**later[0], **cases[0]} for _, later in rules[i + 1:]]:  # an earlier rule wins over every later one
            call(EINVAL, msg, **kw)
    none = dict(x8=None, xs=None, gather=None, w=None, we=None, c=None, offsets=None, work=None, bytes=0)
    call(OK, rows=0, **none)
    call(OK, n=0, ldc=0, wu=P, **none)  # before any pointer rule, the pair included
    call(EINVAL, b"bad splits", rows=0, splits=-1, **none)


def test_workspace_size_is_the_closed_form(built_lib):
    import pli_hip
    size = pli_hip.lib().pli_gemm_grouped_mxfp4_workspace_size
    for rows, sw in ((1, 0), (2, 1), (11, 0), (32, 1)):
        for n, k in ((4096, 14336), (14336, 4096), (144, 640), (16, 128), (256, 2048), (4096, 512)):
            for splits in (0, 1, 2, 3, 5, 16, 40):  # the split rule of include/pli.h, restated
                ks, tiles = k // 128, -(-n // 128)
                s = max(1, min(16, min(splits, ks) if splits else min(-(-512 // tiles), ks // 4)))
                s = -(-ks // -(-ks // s))
                assert size(8, rows, n, k, sw, splits) == (s * rows * n * (1 + sw) * 4 if s >= 2 else 0), (rows, n, k, sw, splits)
    assert size(8, 2, 4096, 14336, 0, 0) == 16 * 2 * 4096 * 4 and size(8, 2, 14336, 4096, 1, 0) == 5 * 2 * 14336 * 2 * 4
    # the call is the plain one: no rows or more than 32, k % 128, n % 16, S < 2, experts past the grid, negative splits
    for e, rows, n, k, splits in ((8, 0, 4096, 4096, 0), (8, 33, 4096, 4096, 0), (8, 8, 4096, 4160, 0), (8, 8, 4100, 4096, 0),
                                  (8, 8, 4096, 4096, 1), (8, 8, 4096, 128, 4), (8, 8, 4096, 256, 0), (65536, 8, 4096, 4096, 0),
                                  (0, 8, 4096, 4096, 0), (8, 8, 4096, 4096, -1)):
        assert size(e, rows, n, k, 0, splits) == 0, (e, rows, n, k, splits)
