"""The weight-only MXFP4 linear entry points of include/pli.h without a GPU (tests/test_capi.py holds that they are
declared and exported): each argument rule returns PLI_EINVAL with its message before any HIP call, empty calls return
PLI_OK with NULL operands."""
import ctypes

import pytest

EINVAL, OK, F32, BF16 = 1000, 0, 0, 2
P = ctypes.c_void_p(4096)  # never dereferenced: validation fails first.  Per call: valid arguments in order, small lds, pointers
CALLS = {
    "pli_linear_mxfp4w": (dict(x=P, w=P, s=P, bias=None, c=P, m=4, n=64, k=512, ldx=512, ldw=256, lds=16, ldc=64, dtype=BF16,
                               ws=None, ws_bytes=0), dict(ldx=511, ldw=255, lds=15, ldc=63), ("x", "w", "s", "c")),
    "pli_linear_swiglu_mxfp4w": (dict(x=P, wg=P, sg=P, wu=P, su=P, h=P, m=4, n=64, k=512, ldx=512, ldwg=256, ldsg=16, ldwu=256,
                                      ldsu=16, ldh=64, dtype=BF16, ws=None, ws_bytes=0),
                                 dict(ldx=8, ldwg=8, ldsg=8, ldwu=8, ldsu=8, ldh=8), ("x", "wg", "sg", "wu", "su", "h")),
    "pli_gemv_mxfp4w": (dict(w=P, s=P, x=P, y=P, m=64, k=512, ldw=256, lds=16, dtype=BF16), dict(ldw=255, lds=15),
                        ("w", "s", "x", "y")),
}


@pytest.mark.parametrize("name", CALLS)
def test_argument_validation_without_gpu(built_lib, name):
    import pli_hip
    L, (defaults, lds, nulls) = pli_hip.lib(), CALLS[name]
    f, err = lambda **kw: getattr(L, name)(*{**defaults, **kw}.values(), None), L.pli_last_error  # noqa: E731
    for dt in (F32, 7, -1):
        assert f(dtype=dt) == EINVAL and (name + ": bad dtype").encode() in err(), dt
    for dim in ("m", "k") + (() if "gemv" in name else ("n",)):
        assert f(**{dim: -1}) == EINVAL and (name + ": bad shape").encode() in err(), dim
    assert f(k=48) == EINVAL and b"not a multiple of the MX block of 32" in err() and f(k=16) == f(k=500) == EINVAL
    for ld, v in lds.items():
        assert f(**{ld: v}) == EINVAL and b"leading dimension too small" in err(), ld
    for p in nulls:  # the scale bytes have no default
        assert f(**{p: None}) == EINVAL and b"null pointer" in err(), p
    if "gemv" not in name:  # the widen route (m > 16, no fast route, a workspace): aligned and large enough
        shape = {d: v for d, v in dict(m=17, n=24, k=64, ldx=64, ldw=32, ldwg=32, ldwu=32, lds=2, ldsg=2, ldsu=2, ldc=24,
                                       ldh=24).items() if d in defaults}
        need = getattr(L, name + "_workspace_size")(17, 24, 64, BF16)
        assert need == (2 if "swiglu" in name else 1) * 24 * 64 * 2
        assert f(ws=P, ws_bytes=need - 1, **shape) == EINVAL and b"workspace" in err()
        assert f(ws=ctypes.c_void_p(4104), ws_bytes=need, **shape) == EINVAL and b"16-byte aligned" in err()
    # m == 0 or n == 0: PLI_OK before any HIP call, every operand may be NULL; the argument checks still come first
    none = {p: None for p in nulls}
    assert f(m=0, **none) == OK and f(m=0, dtype=F32) == EINVAL and f(m=0, k=48) == EINVAL
    assert "gemv" in name or f(n=0, **none) == OK
    assert L.pli_last_route() == b""  # nothing was launched
