"""GPU parity of every plain GEMM / GEMV route (pli_gemm / _ws / _variant,
pli_gemm_f32out, pli_gemv / _variant) against the f64 oracle, per element, over
the case list of tests/gemm_cases.py: gemm_skinny_nt (NB 1 - 16, CPL 2 - 16 at
each K boundary), gemv_vec through pli_gemm, gemm_smallm_nt (NBG 1 - 8),
gemm_midm_nt (MC 1 - 4), the split-K kernels gemm_splitk_nt and
gemm_splitk_lds_nt (MC 1 - 4, NB 2 / 3, partial + reduce and the one-slice
direct store with and without a bias), gemm_mfma, gemm_256 and the phased
gemm_256p at every SCHED and group_m, gemm_w5 (tile, persistent, fp32 epilogue),
gemm_w4v, gemm_f32_mfma (NW 8 / 4), gemm_generic, gemm_f32out_generic and
gemv_vec<ROWS, CPL, NTL, WPB, EXACT> for variants 0 - 16 + gemv_scalar, in bf16
and fp16 (fp32 where the kernel takes it), with

* the kernel name asserted against the CPU replay of the dispatch;
* a and b as views with different row strides, NaN in the padding and in three
  spare rows after each, the bias inside a NaN-filled buffer;
* the output inside a sentinel-filled buffer with guard rows, ldc = n + 8 and
  three spare rows (decode_step_cases.Guarded / assert_untouched);
* two bounds per element, both asserted: (a) the project's, and (b) one output
  rounding + the fp32 accumulation (gemm_cases' docstring).

Relations, bit for bit: the padded and the contiguous operand family per
instance; gemv_vec through pli_gemm and the skinny kernel with a zero bias; the
persistent gemm_w5 walk and its one-tile form (variant 41); pli_gemm's 16-bit
output and pli_gemm_f32out's rounded once, where both run the same chain; K = 0
gives the bias or zero.  Through the C ABI a workspace one byte short takes the
unsplit route and is left alone, an exactly sized one is filled and not
overrun, and the one-slice routes leave their workspace untouched."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import decode_step_cases as dc
import gemm_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
_id = lambda v: gc.case_id(v) if isinstance(v, tuple) else v  # noqa: E731
PAIRS = [(c, dt) for c in gc.ALL_CASES for dt in c.dts]
CONTIG_PAIRS = [(c, dt) for c in gc.CONTIG_CASES for dt in c.dts]
N_DEVICE_CASES = len(gc.device_cases(256))
WS_BYTE = 0xA5
WORST = {}      # (api, kernel) -> [max err / (a), max err / (b)], printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    print("\nworst ratio per route: err / (a), err / (b)")
    for (api, kernel), (ra, rb) in sorted(WORST.items()):
        print(f"  {api:7s} {kernel:40s} {ra:.3f} {rb:.3f}")


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch(c, op, dt, padded=True, variant="case"):
    """one call on the case's device operands into a Guarded output; returns it with the route string
    pli_last_route reports.  ws "auto" goes through pli_hip.gemm, 0 / "min" through the C ABI"""
    import pli_hip
    v = c.variant if variant == "case" else variant
    a, b, bias, out = gc.device_operands(c, op, dt, DEV, padded)
    assert (a.data_ptr() % 16 != 0) == (padded and c.mode == "offa" and c.api != "gemv")
    if c.api == "gemv":
        assert a.stride(0) == gc.leading_dims(c, padded)[1] and (b.data_ptr() % 16 != 0) == (padded and c.mode == "offa")
        pli_hip.gemv(a, b, out=out.view[:c.m], variant=v)
    elif c.api == "f32out":
        assert (a.stride(0), b.stride(0)) == gc.leading_dims(c, padded)[:2]
        o = gc.addressed(c, padded)(out.view).view(c.m, c.n)
        assert (o.data_ptr() % 16 != 0) == (padded and c.mode == "offc")
        pli_hip.gemm_f32out(a, b, out=o)
    elif c.ws == "auto":
        if bias is not None:
            assert bias.data_ptr() % 16 == ({"bias2": 2, "bias8": 8}.get(c.mode, 0) if padded else 0)
        pli_hip.gemm(a, b, trans_b=c.trans_b, bias=bias, out=out.view[:c.m], variant=v)
    else:
        L = pli_hip.lib()
        nbytes = gc.case_ws_bytes(c, dt)
        ws = torch.full((max(nbytes, 16),), WS_BYTE, dtype=torch.uint8, device=DEV)
        rc = L.pli_gemm_ws_variant(a.data_ptr(), b.data_ptr(), out.view.data_ptr(), None if bias is None else bias.data_ptr(),
                                   c.m, c.n, c.k, a.stride(0), b.stride(0), out.view.stride(0), int(c.trans_b),
                                   gc.DTYPE_CODE[dt], ctypes.c_void_p(ws.data_ptr() if nbytes else None), nbytes,
                                   ctypes.c_void_p(_stream()), v or 0)
        assert rc == 0, L.pli_last_error()
        route = pli_hip.last_route()
        torch.cuda.synchronize()
        assert bool((ws == WS_BYTE).all()), "a one-slice route wrote its workspace"
        return out, route
    route = pli_hip.last_route()
    torch.cuda.synchronize()
    return out, route


def _got(out, c, padded=True):
    return gc.addressed(c, padded)(out.view)


def _check(out, c, ref, dt, what, padded=True):
    """the addressed part finite and inside (a) and (b); the spare rows, the row padding and the guards untouched"""
    got = dc.f64(_got(out, c, padded))
    nonfinite = int((~np.isfinite(got)).sum())
    assert nonfinite == 0, f"{what}: {nonfinite} non-finite outputs (padding or a spare row was read)"
    ra, rb = gc.ratios(got, c, ref, dt)
    print(f"{what}: err / (a) {ra:.3f}, err / (b) {rb:.3f}")
    w = WORST.setdefault((c.api, c.kernel), [0.0, 0.0])
    w[0], w[1] = max(w[0], ra), max(w[1], rb)
    assert ra <= 1.0 and rb <= 1.0, (what, ra, rb, gc.worst(got, c, ref, dt))
    dc.assert_untouched(out, gc.addressed(c, padded), what=what)


def _bits(out, c, dt, padded=True):
    return _got(out, c, padded).view(gc.BITS[gc.out_dtype(c, dt)])


@pytest.mark.parametrize("c,dt", PAIRS, ids=_id)
def test_gemm_route_per_element(c, dt):
    op, ref = gc.case_reference(c, dt)
    out, route = _launch(c, op, dt)
    assert route == c.kernel == gc.case_route(c, dt, cus=_cus()).kernel, (gc.case_id(c), route)
    _check(out, c, ref, dt, f"{gc.case_id(c)} {dt}")


@pytest.mark.parametrize("c,dt", CONTIG_PAIRS, ids=_id)
def test_gemm_contiguous_operands_match_padded_bitwise(c, dt):
    """ld == k and ldc == n: the same route, the same bounds, and bit for bit the padded family's values"""
    op, ref = gc.case_reference(c, dt)
    out, route = _launch(c, op, dt, padded=False)
    assert route == c.kernel == gc.case_route(c, dt, padded=False, cus=_cus()).kernel, (gc.case_id(c), route)
    _check(out, c, ref, dt, f"{gc.case_id(c)} {dt} contiguous", padded=False)
    padded, _ = _launch(c, op, dt)
    assert torch.equal(_bits(out, c, dt, False), _bits(padded, c, dt)), gc.case_id(c)


@pytest.mark.parametrize("i", range(N_DEVICE_CASES))
def test_gemm_device_sized_cases_per_element(i):
    """the persistent gemm_w5 walk (pli_gemm and pli_gemm_f32out) and gemm_f32_mfma's four-wave form at shapes
    computed from the device's CU count; the walk bit for bit against the one-tile form (variant 41)"""
    cus = _cus()
    c = gc.device_cases(cus)[i]
    for dt in c.dts:
        r = gc.case_route(c, dt, cus=cus)
        assert (r.kernel, r.inst) == (c.kernel, c.inst), (cus, gc.case_id(c), r)
        op, ref = gc.case_reference(c, dt)
        out, route = _launch(c, op, dt)
        assert route == c.kernel, (gc.case_id(c), route)
        _check(out, c, ref, dt, f"{gc.case_id(c)} {dt} ({cus} CUs)")
        if c.api == "gemm" and c.kernel == gc.W5:
            tile, r41 = _launch(c, op, dt, variant=41)
            assert r41 == gc.W5 and gc.gemm_route(c.m, c.n, c.k, dt, c.trans_b, c.bias, 41, 0, gc.leading_dims(c),
                                                  cus=cus).inst == "w5 tile"
            assert torch.equal(_bits(out, c, dt), _bits(tile, c, dt)), "the walk differs from the one-tile form"
        if c.api == "f32out":       # pli_gemm's 16-bit output is this fp32 result rounded once (the same MFMA chains)
            g = gc._case(gc.W5, c.inst.replace("f32 ", ""), (c.m, c.n, c.k), dts=c.dts)
            assert gc.case_route(g, dt, cus=cus) == gc.Route(g.kernel, g.inst)
            o16, r16 = _launch(g, op, dt)
            assert r16 == gc.W5
            want = _got(out, c).view(c.m, c.n).to(gc.TDT3[dt])
            assert torch.equal(o16.view[:c.m].view(gc.BITS[dt]), want.view(gc.BITS[dt]))


SKINNY_ONE_ROW = [(c, dt) for c in gc.GEMM_CASES if c.kernel == gc.GEMV_VEC and c.kind == "default" for dt in c.dts]


@pytest.mark.parametrize("c,dt", SKINNY_ONE_ROW, ids=_id)
def test_gemv_through_gemm_equals_the_skinny_kernel_bitwise(c, dt):
    """M = 1 without a bias is gemv_vec, with one (zeros) gemm_skinny_nt<1, CPL>: the same per-lane chunk and FMA
    order, at each K boundary of the skinny kernel's CPL choice"""
    assert (c.m, c.bias) == (1, False) and len(SKINNY_ONE_ROW) == 2 * len(gc.SKINNY_KS)
    op, _ = gc.case_reference(c, dt)
    y, r0 = _launch(c, op, dt)
    sk = c._replace(kernel=gc.SKINNY, inst=f"NB1,CPL{gc.SKINNY_K_CPL[c.k]}", bias=True)
    assert gc.case_route(sk, dt) == gc.Route(sk.kernel, sk.inst)
    z, r1 = _launch(sk, gc.Operands(op.a, op.b, np.zeros(c.n, np.float32)), dt)
    assert (r0, r1) == (gc.GEMV_VEC, gc.SKINNY)
    assert torch.equal(_bits(y, c, dt), _bits(z, sk, dt))


F32_PAIRS = [(c, dt) for c in gc.F32OUT_CASES if c.kernel == gc.SPLIT_L and 16 < c.m <= 2048 and c.kind == "default"
             for dt in c.dts]


@pytest.mark.parametrize("c,dt", F32_PAIRS, ids=_id)
def test_gemm_16bit_output_is_the_f32out_result_rounded_once(c, dt):
    """gemm_splitk_lds_nt with one slice: pli_gemm (variant 25, any workspace) stores the tile rounded, pli_gemm_f32out
    stores it as fp32 -- the same MFMA chain"""
    op, _ = gc.case_reference(c, dt)
    f32, _ = _launch(c, op, dt)
    g = gc._case(gc.SPLIT_L, f"MC{gc._mc(c.m)},ks1,lds,NB2,direct-store", (c.m, c.n, c.k), variant=25, ws="min")
    assert gc.case_route(g, dt) == gc.Route(g.kernel, g.inst)
    o16, route = _launch(g, op, dt)
    assert route == gc.SPLIT_L
    want = _got(f32, c).view(c.m, c.n).to(gc.TDT3[dt])
    assert torch.equal(o16.view[:c.m].view(gc.BITS[dt]), want.view(gc.BITS[dt]))


# ------------------------------------------------------------------- K == 0
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("tb", [True, False], ids=["NT", "NN"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_gemm_k0_gives_the_bias_or_zero_bitwise(dt, tb, bias):
    """gemm_generic at K = 0: C = bias (or 0), A and B not read"""
    import pli_hip
    m, n = 65, 33
    assert gc.gemm_route(m, n, 0, dt, tb, bias, None, 0).kernel == gc.GENERIC
    a = torch.empty(m, 0, dtype=gc.TDT3[dt], device=DEV)
    b = torch.empty((n, 0) if tb else (0, n), dtype=gc.TDT3[dt], device=DEV)
    bv = torch.from_numpy(gc.round_to_dtype(gc.seeded_normal((n,), 77), dt)).to(gc.TDT3[dt]).to(DEV) if bias else None
    out = dc.Guarded((m + 3, n), dt, DEV, strides=(n + 8, 1))
    pli_hip.gemm(a, b, trans_b=tb, bias=bv, out=out.view[:m])
    assert pli_hip.last_route() == gc.GENERIC
    torch.cuda.synchronize()
    want = bv.expand(m, n) if bias else torch.zeros(m, n, dtype=gc.TDT3[dt], device=DEV)
    assert torch.equal(out.view[:m].view(gc.BITS[dt]), want.contiguous().view(gc.BITS[dt]))
    dc.assert_untouched(out, lambda v: v[:m], what="K = 0")


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_gemv_and_f32out_k0_give_zeros(dt):
    import pli_hip
    m, n = 9, 33
    y = dc.Guarded((m + 3,), dt, DEV)
    pli_hip.gemv(torch.empty(m, 0, dtype=gc.TDT3[dt], device=DEV), torch.empty(0, dtype=gc.TDT3[dt], device=DEV),
                 out=y.view[:m])
    torch.cuda.synchronize()
    assert bool((y.view[:m].view(gc.BITS[dt]) == 0).all())
    dc.assert_untouched(y, lambda v: v[:m], what="gemv K = 0")
    if dt != "fp32":
        c = dc.Guarded((m * n,), "fp32", DEV)
        pli_hip.gemm_f32out(torch.empty(m, 0, dtype=gc.TDT3[dt], device=DEV), torch.empty(n, 0, dtype=gc.TDT3[dt], device=DEV),
                            out=c.view.view(m, n))
        assert pli_hip.last_route() == gc.F32OUT_GENERIC
        torch.cuda.synchronize()
        assert bool((c.view.view(torch.int32) == 0).all())
        dc.assert_untouched(c, lambda v: v, what="f32out K = 0")


# ---------------------------------------- the workspace, through the C ABI
WS_CASES = [c for c in gc.GEMM_CASES if c.kind == "default" and c.variant is None and
            (c.m, c.n, c.k) in ((65, 160, 512), (129, 32, 1024), (520, 160, 512))]


def _call_ws(c, op, dt, ws_ptr, ws_bytes):
    """pli_gemm_ws on the padded operands; returns the Guarded output and the route"""
    import pli_hip
    a, b, bias, out = gc.device_operands(c, op, dt, DEV)
    rc = pli_hip.lib().pli_gemm_ws(a.data_ptr(), b.data_ptr(), out.view.data_ptr(), None if bias is None else bias.data_ptr(),
                                   c.m, c.n, c.k, a.stride(0), b.stride(0), out.view.stride(0), 1, gc.DTYPE_CODE[dt],
                                   ctypes.c_void_p(ws_ptr), ws_bytes, ctypes.c_void_p(_stream()))
    assert rc == 0, pli_hip.lib().pli_last_error()
    route = pli_hip.last_route()
    torch.cuda.synchronize()
    return out, route


@pytest.mark.parametrize("c,dt", [(c, dt) for c in WS_CASES for dt in c.dts], ids=_id)
def test_gemm_workspace_one_byte_short_takes_the_unsplit_route(c, dt):
    assert len(WS_CASES) == 3
    op, ref = gc.case_reference(c, dt)
    ks = gc.split_ks(c)
    need = ks * c.m * c.n * 4          # the slices this call uses (pli_gemm_workspace_size covers every variant's)
    assert 0 < need <= gc.workspace_size(c.m, c.n, c.k, True, dt)
    ws = torch.full((need,), WS_BYTE, dtype=torch.uint8, device=DEV)
    out, route = _call_ws(c, op, dt, ws.data_ptr(), need - 1)
    unsplit = gc.case_route(c, dt, workspace=need - 1)
    assert route == unsplit.kernel and "splitk" not in route, (route, unsplit)
    _check(out, c._replace(kernel=unsplit.kernel), ref, dt, f"{gc.case_id(c)} {dt} short workspace")
    assert bool((ws == WS_BYTE).all()), "the refused workspace was written"


@pytest.mark.parametrize("c,dt", [(c, dt) for c in WS_CASES for dt in c.dts], ids=_id)
def test_gemm_workspace_exactly_sized_is_not_overrun(c, dt):
    op, ref = gc.case_reference(c, dt)
    need, guard = gc.split_ks(c) * c.m * c.n * 4, 4096
    buf = torch.full((need + 2 * guard,), WS_BYTE, dtype=torch.uint8, device=DEV)
    out, route = _call_ws(c, op, dt, buf.data_ptr() + guard, need)
    assert route == c.kernel == gc.case_route(c, dt, workspace=need).kernel
    _check(out, c, ref, dt, f"{gc.case_id(c)} {dt} exact workspace")
    assert bool((buf[:guard] == WS_BYTE).all()) and bool((buf[guard + need:] == WS_BYTE).all()), \
        "bytes outside the workspace were written"
    planes = buf[guard:guard + need].view(torch.int32)   # ks planes of m x n fp32, every element written
    unwritten = int((planes == int.from_bytes(bytes([WS_BYTE] * 4), "little", signed=True)).sum())
    assert unwritten == 0 and bool(torch.isfinite(planes.view(torch.float32)).all()), unwritten
