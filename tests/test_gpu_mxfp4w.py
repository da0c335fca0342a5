"""Weight-only MXFP4 linear (pli_linear_mxfp4w / pli_gemv_mxfp4w / pli_linear_swiglu_mxfp4w) on the device.

Oracle: float64 numpy over pli_hip.dequantize_weight_mxfp4.  Bound: the project's linear bound
|err| <= LIN_TOL[dt] * (|ref| + 1), bf16 1e-2, fp16 4e-3; an fp32-accumulate emulation of these semantics stays under
EMULATION_WORST of it at these shapes (tests/test_mxfp4w_emulation_cpu.py asserts that figure).  Scale bytes differ
between neighbouring blocks and rows (weight()), so a scale taken from the wrong block or row shows.  The cost of
quantising is the format's, not the kernels', and is asserted nowhere.  pli_last_route is asserted for each.
"""
import numpy as np
import pytest
import torch

from oracle.numerics import seeded_normal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LIN_TOL = {"bf16": 1e-2, "fp16": 4e-3}
EMULATION_WORST = 0.40
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
SENTINEL = -1024.0  # exact in bf16 and fp16
VEC, SMALLM = "mxfp4w_vec", "mxfp4w_smallm"
# (m, n, k, bias, pad, swiglu, route).  mxfp4w_vec_cfg: K <= 2048 -> (ROWS 8, CPL 1), K <= 4096 -> (4, 2), else (2, 4); a
# trip is 64 CPL chunks of 32.  vec: one block; a lane tail (65 chunks, a (4, 2) case); +-32 of the trip boundaries 2048,
# 4096, 8192; n % ROWS: ROWS 8 (first two rows) tails 3 2 4 7 5 6 3 1, ROWS 4 tails 1 3 2 1, ROWS 2 tail 1; m in {1, 2, 3,
# 16}.  smallm: 1, 2, unroll depth + 1 granules of 512, m around every batch-group count.  SwiGLU: NBG 1 and 4 on smallm.
CASES = [(1, 3, 32, 0, 0, 0, VEC), (1, 10, 64, 0, 0, 0, VEC), (2, 12, 992, 1, 0, 0, VEC), (2, 15, 2016, 0, 1, 0, VEC),
         (1, 13, 2048, 0, 0, 0, VEC), (3, 6, 2048, 0, 1, 0, VEC), (16, 11, 288, 0, 1, 0, VEC), (3, 17, 96, 1, 0, 0, VEC),
         (1, 9, 32 * 65, 1, 0, 0, VEC), (3, 7, 2080, 1, 1, 0, VEC), (1, 6, 4064, 0, 0, 0, VEC), (16, 5, 4096, 1, 1, 0, VEC),
         (1, 3, 4128, 1, 1, 0, VEC), (2, 3, 8160, 0, 0, 0, VEC), (16, 5, 8192, 0, 1, 0, VEC), (2, 3, 8224, 1, 0, 0, VEC)]
CASES += [(m, 16 if (m + k // 512) % 2 else 48, k, 1, m in (15, 33), 0, SMALLM)
          for k in (512, 1024, 9 * 512) for m in (2, 15, 16, 17, 33, 128)]
CASES += [(1, 33, 256, 0, 0, 1, VEC), (3, 5, 4128, 0, 1, 1, VEC), (16, 48, 5 * 512, 0, 1, 1, SMALLM), (33, 16, 1024, 0, 1, 1, SMALLM)]


def weight(n, k, seed, dt, gain=1.0):
    """(codes, exps, dequantised float64) on the CPU: N(0,1) * 2^p * gain, p a seeded permutation of -6 .. 6 per block"""
    import pli_hip
    p = (np.random.RandomState(seed).permutation(n * k // 32) % 13 - 6).reshape(n, k // 32)
    w = seeded_normal((n, k), seed, "fp32") * np.repeat(np.exp2(p), 32, axis=1).astype(np.float32) * np.float32(gain)
    codes, exps = pli_hip.quantize_weight_mxfp4(torch.from_numpy(w), TORCH_DT[dt])
    return codes, exps, pli_hip.dequantize_weight_mxfp4(codes, exps).double().numpy()


def operands(m, n, k, bias, swiglu, dt):
    seed = 5000 + m + n + k  # -> (x, [(codes, exps, deq)], bias or None, float64 reference) on the CPU
    x = seeded_normal((m, k), seed, dt)
    ws = [weight(n, k, seed + 1 + i, dt, 2.0 ** -5 if swiglu else 1.0) for i in range(2 if swiglu else 1)]
    b = seeded_normal((n,), seed + 7, dt) if bias else None
    ref = x.astype(np.float64) @ ws[0][2].T
    if swiglu:
        ref = ref / (1.0 + np.exp(-ref)) * (x.astype(np.float64) @ ws[1][2].T)
    return x, ws, b, (ref if b is None else ref + b.astype(np.float64))


def ratio(got, ref, dt):  # max |err| / bound
    return float((np.abs(np.asarray(got, np.float64) - ref) / (LIN_TOL[dt] * (np.abs(ref) + 1.0))).max())


@pytest.fixture(scope="module")
def pli(built_lib):
    return __import__("pli_hip")


class Case:
    """operands() on the device; pad: views with padded leading dimensions, NaN / 0xFF in the padding, C in a frame"""

    def __init__(self, m, n, k, dt, bias=False, pad=False, swiglu=False):
        tdt, p = TORCH_DT[dt], int(pad)
        x, ws, b, self.ref = operands(m, n, k, bias, swiglu, dt)
        self.m, self.n, self.dt = m, n, dt
        xw = torch.full((m, k + 8 * p), float("nan"), dtype=tdt)
        xw[:, :k] = torch.from_numpy(x).to(tdt)
        self.x, self.w = xw.to(DEV)[:, :k], []
        for codes, exps, _ in ws:
            cw = torch.full((n, k // 2 + 48 * p), 0x77, dtype=torch.uint8)
            ew = torch.full((n, k // 32 + 5 * p), 0xFF, dtype=torch.uint8)
            cw[:, 16 * p:16 * p + k // 2], ew[:, 3 * p:3 * p + k // 32] = codes, exps
            self.w += [cw.to(DEV)[:, 16 * p:16 * p + k // 2], ew.to(DEV)[:, 3 * p:3 * p + k // 32]]
        self.bias = torch.from_numpy(b).to(tdt).to(DEV) if bias else None
        self.whole = torch.full((m + 2 * p, n + 8 * p), SENTINEL, dtype=tdt, device=DEV)
        self.out = self.whole[:m, :n]

    def run(self, pli, route, **kw):  # the linear (SwiGLU for two weights): route, bound, frame untouched
        fn = pli.linear_swiglu_mxfp4w if len(self.w) == 4 else pli.linear_mxfp4w
        self.whole.fill_(SENTINEL)
        fn(self.x, *self.w, out=self.out, **({} if len(self.w) == 4 else {"bias": self.bias}), **kw)
        assert pli.last_route().startswith(route), pli.last_route()
        r = ratio(self.out.float().cpu().numpy(), self.ref, self.dt)
        w = self.whole.float().cpu()
        assert r <= 1.0 and bool((w[self.m:] == SENTINEL).all()) and bool((w[:, self.n:] == SENTINEL).all()), (route, r)
        return self.out


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "m{}n{}k{}{}{}{}".format(*c[:3], *("b" * c[3], "p" * c[4], "s" * c[5])))
def test_fast_routes_against_oracle(pli, case, dt):
    m, n, k, bias, pad, swiglu, route = case
    c = Case(m, n, k, dt, bias, pad, swiglu)
    got = c.run(pli, route + "<swiglu>" * swiglu)
    if m == 1 and not bias and not swiglu:  # the gemv is bitwise the linear call, on the same kernel
        assert torch.equal(pli.gemv_mxfp4w(*c.w, c.x[0]), got[0]) and pli.last_route() == route


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_generic_widen_and_k0(pli, dt):
    tdt = TORCH_DT[dt]
    c = Case(2, 16, 512, dt)
    buf = torch.zeros(16 * 256 + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = c.w[0].reshape(-1)
    c.w[0] = buf[1:].view(16, 256)  # the codes start 1 byte into their buffer
    c.run(pli, "mxfp4w_generic")
    # m = 17, n = 24, k = 64: generic without a workspace, widen + the 16-bit GEMM with one, plain and SwiGLU
    for swiglu in (False, True):
        c = Case(17, 24, 64, dt, bias=not swiglu, swiglu=swiglu)
        c.run(pli, "mxfp4w_generic")
        nbytes = pli.linear_mxfp4w_workspace_bytes(17, 24, 64, tdt, swiglu=swiglu)
        assert nbytes == (1 + swiglu) * 24 * 64 * 2
        ws = torch.zeros(nbytes + 64, dtype=torch.uint8, device=DEV)
        c.run(pli, "mxfp4w_widen+mxfp4w_widen+" if swiglu else "mxfp4w_widen+", workspace=ws)
        assert "mxfp4w" not in pli.last_route().replace("mxfp4w_widen+", "") and bool((ws[nbytes:] == 0).all())
    x, empty = torch.zeros(3, 0, dtype=tdt, device=DEV), torch.zeros(5, 0, dtype=torch.uint8, device=DEV)  # k = 0
    bias, out = torch.arange(5, dtype=tdt, device=DEV), torch.full((3, 5), SENTINEL, dtype=tdt, device=DEV)
    assert bool((pli.linear_mxfp4w(x, empty, empty, out=out) == 0).all())
    assert torch.equal(pli.linear_mxfp4w(x, empty, empty, bias=bias, out=out), bias.expand(3, 5))
    assert pli.last_route() == "mxfp4w_generic"
    assert bool((pli.linear_swiglu_mxfp4w(x, empty, empty, empty, empty, out=out) == 0).all())


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_scale_contract_ends_widen_exactly(pli, dt):
    """scale bytes at both ends of the contract range, every code (0.5 * 2^lo is T's smallest normal): the widened
    workspace is bitwise the dequantised weight, every route meets the oracle"""
    tdt, (lo, hi), n, k = TORCH_DT[dt], pli.MXFP4_EXP_RANGE[TORCH_DT[dt]], 24, 512
    codes = (torch.arange(n * k // 2) * 37 % 256).to(torch.uint8).view(n, k // 2)
    e = torch.tensor([lo, hi]).repeat(n, k // 64)  # the ends alternate along k; X is scaled against them per block
    x_np = seeded_normal((17, k), 8300, dt).round().clip(-2, 2) * np.exp2(np.where(e[0] > 0, 5 - hi, -5 - lo).repeat(32))
    w = [codes.to(DEV), (e + 127).to(torch.uint8).to(DEV)]
    deq = pli.dequantize_weight_mxfp4(*w)
    assert float(deq.abs().max()) == 6.0 * 2.0 ** hi and float(deq[deq != 0].abs().min()) == 2.0 ** (lo - 1)
    x, ref = torch.from_numpy(x_np).to(tdt).to(DEV), x_np.astype(np.float64) @ deq.double().cpu().numpy().T
    ws = torch.zeros(n * k * 2, dtype=torch.uint8, device=DEV)
    for m, rows, route in ((17, n, "mxfp4w_widen+"), (17, 16, SMALLM), (1, n, VEC)):
        got = pli.linear_mxfp4w(x[:m], w[0][:rows], w[1][:rows], workspace=ws)
        assert pli.last_route().startswith(route)
        assert ratio(got.float().cpu().numpy(), ref[:m, :rows], dt) <= 1.0, route
    assert torch.equal(ws.view(tdt).view(n, k), deq.to(tdt))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("m,n,k,route", [(3, 7, 2080, VEC), (17, 48, 1024, SMALLM)])
def test_nan_scale_byte_poisons_exactly_its_row(pli, m, n, k, route, dt):
    c = Case(m, n, k, dt, bias=True)
    a, keep = c.run(pli, route).clone(), [j for j in range(n) if j != 4]
    for blk in (0, k // 64, k // 32 - 1):
        exps = c.w[1].clone()
        exps[4, blk] = 0xFF
        b = pli.linear_mxfp4w(c.x, c.w[0], exps, bias=c.bias)
        assert pli.last_route() == route and bool(torch.isnan(b[:, 4]).all()) and torch.equal(a[:, keep], b[:, keep]), blk


@pytest.mark.parametrize("m,n,k,route", [(4, 48, 1024, SMALLM), (4, 7, 2080, VEC)])
def test_graph_replays_after_in_place_changes(pli, m, n, k, route):
    c = Case(m, n, k, "bf16", swiglu=True)
    x, gc, ge, uc, ue, out, h = [t.clone() for t in (c.x, *c.w, c.out, c.out)]

    step = lambda: (pli.linear_mxfp4w(x, gc, ge, out=out), pli.linear_swiglu_mxfp4w(x, gc, ge, uc, ue, out=h))  # noqa: E731
    step(), torch.cuda.synchronize()  # warm up outside the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for rep in range(3):  # change x, the codes and the scale bytes in place, then replay
        x.copy_(torch.from_numpy(seeded_normal((m, k), 9600 + rep, "bf16")).to(torch.bfloat16))
        gc.copy_(torch.roll(uc, rep + 1, dims=0))
        uc[1] = 0x3A
        ge.copy_(torch.flip(ue, dims=[0]))
        ue.sub_(1)
        g.replay()
        torch.cuda.synchronize()
        got_out, got_h = out.clone(), h.clone()
        assert torch.equal(got_out, pli.linear_mxfp4w(x, gc, ge)) and pli.last_route() == route, rep
        assert torch.equal(got_h, pli.linear_swiglu_mxfp4w(x, gc, ge, uc, ue)) and pli.last_route() == route + "<swiglu>"


def test_ch03_benchmark_gemv_mxfp4w_runs_the_kernel(pli):
    import ch03
    r = ch03.benchmark_gemv_mxfp4w(256, 512, dtype=torch.bfloat16, warmup=2, iterations=5)
    assert pli.last_route() == VEC and r.kernel_us is not None and r.kernel_us > 0 and r.kernel_gbps > 0
