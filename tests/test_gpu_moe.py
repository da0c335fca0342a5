"""GPU parity of the MoE path: pli_moe_route, pli_gemm_grouped (plain and
fused SwiGLU), pli_moe_combine and ch09.MoELayer, against the f64 oracle and
the reference's own layer output (moe.npz).

The first three tests are the end-to-end ones (max-norm bounds).  The others
hold every kernel per element, on the case lists of tests/moe_cases.py, with
every output inside a sentinel-filled buffer with guard rows
(tests/decode_step_cases.py: Guarded / assert_untouched) and NaN wherever a
kernel has no business reading (tokens no expert references, row and weight
padding, the weights of experts without rows, rows of Y no pos names, the
padding of the logits):

* grouped GEMM: |err| <= LIN_TOL * (|ref| + 1) per element (bf16 1e-2, fp16
  4e-3), ref = oracle.linear.linear / swiglu in float64 per expert on
  x[gather[rows]]; the output has three spare rows and, padded, ldc = n + 8,
  all of which must keep the sentinel.  The CPU emulation of the semantics
  (tests/test_moe_emulation_cpu.py) sits at 0.20 .. 0.33 (bf16) and
  0.05 .. 0.10 (fp16) of the bound.  Each case's id names the instance it
  reaches, asserted on the CPU against a replay of grouped_dispatch and here
  against pli_last_route:
    gemm_grouped_nt<T, NBG 1/2/4/8, SW 0/1>      remainder loop only, one body
      step, body + remainder, two chunks of the c0 loop (130 rows)
    gemm_grouped_lds_nt<T, MC 1/2/3/4, SW 0/1>   K 128 (two steps), three
      column tiles, slabs of 1 / 128 rows, rows_bound 1024
    gemm_256g<T, SW 0/1>                          255 / 256 / 257 / 1 rows,
      ragged last column tile, (1100, 1100) at rows_bound 2200
  in bf16 and fp16.  No bitwise equality between routes is asserted: the
  kernels' comments claim none.  One more case has 65536 experts, more than
  blockIdx.z of the LDS-staged kernel holds: the dispatch takes the
  weight-streaming kernel, every empty expert's table entry names one NaN
  weight.
* the chain W1/W3 -> W2 -> combine: each stage against its own float64
  reference on the previous stage's stored output.
* router, through the C ABI (ld_logits > experts, NaN padding), for
  moe_route_kernel<float / f16 / bf16>: expert_idx equal to the oracle's
  (ties to the lower index), weights rtol 1e-5 / atol 1e-6, rows summing to 1
  within 1e-6 when normalised, offsets / pos / gather consistent, guards and
  gather past T * k untouched.
* combine alone, moe_combine_kernel<f16 / bf16>: moe_cases.combine_ratio <= 1
  (one rounding to the storage type + the fp32 fma chain), H 8 / 2048 / 2056 /
  4104 (one, one full, two and three passes of the column loop), K 1 / 2 / 8.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import decode_step_cases as dc
import moe_cases as mc
from conftest import load_golden
from oracle.linear import moe_route, swiglu
from oracle.numerics import round_to_dtype, seeded_normal

pytestmark = pytest.mark.gpu
DEV = "cuda"
# what pli_last_route reports for each kernel family
LAUNCH_NAME = {"gemm_grouped_nt": "pli_gemm_grouped", "gemm_grouped_lds_nt": "gemm_grouped_lds_nt",
               "gemm_256g": "gemm_256g"}


@pytest.mark.parametrize("T,E,k", [(1, 8, 2), (37, 8, 2), (256, 16, 4), (5, 64, 8)])
def test_moe_route_vs_oracle(T, E, k):
    import pli_hip
    logits = torch.from_numpy(seeded_normal((T, E), T * E)).cuda()
    w, idx, pos, gather, offsets = pli_hip.moe_route(logits, k)
    rw, ridx = moe_route(logits.double().cpu().numpy(), k)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_allclose(w.cpu().numpy(), rw, rtol=1e-5, atol=1e-6)
    off = offsets.cpu().numpy()
    counts = np.bincount(ridx.ravel(), minlength=E)
    np.testing.assert_array_equal(np.diff(off), counts)
    p, gth = pos.cpu().numpy(), gather.cpu().numpy()[:T * k]
    assert sorted(p.ravel().tolist()) == list(range(T * k))          # a permutation
    for t in range(T):
        for j in range(k):
            e = ridx[t, j]
            assert off[e] <= p[t, j] < off[e + 1] and gth[p[t, j]] == t


@pytest.mark.parametrize("variant", [None, 1, 2])
@pytest.mark.parametrize("T,E,k,H,I,dead", [
    (4, 8, 2, 256, 512, ()),         # decode sizes: weight-streaming grouped kernel
    (24, 8, 2, 256, 512, ()),        # 48 rows: the LDS-staged grouped kernel (default)
    (64, 8, 2, 512, 1024, ()),       # 16 rows / expert: LDS kernel (default) / phased 256-row tile (1)
    (300, 8, 2, 256, 256, ()),       # 600 rows: experts span several 128-row slabs
    (1200, 4, 2, 384, 640, ()),      # ~600 rows / expert = 3 slots each; ragged n on both GEMMs
    (600, 16, 1, 256, 512, (3, 7, 11)),  # experts with no rows: their slots / slabs are skipped
])
def test_grouped_gemm_and_combine_vs_oracle(T, E, k, H, I, dead, variant):
    import pli_hip
    x = torch.from_numpy(seeded_normal((T, H), 1, "bf16")).cuda().bfloat16()
    logits = torch.from_numpy(seeded_normal((T, E), 2)).cuda()
    for e in dead:
        logits[:, e] -= 100.0
    ws = [[torch.from_numpy(seeded_normal(s, 10 * e + i, "bf16") * s[1] ** -0.5).cuda().bfloat16()
           for i, s in enumerate(((I, H), (H, I), (I, H)))] for e in range(E)]
    w, idx, pos, gather, offsets = pli_hip.moe_route(logits, k)
    t1 = pli_hip.weight_table([e[0] for e in ws])
    t2 = pli_hip.weight_table([e[1] for e in ws])
    t3 = pli_hip.weight_table([e[2] for e in ws])
    h = pli_hip.gemm_grouped(x, gather, t1, offsets, T * k, I, H, H, wu_table=t3, variant=variant)
    y = pli_hip.gemm_grouped(h, None, t2, offsets, T * k, H, I, I, variant=variant)
    out = pli_hip.moe_combine(y, pos, w, T)
    # per-row check of the grouped SwiGLU against the oracle
    xn, gth = x.double().cpu().numpy(), gather.cpu().numpy()
    off = offsets.cpu().numpy()
    hn = h.double().cpu().numpy()
    for e in range(E):
        rows = range(off[e], off[e + 1])
        if not len(rows):
            continue
        ref = swiglu(xn[gth[list(rows)]], ws[e][0].double().cpu().numpy(), ws[e][2].double().cpu().numpy())
        assert np.abs(hn[list(rows)] - ref).max() <= 1e-2 * (np.abs(ref).max() + 1)
    # end to end vs the f64 layer with the same routing
    if dead:
        assert all(off[e] == off[e + 1] for e in dead)
    rw, ridx = moe_route(logits.double().cpu().numpy(), k)
    exp = np.zeros((T, H))
    for t in range(T):
        for j in range(k):
            e = ridx[t, j]
            hh = swiglu(xn[t:t + 1], ws[e][0].double().cpu().numpy(), ws[e][2].double().cpu().numpy())
            exp[t] += rw[t, j] * (hh @ ws[e][1].double().cpu().numpy().T)[0]
    got = out.double().cpu().numpy()
    assert np.abs(got - exp).max() <= 2e-2 * (np.abs(exp).max() + 1)


def test_moe_layer_gpu_matches_reference():
    from ch09 import MoEConfig, MoELayer
    g = load_golden("moe.npz")
    cfg = MoEConfig(hidden_dim=256, expert_dim=512, num_experts=8, num_experts_per_tok=2)
    torch.manual_seed(9)
    moe = MoELayer(cfg).cuda()
    x = torch.from_numpy(seeded_normal((2, 8, 256), 61)).cuda()
    with torch.no_grad():
        y32 = moe(x).cpu().numpy()                      # fp32: dense HIP path
        yb = moe.bfloat16()(x.bfloat16()).float().cpu().numpy()  # bf16: grouped path
    np.testing.assert_allclose(y32, g["y"], rtol=1e-3, atol=1e-4)
    rel = np.linalg.norm(yb - g["y"]) / np.linalg.norm(g["y"])
    assert rel < 2e-2, rel


# ------------------------------------------------- grouped GEMM per element
def _launch_grouped(x, gather, w, wu, offsets, rows, n, k, variant, padded, dt, route):
    """one pli_gemm_grouped call into a Guarded [rows + 3, n] (ldc = n + 8 when padded); checks the kernel family
    pli_last_route names and waits, so the operands the pointer table names outlive the launch"""
    import pli_hip
    out = dc.Guarded((rows + 3, n), dt, DEV, strides=(n + (8 if padded else 0), 1))
    assert len({t.stride(0) for t in w + (wu or [])}) == 1
    pli_hip.gemm_grouped(x, gather, pli_hip.weight_table(w), offsets, rows, n, k, w[0].stride(0),
                         wu_table=pli_hip.weight_table(wu) if wu else None, out=out.view, variant=variant)
    assert pli_hip.last_route() == LAUNCH_NAME[route.split("<")[0]], (route, pli_hip.last_route())
    torch.cuda.synchronize()
    return out


def _run_grouped(c, dt):
    op = mc.grouped_operands(c, dt)
    d = mc.grouped_device(c, op, dt, DEV)
    assert (d.x.stride(0) > c.k) == c.padded and (d.gather is None) == (not c.use_gather)
    out = _launch_grouped(d.x, d.gather, d.w, d.wu, d.offsets, mc.rows_bound(c), c.n, c.k, c.variant, c.padded, dt,
                          c.route)
    return op, out


def _check_rows(out, ref, dt, what):
    """rows [0, len(ref)) per element; the spare rows, the row padding and the guards untouched"""
    rows = ref.shape[0]
    got = dc.f64(out.view[:rows])
    nonfinite = int((~np.isfinite(got)).sum())
    assert nonfinite == 0, f"{what}: {nonfinite} non-finite outputs (a NaN operand was read)"
    ratio = dc.lin_ratio(got, ref, dt)
    print(f"{what}: {rows} rows, err / bound {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)
    dc.assert_untouched(out, lambda v: v[:rows], what=what)


@pytest.mark.parametrize("dt", dc.DTYPES)
@pytest.mark.parametrize("c", mc.GROUPED_CASES, ids=mc.grouped_id)
def test_grouped_gemm_per_element(c, dt):
    op, out = _run_grouped(c, dt)
    _check_rows(out, mc.grouped_reference(op), dt, f"{mc.grouped_id(c)} {dt}")


@pytest.mark.parametrize("dt", dc.DTYPES)
@pytest.mark.parametrize("c", mc.AGREEMENT_CASES, ids=mc.grouped_id)
def test_grouped_routes_each_meet_the_oracle(c, dt):
    """one shape under variant None / 1 / 2 (two different kernels): each is held to the oracle on its own"""
    op, out = _run_grouped(c, dt)
    _check_rows(out, mc.grouped_reference(op), dt, f"{mc.grouped_id(c)} {dt}")


@pytest.mark.parametrize("dt", dc.DTYPES)
@pytest.mark.parametrize("sw", [False, True], ids=["plain", "swiglu"])
def test_grouped_gemm_with_more_experts_than_grid_z(sw, dt):
    """E = 65536, rows only in experts 0, 40000 and 65535 (5, 9, 6): the LDS-staged kernel would need blockIdx.z =
    65535 + 1, so the dispatch takes the weight-streaming kernel.  Every empty expert's table entry names one NaN
    weight; the output is held per element like the other grouped cases."""
    import pli_hip
    E, n, k, live = 65536, 128, 128, {0: 5, 40000: 9, 65535: 6}
    rows = sum(live.values())
    assert mc.grouped_route(E, rows, n, sw, None) == f"gemm_grouped_nt<NBG2,SW{int(sw)}>"
    seed = 4000 + (500 if dt == "fp16" else 0) + int(sw)
    tokens = max(live.values()) + 3
    compact, gather = mc.synthetic_routing(list(live.values()), tokens, seed)
    x = round_to_dtype(seeded_normal((tokens, k), seed + 1), dt)
    used = np.zeros(tokens, bool)
    used[gather] = True
    x[~used] = np.nan
    wgt = lambda s: round_to_dtype(seeded_normal((n, k), s) * np.float32(k ** -0.5), dt)  # noqa: E731
    w = [wgt(seed + 10 + i) for i in range(3)]
    wu = [wgt(seed + 110 + i) for i in range(3)] if sw else None
    op = mc.GroupedOperands(x, w, wu, gather, compact, tokens)
    counts = np.zeros(E, np.int64)
    counts[list(live)] = list(live.values())
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(DEV)

    def table(ws):
        dead = dc.weight_view(np.full((n, k), np.nan, np.float32), dt, DEV, True)
        held = [dc.weight_view(a, dt, DEV, True) for a in ws]
        t = torch.full((E,), dead.data_ptr(), dtype=torch.int64)
        t[list(live)] = torch.tensor([h.data_ptr() for h in held], dtype=torch.int64)
        return t.to(DEV), held + [dead]

    wt, keep = table(w)
    wut, keep_u = table(wu) if sw else (None, None)
    out = dc.Guarded((rows + 3, n), dt, DEV, strides=(n + 8, 1))
    pli_hip.gemm_grouped(dc.row_view(x, dt, DEV, 8), torch.from_numpy(gather).to(DEV), wt, offsets, rows, n, k,
                         keep[0].stride(0), wu_table=wut, out=out.view)
    assert pli_hip.last_route() == LAUNCH_NAME["gemm_grouped_nt"], pli_hip.last_route()
    torch.cuda.synchronize()
    _check_rows(out, mc.grouped_reference(op), dt, f"E65536 {'swiglu' if sw else 'plain'} {dt}")


def _combine_checked(y, pos, w, T, K, H, padded, dt, what):
    """pli_moe_combine of y (a [R, H] view) into a Guarded [T, H] (ldo = H + 8 when padded) against float64 on the
    stored y"""
    import pli_hip
    out = dc.Guarded((T, H), dt, DEV, strides=(H + (8 if padded else 0), 1))
    pli_hip.moe_combine(y, torch.from_numpy(pos).to(DEV), torch.from_numpy(w).to(DEV), T, out=out.view)
    torch.cuda.synchronize()
    ref, mag = mc.combine_reference(dc.f64(y), pos, w)
    ratio = mc.combine_ratio(dc.f64(out.view), ref, mag, K, dt)
    print(f"{what}: err / bound {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)
    dc.assert_untouched(out, lambda v: v, what=what)


@pytest.mark.parametrize("dt", dc.DTYPES)
@pytest.mark.parametrize("c1,n2", mc.CHAIN_CASES, ids=lambda v: mc.grouped_id(v) if isinstance(v, tuple) else f"n2_{v}")
def test_two_stage_chain_per_element(c1, n2, dt):
    """h = silu(x W1^T) * (x W3^T), then W2 over the stored h, then the combine over the stored y"""
    op, h = _run_grouped(c1, dt)
    rows = mc.rows_bound(c1)
    what = f"{mc.grouped_id(c1)} {dt}"
    _check_rows(h, mc.grouped_reference(op), dt, what + " h")
    seed = mc.grouped_seed(c1, dt) + 700
    w2 = [round_to_dtype(seeded_normal((n2, c1.n), seed + e) * np.float32(c1.n ** -0.5), dt) if c1.counts[e] else
          np.full((n2, c1.n), np.nan, np.float32) for e in range(c1.E)]
    hs = h.view[:rows]                                   # the stored h: row stride ldc, already expert-sorted
    route2 = mc.grouped_route(c1.E, rows, n2, False, c1.variant)
    y = _launch_grouped(hs, None, [dc.weight_view(a, dt, DEV, c1.padded) for a in w2], None,
                        torch.from_numpy(op.offsets).to(DEV), rows, n2, c1.n, c1.variant, c1.padded, dt, route2)
    op2 = mc.GroupedOperands(None, w2, None, None, op.offsets, None)
    _check_rows(y, mc.grouped_reference(op2, x_sorted=dc.f64(hs)), dt, f"{what} y ({route2})")
    T, K = 3, 2
    cb = mc.combine_operands(T, K, 8, dt, rows=rows, seed=seed + 50)   # its pos and weights; y is the stored one
    _combine_checked(y.view[:rows], cb.pos, cb.w, T, K, n2, c1.padded, dt, what + " combine")


# ----------------------------------------------------------------- combine
@pytest.mark.parametrize("dt", dc.DTYPES, ids=lambda dt: f"moe_combine_kernel<{'f16' if dt == 'fp16' else dt}>")
@pytest.mark.parametrize("c", mc.COMBINE_CASES, ids=mc.combine_id)
def test_combine_alone_per_element(c, dt):
    op = mc.combine_operands(c.T, c.K, c.H, dt)
    y = dc.row_view(op.y, dt, DEV, 8 if c.padded else 0)
    _combine_checked(y, op.pos, op.w, c.T, c.K, c.H, c.padded, dt, f"{mc.combine_id(c)} {dt}")


# ------------------------------------------------------------------ router
@pytest.mark.parametrize("c", mc.ROUTE_CASES, ids=mc.route_id)
def test_moe_route_c_abi(c):
    import pli_hip
    L = pli_hip.lib()
    T, E, k = c.T, c.E, c.k
    lg = mc.route_logits(c)
    tdt = dc.GUARDED_DT[c.logits_dtype]
    buf = torch.full((T, E + c.ld_pad), float("nan"), dtype=tdt, device=DEV)
    buf[:, :E] = torch.from_numpy(lg).to(tdt)
    assert np.array_equal(buf[:, :E].float().cpu().numpy(), lg)      # the logits are values of the type
    wts = dc.Guarded((T, k), "fp32", DEV)
    idx, pos, gather = mc.GuardedInts(T * k, DEV), mc.GuardedInts(T * k, DEV), mc.GuardedInts(T * k + 5, DEV)
    offsets, ws = mc.GuardedInts(E + 1, DEV), mc.GuardedInts(E + T * k, DEV)
    rc = L.pli_moe_route(buf.data_ptr(), E + c.ld_pad, T, E, k, c.normalize, {"fp32": 0, "fp16": 1, "bf16": 2}[
        c.logits_dtype], wts.view.data_ptr(), idx.view.data_ptr(), pos.view.data_ptr(), gather.view.data_ptr(),
        offsets.view.data_ptr(), ws.view.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.pli_last_error()
    torch.cuda.synchronize()
    rw, ridx = moe_route(lg, k, bool(c.normalize))
    gi = idx.view.cpu().numpy().reshape(T, k)
    np.testing.assert_array_equal(gi, ridx)                          # ties included: the lower index first
    gw = wts.view.cpu().numpy()
    np.testing.assert_allclose(gw, rw, rtol=1e-5, atol=1e-6)
    if c.normalize:
        assert np.abs(gw.astype(np.float64).sum(-1) - 1).max() <= 1e-6
    off = offsets.view.cpu().numpy()
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(ridx.ravel(), minlength=E))]))
    p, gth = pos.view.cpu().numpy().reshape(T, k), gather.view.cpu().numpy()
    assert sorted(p.ravel().tolist()) == list(range(T * k))          # a permutation
    assert (gth[p] == np.arange(T)[:, None]).all()
    assert (off[gi] <= p).all() and (p < off[gi + 1]).all()
    dc.assert_untouched(wts, lambda v: v, what="weights")
    for name, g, written in (("expert_idx", idx, None), ("pos", pos, None), ("gather", gather, T * k),
                             ("offsets", offsets, None), ("workspace", ws, None)):
        bad = g.stray_writes(written)
        assert bad.numel() == 0, f"{name}: written outside its {g.n if written is None else written} elements at " \
                                 f"{bad[:8].tolist()}"
