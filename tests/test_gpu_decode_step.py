"""The kernels under the fused decode step against the float64 oracle:
pli_rms_gemm_nt (rms_linear / rms_swiglu / rms_qkv_into_cache), pli_rmsnorm,
pli_gemm_multi_nt (qkv_into_cache), pli_kv_append and pli_attn_decode_dev.

Inputs are seeded (oracle.numerics.seeded_normal), optionally views of wider
NaN-filled buffers; every output is a view inside a sentinel-filled buffer
with guard rows and everything outside the addressed elements must keep the
sentinel's bits (tests/decode_step_cases.py).

Bounds, all per element:
* h_out: bitwise the torch CPU add a + residual in the storage type.
* fused outputs and qkv_into_cache: |err| <= LIN_TOL * (|ref| + 1), bf16 1e-2,
  fp16 4e-3 (the project's linear bound), ref = float64 on the stored h.  A
  CPU emulation of the kernel's semantics (tests/test_decode_step_emulation_cpu.py)
  over this file's case list reaches these fractions of it:
      linear 0.36 (bf16) / 0.10 (fp16), SwiGLU 0.41 / 0.11, qkv 0.47 / 0.13;
      statistics edges 0.48 / 0.10 (linear), 0.23 / 0.09 (SwiGLU).
  SwiGLU at K = 8 emulated at 0.61 and was replaced by the linear form there.
  The kernels on an MI355X reach the same figures (worst element: linear 0.48 /
  0.10 with the statistics edges, SwiGLU 0.41 / 0.11, qkv 0.47 / 0.13; the
  unfused qkv_into_cache 0.26 / 0.09; y of pli_rmsnorm 0.95 / 0.89 of its
  bound; attn_decode_dev 4.4e-3).
* y of pli_rmsnorm: |err| <= 1.05 * half an ulp * |ref| + the smallest normal
  (half an ulp: 2^-8 bf16, 2^-11 fp16; emulation 0.995 / 0.961 of half an ulp).
* kv_append: an exact copy.  attn_decode_dev: 1e-2 absolute against
  naive_attention, the tolerance of tests/test_gpu_decode.py.

Kernel instances each case group reaches:
* rms_gemm_skinny<T, NB, SW, RPT> (CPL 4 when SW or RPT 1, else 8), T bf16 and
  fp16 each: K 8 / 2048 -> RPT 1; 2056 / 4096 -> RPT 2; 4104 / 6144 / 6152 /
  8184 / 8192 -> RPT 4; M 1 / 2 / 3-4 -> NB 1 / 2 / 4 (M 3: bb < M masked).
  Every (K, M) pair runs; all 9 (NB, RPT) pairs run with SW false (linear or
  qkv form) and all 9 with SW true (SwiGLU: K 2048 at M 1 / 2 / 4, 2056 M 3,
  4096 M 1 / 2, 4104 M 1 / 4, 6144 M 3, 6152 M 2 / 3, 8184 M 1 / 4, 8192 M 3);
  the CPU test asserts that no instance is missing from the list.  K 8 / 2056 /
  4104 / 6152 / 8184 leave the last weight trip partial (clamped loads); the
  CPL 8 loop takes its second trip from K 4104; widths (5, 3, 2) put group
  boundaries inside a workgroup's 4 waves and leave 2 waves inactive, (1,)
  leaves 3.
* m 4, k 8192 (65536 bytes of dynamic LDS + 16 static = 65552 of the 163840 a
  gfx950 workgroup may use): test_fused_m4_k8192.
* rmsnorm_vec<T, RPT> RPT 1 (n 8, 2048), 2 (2056), 4 (4104, 8192), padded
  rows; rmsnorm_generic<T> (n 8200, and a row stride that is no multiple of 8).
* gemm_skinny_multi<T, NB, CPL>: CPL 2 (K 8, 1024), 4 (1032, 2048), 8 (2056,
  4104: second trip partial); NB 1 / 8 / 16 (M 1 / 5, 8 / 9, 16).
* gemm_smallm_nt<T, NBG, MULTI>: NBG 2 (M 17, 32), 4 (33, 64), 8 (65, 128);
  K 128 remainder loop only, 1024 one body step, 1152 body + remainder, 2176
  two body steps + remainder; three groups and two.
* kv_append_kernel: D 8 and 64.  attn_decode_chunk<T, D, 13> D 64 / 128 with
  the device length, 1 and 4 splits (+ attn_decode_combine).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import decode_step_cases as dc
from oracle import attention as oatt
from oracle import linear as olin
from oracle.numerics import seeded_normal

pytestmark = pytest.mark.gpu
DEV = "cuda"
S_MAX = dc.S_MAX


@pytest.fixture(scope="module")
def L():
    import pli_hip
    return pli_hip.lib()


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int16)


def _check_groups(outs, refs, widths, B, S, p0, dt, what):
    """each group's written rows against its float64 reference [B * S, n]; everything else untouched"""
    for gi, (o, ref, n) in enumerate(zip(outs, refs, widths)):
        r0, nr = dc.written_rows(gi, S, p0, o.shape[1])
        got = dc.f64(o.view[:, r0:r0 + nr, :n])
        ratio = dc.lin_ratio(got, ref.reshape(B, S, n)[:, :nr], dt)
        print(f"{what} group {gi}: rows {r0}..{r0 + nr - 1}, err / bound {ratio:.3f}")
        assert ratio <= 1.0, (what, gi, ratio)
        dc.assert_untouched(o, lambda v: v[:, r0:r0 + nr, :n], what=f"{what} group {gi}")


def _run_fused(c, dt, eps=dc.EPS, scale=1.0, op=None):
    """one fused call of case c -> (operands, h Guarded | None, output Guardeds [B, rows, n])"""
    import pli_hip
    op = op or dc.case_operands(c, dt, scale)
    pad = 8 if c.padded else 0
    a = dc.row_view(op.a, dt, DEV, pad)
    r = dc.row_view(op.residual, dt, DEV, pad) if op.residual is not None else None
    g = dc.t16(op.g, dt, DEV)
    w = [dc.weight_view(x, dt, DEV, c.padded) for x in op.w]
    h = dc.Guarded((c.M, c.K), dt, DEV, strides=(c.K + pad, 1)) if "h" in c.res else None
    hv = h.view if h is not None else None
    if c.kind == "qkv":
        pos = torch.tensor([dc.POS[c.pos]], dtype=torch.int32, device=DEV)
        outs = dc.group_outputs(c.B, c.S, c.widths, S_MAX, dt, DEV, c.padded)
        pli_hip.rms_qkv_into_cache(a.unflatten(0, (c.B, c.S)), g, eps, w[0], w[1], w[2], outs[0].view,
                                   outs[1].view.unsqueeze(2), outs[2].view.unsqueeze(2), pos,
                                   residual=r.unflatten(0, (c.B, c.S)) if r is not None else None, h_out=hv)
        return op, h, outs
    n = c.widths[0]
    st = n + (4 if c.padded else 0)
    out = dc.Guarded((c.M, 1, n), dt, DEV, strides=(st, st, 1))
    if c.kind == "linear":
        pli_hip.rms_linear(a, g, eps, w[0], residual=r, h_out=hv, out=out.view[:, 0])
    else:
        wu = dc.weight_view(op.wu[0], dt, DEV, c.padded)
        pli_hip.rms_swiglu(a, g, eps, w[0], wu, residual=r, h_out=hv, out=out.view[:, 0])
    return op, h, [out]


def _check_fused(c, dt, op, h, outs, eps=dc.EPS, check_h=True):
    what = f"{dc.case_id(c)} {dt}"
    if h is not None:
        if check_h:
            assert torch.equal(_bits(h.view), _bits(dc.stored_h(op, dt))), f"{what}: h_out is not the torch add"
        dc.assert_untouched(h, lambda v: v, what=f"{what} h_out")
    refs = dc.reference_fused(op, dt, eps, c.kind == "swiglu")
    _check_groups(outs, refs, c.widths, c.B, c.S, dc.POS[c.pos] if c.pos else 0, dt, what)


@pytest.mark.parametrize("dt", dc.DTYPES)
@pytest.mark.parametrize("case", dc.FUSED_CASES, ids=dc.case_id)
def test_fused_vs_oracle(case, dt):
    """h_out bitwise the torch add (written once whatever the grid, not at all when NULL), the outputs within the
    linear bound of the float64 reference on the stored h, rows past the capacity dropped, nothing else written"""
    op, h, outs = _run_fused(case, dt)
    _check_fused(case, dt, op, h, outs)


@pytest.mark.parametrize("dt", dc.DTYPES)
@pytest.mark.parametrize("case", dc.LDS_CASES, ids=dc.case_id)
def test_fused_m4_k8192(case, dt):
    """the largest accepted shape: 4 rows of 8192 take 65536 bytes of dynamic LDS next to the kernel's 16 static
    ones, past 64 KiB.  A gfx950 workgroup may use 160 KiB and the HIP runtime asks for no opt-in below the
    device's limit, so the launch is accepted and computes the same thing as every other shape."""
    op, h, outs = _run_fused(case, dt)
    _check_fused(case, dt, op, h, outs)


@pytest.mark.parametrize("dt", dc.DTYPES)
@pytest.mark.parametrize("K", [2048, 4104])
@pytest.mark.parametrize("kind", ["linear", "swiglu"])
def test_fused_statistics_edges(kind, K, dt):
    c = dc.FusedCase(kind, K, 2, 2, 1, (10,), False, "res+h", None)
    # eps dominating the mean (rows scaled by 2^-12), and eps = 0 on unit rows
    for scale, eps in ((2.0 ** -12, 1e-6), (1.0, 0.0)):
        op, h, outs = _run_fused(c, dt, eps=eps, scale=scale)
        _check_fused(c, dt, op, h, outs, eps=eps)
    # an all-zero row with eps > 0: exact zeros, the other row unaffected
    op = dc.case_operands(c, dt)
    op.a[0], op.residual[0] = 0, 0
    op, h, outs = _run_fused(c, dt, op=op)
    _check_fused(c, dt, op, h, outs)
    assert (outs[0].view[0] == 0).all()
    # one NaN in row 1 (in the last, partial chunk trip at K 4104): exactly row 1's outputs are NaN
    op = dc.case_operands(c, dt)
    _, _, clean = _run_fused(c, dt, op=op)
    op.a[1, K - 3] = np.nan
    _, h, outs = _run_fused(c, dt, op=op)
    assert torch.isnan(outs[0].view[1]).all()
    assert torch.equal(_bits(outs[0].view[0]), _bits(clean[0].view[0]))
    assert torch.isnan(h.view[1, K - 3]) and torch.isnan(h.view).sum().item() == 1
    dc.assert_untouched(outs[0], lambda v: v, what="NaN run")
    dc.assert_untouched(h, lambda v: v, what="NaN run h_out")


@pytest.mark.parametrize("dt", dc.DTYPES)
@pytest.mark.parametrize("K", [2056, 4096, 6144, 8192])
def test_fused_is_bitwise_the_unfused_launches_at_one_row(K, dt):
    """decode_fused.hip's claim beyond K = 2048: the same reduction and per-lane chunk order as pli_rmsnorm and
    the skinny GEMMs (CPL 8 / 12 / 16), so at one row the results are equal bit for bit"""
    import pli_hip
    op = dc.operands(K, 1, (16, 8, 8), dt, 300 + K, swiglu=True)
    a, r, g = dc.t16(op.a, dt, DEV), dc.t16(op.residual, dt, DEV), dc.t16(op.g, dt, DEV)
    w = [dc.t16(x, dt, DEV) for x in op.w]
    wu = dc.t16(op.wu[0], dt, DEV)
    h_ref, y = pli_hip.rmsnorm(a, g, dc.EPS, residual=r)
    h = torch.empty_like(a)
    out = pli_hip.rms_linear(a, g, dc.EPS, w[0], residual=r, h_out=h)
    assert torch.equal(_bits(h), _bits(h_ref))
    assert torch.equal(_bits(out), _bits(pli_hip.gemm(y, w[0], trans_b=True)))
    assert torch.equal(_bits(pli_hip.rms_swiglu(a, g, dc.EPS, w[0], wu, residual=r)),
                       _bits(pli_hip.gemm_swiglu(y, w[0], wu)))
    if K == 8192:
        return
    pos = torch.tensor([3], dtype=torch.int32, device=DEV)
    got = [torch.zeros(s, dtype=dc.TDT[dt], device=DEV) for s in ((1, 1, 16), (1, S_MAX, 1, 8), (1, S_MAX, 1, 8))]
    ref = [torch.zeros_like(t) for t in got]
    pli_hip.rms_qkv_into_cache(a.view(1, 1, K), g, dc.EPS, *w, *got, pos, residual=r.view(1, 1, K))
    pli_hip.qkv_into_cache(y.view(1, 1, K), *w, *ref, pos)
    for x, z in zip(got, ref):
        assert torch.equal(_bits(x), _bits(z))
    assert got[1][0, 3].abs().sum().item() > 0


# ---------------------------------------------------------------- pli_rmsnorm
NORM_CASES = [  # rows, n, residual, layout: contiguous / rows padded by 8 / a row stride that is no multiple of 8
    (3, 8, True, "contig"),        # one chunk: a single active thread
    (2, 2048, False, "contig"),    # RPT 1, full
    (2, 2056, True, "padded"),     # RPT 2, its second chunk on one thread only
    (3, 4104, False, "padded"),    # RPT 4
    (2, 8192, True, "contig"),     # the last vector size
    (2, 8200, True, "contig"),     # the first generic size for 16-bit storage
    (3, 2056, True, "odd"),        # unaligned rows: the generic kernel
]


@pytest.mark.parametrize("dt", dc.DTYPES)
@pytest.mark.parametrize("rows,n,res,layout", NORM_CASES)
def test_rmsnorm_y_per_element(L, rows, n, res, layout, dt):
    pad = {"contig": 0, "padded": 8, "odd": 3}[layout]
    op = dc.operands(n, rows, (), dt, 900 + n + rows, residual=res)
    x = dc.row_view(op.a, dt, DEV, pad)
    r = dc.row_view(op.residual, dt, DEV, pad) if res else None
    g = dc.t16(op.g, dt, DEV)
    y = dc.Guarded((rows, n), dt, DEV, strides=(n + pad, 1))
    h = dc.Guarded((rows, n), dt, DEV, strides=(n + pad, 1)) if res else None
    rc = dc.call_rmsnorm(L, x, r, g, y.view, h.view if res else None, dc.EPS, dt)
    assert rc == 0, L.pli_last_error()
    assert L.pli_last_route() == (b"rmsnorm_generic" if layout == "odd" or n > 8192 else b"rmsnorm_vec")
    hs = dc.stored_h(op, dt)
    if res:
        assert torch.equal(_bits(h.view), _bits(hs))
        dc.assert_untouched(h, lambda v: v, what="h_out")
    ratio = dc.norm_ratio(dc.f64(y.view), olin.rms_norm(dc.f64(hs), op.g, dc.EPS), dt)
    print(f"rmsnorm rows {rows} n {n} {layout} {dt}: err / bound {ratio:.4f}")
    assert ratio <= 1.0
    dc.assert_untouched(y, lambda v: v, what="y")


# ---------------------------------------------------- pli_gemm_multi_nt (unfused)
def _multi(L, c, dt):
    M = c.B * c.S
    op = dc.operands(c.K, M, c.widths, dt, 5000 + c.K + M, residual=False)
    x = dc.row_view(op.a, dt, DEV, 8 if c.padded else 0)
    w = [dc.weight_view(t, dt, DEV, c.padded) for t in op.w]
    outs = dc.group_outputs(c.B, c.S, c.widths, S_MAX, dt, DEV, c.padded)
    pos = torch.tensor([c.pos], dtype=torch.int32, device=DEV)
    rc = dc.call_multi(L, x, c.S, w, outs, pos, S_MAX, dt)
    assert rc == 0, L.pli_last_error()
    assert L.pli_last_route() == (b"pli_gemm_multi_nt<smallm>" if M > 16 else b"pli_gemm_multi_nt")
    _check_groups(outs, [olin.linear(op.a, t) for t in op.w], c.widths, c.B, c.S, c.pos, dt, f"{dc.multi_id(c)} {dt}")


@pytest.mark.parametrize("dt", dc.DTYPES)
@pytest.mark.parametrize("case", dc.SKINNY_MULTI_CASES, ids=dc.multi_id)
def test_qkv_into_cache_skinny_vs_oracle(L, case, dt):
    _multi(L, case, dt)


@pytest.mark.parametrize("dt", dc.DTYPES)
@pytest.mark.parametrize("case", dc.SMALLM_MULTI_CASES, ids=dc.multi_id)
def test_qkv_into_cache_smallm_vs_oracle(L, case, dt):
    _multi(L, case, dt)


# ------------------------------------------------------------------ pli_kv_append
@pytest.mark.parametrize("dt", dc.DTYPES)
@pytest.mark.parametrize("D", [8, 64])
def test_kv_append_is_an_exact_copy_of_strided_slices(D, dt):
    """k / v taken as slices of one packed [B, T, (H + 2 Hkv) * D] projection output, T spanning the capacity"""
    import pli_hip
    B, T, H, Hkv = 3, 5, 4, 2
    packed = dc.t16(seeded_normal((B, T, (H + 2 * Hkv) * D), 40 + D, dt), dt, DEV)
    kn = packed[..., H * D:(H + Hkv) * D].unflatten(-1, (Hkv, D))
    vn = packed[..., (H + Hkv) * D:].unflatten(-1, (Hkv, D))
    assert not kn.is_contiguous() and kn.stride(1) == (H + 2 * Hkv) * D
    for p0 in (1, S_MAX - 2, S_MAX):  # all rows fit / two of five fit / pos == capacity: nothing written
        st = Hkv * D + 8
        kc, vc = (dc.Guarded((B, S_MAX, Hkv, D), dt, DEV, strides=((S_MAX + 1) * st, st, D, 1)) for _ in range(2))
        pli_hip.kv_append(kn, vn, kc.view, vc.view, torch.tensor([p0], dtype=torch.int32, device=DEV))
        nr = max(0, min(T, S_MAX - p0))
        for cache, new in ((kc, kn), (vc, vn)):
            assert torch.equal(_bits(cache.view[:, p0:p0 + nr]), _bits(new[:, :nr]))
            dc.assert_untouched(cache, lambda v: v[:, p0:p0 + nr], what=f"kv_append pos {p0}")


# ------------------------------------------------------------ pli_attn_decode_dev
ATTN_CASES = [  # n_dev, add, S_max, B, Hkv, G, D, dtype
    (0, 1, 64, 2, 2, 4, 64, "bf16"),        # the first token: one valid key
    (1, 0, 64, 2, 2, 1, 128, "fp16"),       # length already counted, G 1
    (63, 1, 64, 2, 1, 16, 128, "bf16"),     # fills the cache exactly, a full 16-row tile
    (159, 3, 160, 2, 2, 4, 64, "fp16"),     # 162 clamped to the capacity, 3-token causal chunk, 2 splits
    (37, 2, 512, 1, 1, 4, 128, "bf16"),     # 4 splits planned for 512 keys, 39 valid: 3 chunks exit empty
    (37, 2, 64, 2, 2, 1, 64, "fp16"),
    (300, 1, 512, 1, 2, 16, 64, "fp16"),    # 4 splits, the third ragged, the fourth empty
    (7, 1, 16, 3, 1, 4, 128, "bf16"),       # capacity below one 128-key chunk
]


@pytest.mark.parametrize("n_dev,add,s_max,B,Hkv,G,D,dt", ATTN_CASES)
def test_attn_decode_dev_vs_oracle(n_dev, add, s_max, B, Hkv, G, D, dt):
    import pli_hip
    Sq, H = max(add, 1), Hkv * G
    n = min(n_dev + add, s_max)
    seed = 7000 + n_dev + 10 * add + D
    q = seeded_normal((B, Sq, H, D), seed, dt)
    kc = seeded_normal((B, s_max, Hkv, D), seed + 1, dt)
    vc = seeded_normal((B, s_max, Hkv, D), seed + 2, dt)
    kc[:, n:], vc[:, n:] = 300.0, 1e4  # stale rows at and past the valid length must not leak in
    out = dc.Guarded((B, Sq, H, D), dt, DEV)
    pli_hip.attn_decode_dev(dc.t16(q, dt, DEV), dc.t16(kc, dt, DEV), dc.t16(vc, dt, DEV),
                            torch.tensor([n_dev], dtype=torch.int32, device=DEV), n_kv_add=add, causal=Sq > 1,
                            out=out.view)
    ref = oatt.naive_attention(q.transpose(0, 2, 1, 3), kc[:, :n].transpose(0, 2, 1, 3),
                               vc[:, :n].transpose(0, 2, 1, 3), causal=Sq > 1)
    got = dc.f64(out.view).transpose(0, 2, 1, 3)
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max()
    print(f"attn_decode_dev n {n} of {s_max}: max |err| {err:.3e}")
    assert err <= 1e-2
    dc.assert_untouched(out, lambda v: v, what="attn_decode_dev out")
