"""The replay and the bounds of tests/gemm_cases.py without a GPU, over the GPU
test's own case list.

* Every case's kernel and instance equal the replay of the dispatch (asserted
  when gemm_cases is imported; restated here so a failure names the case), the
  set of template instances in the list equals the set the launchers can
  instantiate, and pli_gemm_workspace_size equals the replay's.
* A CPU emulation of the semantics -- fp32 products and sums of the rounded
  inputs, the split routes as ks ordered fp32 partials summed in plane order, the
  bias added in fp32, one rounding to the output type -- is held to 0.5 of the
  fp32 bracket of (b) before the rounding and to 1.0 of (b) after it.  It is not
  the kernels' summation order; it shows that a correct fp32 evaluation leaves
  room inside the bound the kernels are held to.

The device cases (the persistent gemm_w5 walk and gemm_f32_mfma's four-wave
form, 256 CUs here) have millions of outputs: the emulation samples 64 of
their rows (1.5 % to 3 % of M), the GPU test checks every element.

Measured over the list: the chain takes at most 0.07
(bf16 inputs), 0.13 (fp16) and 0.26 (fp32) of the bracket; the rounded value up
to 0.95 (bf16), 0.92 (fp16) and 0.24 (fp32) of (b) -- a correct rounding alone
uses up to 1 / 1.05 of its first term -- and at most 0.39, 0.12 and 0.04 of (a).
"""
from __future__ import annotations

import numpy as np
import pytest

import gemm_cases as gc

_id = lambda v: gc.case_id(v) if isinstance(v, tuple) else v  # noqa: E731
PAIRS = [(c, dt) for c in gc.ALL_CASES for dt in c.dts]
DEVICE_PAIRS = [(c, dt) for c in gc.device_cases(256) for dt in c.dts]


def test_every_case_reaches_the_instance_it_names():
    for family, padded in ((gc.ALL_CASES + gc.device_cases(256), True), (gc.CONTIG_CASES, False)):
        for c in family:
            for dt in c.dts:
                r = gc.case_route(c, dt, padded)
                assert (r.kernel, r.inst) == (c.kernel, c.inst), (gc.case_id(c), dt, padded, r)
    for cus in (8, 64, 256, 304):                       # the device cases follow the CU count
        for c in gc.device_cases(cus):
            for dt in c.dts:
                r = gc.case_route(c, dt, True, cus)
                assert (r.kernel, r.inst) == (c.kernel, c.inst), (cus, gc.case_id(c), r)


def test_the_case_list_covers_every_instance_the_launchers_can_make():
    want, have = gc.launchable_instances(), gc.covered_instances()
    assert want - have == set(), sorted(want - have, key=str)
    assert have - want == set(), sorted(have - want, key=str)
    assert {(c.api, c.kernel) for c in gc.ALL_CASES if c.kind == "large"} == {(c.api, c.kernel) for c in gc.ALL_CASES}


def test_forced_variants_that_fall_through_are_not_counted():
    """what the earlier tests could not see: the replay names the kernel a forced variant really reaches"""
    r = lambda *a, **kw: gc.gemm_route(*a, **kw).kernel  # noqa: E731
    assert r(100, 288, 4160, "bf16", True, False, 20, 0) == gc.G256                     # variant 20, K % 256 != 0
    assert r(100, 288, 4104, "bf16", True, False, 20, 0) == gc.MFMA
    assert r(100, 288, 4096, "bf16", True, False, 20, 0) == gc.MIDM
    assert r(64, 64, 4096, "bf16", True, False, 22, 0) == gc.SMALLM                     # no workspace: no split-K
    assert r(64, 64, 4096, "bf16", True, False, 22, True) == gc.SPLIT_D + "+" + gc.REDUCE
    assert gc.gemm_route(512, 512, 128, "bf16", True, False, 43, 0).inst == "w5 persistent1"   # 4 tiles: no walk
    assert gc.gemm_route(512, 512, 64, "bf16", True, False, 43, 0).inst == "w5 tile"
    assert r(300, 520, 128, "bf16", True, False, 43, 0) == gc.G256                      # M, N % 256 != 0: variant >= 2
    assert r(1, 64, 64, "bf16", True, False, None, 0) == gc.GEMV_VEC and r(1, 64, 64, "bf16", True, True, None, 0) == gc.SKINNY
    # the default's 256-tile choices need gemm_w5 refused: a leading dimension of 2^22 elements
    big = dict(lds=(1 << 22, 1 << 22, 4096))
    assert gc.gemm_route(4096, 4096, 1024, "bf16", True, False, None, 0, **big).inst == "256 g4"
    assert gc.gemm_route(4096, 4096, 8192, "bf16", True, False, None, 0, **big).inst == "256p SCHED7 g4"
    assert gc.gemm_route(4096, 4096, 1024, "bf16", False, False, None, 0, lds=(1024, 1 << 24, 4096)).inst == "256p SCHED7 g4"
    assert r(4096, 4096, 1024, "bf16", True, False, None, 0) == gc.W5


def test_workspace_size_equals_the_replay(built_lib):
    import pli_hip
    L = pli_hip.lib()
    for c in gc.GEMM_CASES + [c for c in gc.device_cases(256) if c.api == "gemm"]:
        for dt in c.dts:
            got = L.pli_gemm_workspace_size(c.m, c.n, c.k, int(c.trans_b), gc.DTYPE_CODE[dt])
            assert got == gc.workspace_size(c.m, c.n, c.k, c.trans_b, dt), (gc.case_id(c), dt)
    size = lambda m, n, k, tb=1, dt=2: L.pli_gemm_workspace_size(m, n, k, tb, dt)  # noqa: E731
    ks_of = lambda m, n, k: size(m, n, k) // (m * n * 4)  # noqa: E731
    assert [ks_of(m, 64, 1024) for m in (16, 17, 256, 257, 2048, 2049)] == [0, 4, 4, 4, 4, 0]
    assert [ks_of(64, n, 1024) for n in (32, 40, 48, 64)] == [4, 0, 0, 4]
    assert [ks_of(64, 64, k) for k in (64, 256, 448, 512, 960, 1024, 2048)] == [0, 0, 0, 2, 0, 4, 8]   # ks 1: no planes
    # the 512-workgroup target: tiles * ks <= 512
    assert ks_of(2048, 4096, 1 << 16) == 0 and ks_of(1024, 4096, 1 << 16) == 2 and ks_of(128, 128, 1 << 20) == 512
    assert size(64, 64, 1024, 0) == 0 and size(64, 64, 1024, 1, 0) == 0 and size(64, 64, 1024, 1, 5) == 0
    for bad in ((0, 64, 1024), (64, 0, 1024), (64, 64, 0), (-1, 64, 1024)):
        assert size(*bad) == 0


def _emulated(c, dt, rows=None):
    op, ref = gc.case_reference(c, dt)
    ks = gc.split_ks(c)
    chain = gc.chain_ratio(gc.emulate_f32(op, c.trans_b, ks, rows), ref, rows)
    got = gc.emulate(op, gc.out_dtype(c, dt), c.trans_b, ks, rows)
    sub = ref if rows is None else gc.Reference(ref.c[rows], ref.bracket[rows], ref.k)
    ra, rb = gc.ratios(got, c, sub, dt)
    print(f"{gc.case_id(c)} {dt}: chain / bracket {chain:.3f}, rounded / (b) {rb:.3f}, rounded / (a) {ra:.3f}")
    assert chain <= 0.5, (gc.case_id(c), dt, chain)
    assert rb <= 1.0 and ra <= 1.0, (gc.case_id(c), dt, ra, rb, gc.worst(got, c, sub, dt))


@pytest.mark.parametrize("c,dt", PAIRS, ids=_id)
def test_emulated_gemm_sits_inside_both_bounds(c, dt):
    _emulated(c, dt)


@pytest.mark.parametrize("c,dt", DEVICE_PAIRS, ids=_id)
def test_emulated_device_cases_on_sampled_rows(c, dt):
    """64 of the rows (of 4352 / 2048 at 256 CUs: 1.5 % / 3 %)"""
    rows = np.sort(np.random.default_rng(7).choice(c.m, 64, replace=False))
    _emulated(c, dt, rows)


def test_bound_b_is_the_tighter_one_at_small_k_and_the_looser_at_large():
    """(b) / (a) per element on default operands (|ref| ~ 0.5): below 1 / 10 at K = 8, above 1 at K = 8192 (why
    both are asserted)"""
    for k, lo, hi in ((8, 0, 1 / 10), (8192, 1, 4)):
        c = next(c for c in gc.GEMM_CASES if (c.m, c.k) == (2, k) and c.kind == "default" and c.kernel == gc.SKINNY)
        _, ref = gc.case_reference(c, "bf16")
        assert lo < np.median(gc.bound_b(c, ref, "bf16") / gc.bound_a(c, ref, "bf16")) < hi


def test_the_reference_is_the_oracle():
    from oracle.linear import linear
    for c in [c for c in gc.GEMM_CASES if c.trans_b][:6]:
        op, ref = gc.case_reference(c, c.dts[0])
        np.testing.assert_allclose(ref.c, linear(op.a, op.b, op.bias), rtol=1e-15, atol=0)


def test_an_accumulator_rounded_before_the_bias_breaks_b_only():
    """what (b) buys: rounding the fp32 sum to bf16 before the bias add stays inside (a) and leaves (b)"""
    import torch
    c = next(c for c in gc.GEMM_CASES if c.kernel == gc.MIDM and c.bias and c.kind == "default")
    op, ref = gc.case_reference(c, "bf16")
    a, b, bias = (torch.from_numpy(np.array(x, dtype=np.float32)) for x in op)
    got = gc.f64(((a @ b.t()).bfloat16().float() + bias).bfloat16())
    ra, rb = gc.ratios(got, c, ref, "bf16")
    assert ra <= 1.0 < rb, (ra, rb)
    # and a dropped split-K plane of small magnitude: the last eighth of K missing
    c = next(c for c in gc.GEMM_CASES if "ks8" in c.inst and c.kind == "default")
    op, ref = gc.case_reference(c, "bf16")
    a, b = (torch.from_numpy(np.array(x, dtype=np.float32)) for x in op[:2])
    k7 = c.k * 7 // 8
    got = a[:, :k7] @ b[:, :k7].t()
    got = gc.f64((got + torch.from_numpy(np.array(op.bias, dtype=np.float32)) if c.bias else got).bfloat16())
    ra, rb = gc.ratios(got, c, ref, "bf16")
    assert rb > 1.0, (ra, rb)
