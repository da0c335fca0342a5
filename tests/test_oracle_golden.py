"""Pin the CPU oracle to the reference's own outputs (golden fixtures).

The fixtures were produced by running the reference (tests/golden/make_golden.py);
every oracle function used as a checker elsewhere is held to them here.
"""
from __future__ import annotations

import glob
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from oracle import attention as oatt
from oracle.numerics import (array_hash, bf16_bits, bf16_from_bits, round_to_bf16,
                             seeded_normal)

FLASH_FILES = sorted(glob.glob(os.path.join(GOLDEN, "flash_*.npz")))
TDT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def flash_case(path):
    g = load_golden(os.path.basename(path))
    B, H, N, D = (int(x) for x in g["shape"])
    dt, seed = str(g["dtype"]), int(g["seed"])
    q, k, v = (seeded_normal((B, H, N, D), seed * 10 + i, dt) for i in range(3))
    return g, dt, (q, k, v)


def ref_flash_values(g, dt):
    x = g["ref_flash"]
    if dt == "bf16":
        return bf16_from_bits(x)
    return x.astype(np.float32)


def test_bf16_rounding_matches_torch():
    x = np.random.RandomState(0).standard_normal(10000).astype(np.float32) * 100
    x[:4] = [np.inf, -np.inf, 0.0, -0.0]
    ours = round_to_bf16(x)
    theirs = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    np.testing.assert_array_equal(ours, theirs)
    np.testing.assert_array_equal(bf16_from_bits(bf16_bits(x)), ours)


@pytest.mark.parametrize("path", FLASH_FILES, ids=os.path.basename)
def test_inputs_regenerate_bit_exact(path):
    g, dt, (q, k, v) = flash_case(path)
    assert array_hash(q) == str(g["hash_q"])
    assert array_hash(k) == str(g["hash_k"])
    assert array_hash(v) == str(g["hash_v"])


@pytest.mark.parametrize("path", FLASH_FILES, ids=os.path.basename)
def test_oracle_naive_matches_reference_f64(path):
    """oracle.naive_attention (numpy f64) == reference naive_attention in f64."""
    g, dt, (q, k, v) = flash_case(path)
    ours = oatt.naive_attention(q, k, v)
    np.testing.assert_allclose(ours, g["ref_naive_f64"].astype(np.float64), rtol=2e-6, atol=2e-6)


# Host-BLAS summation order (AVX2 / AVX-512, AMD / Intel hosts) moves the last
# bit of the tile loop's matmuls, so the fixture (made on another host) is held
# to ~2 ulp of the dtype; the live reference on THIS host is held bit-exact.
FIXTURE_ATOL = {"fp32": 2e-6, "fp16": 1e-3, "bf16": 4e-3}


@pytest.mark.parametrize("path", FLASH_FILES, ids=os.path.basename)
def test_tile_loop_restatement_matches_fixture(path):
    """oracle.flash_tile_loop_torch reproduces the reference tile loop's
    recorded output (same torch ops in the same order and dtype)."""
    g, dt, (q, k, v) = flash_case(path)
    tq, tk, tv = (torch.from_numpy(a).to(TDT[dt]) for a in (q, k, v))
    ours = oatt.flash_tile_loop_torch(tq, tk, tv).float().numpy()
    np.testing.assert_allclose(ours, ref_flash_values(g, dt), rtol=0, atol=FIXTURE_ATOL[dt])


REF_FLASH = os.path.join(os.environ.get("PLI_REFERENCE", "/root/reference"), "ch06", "flash_attention.py")


@pytest.mark.skipif(not os.path.exists(REF_FLASH), reason="reference checkout absent (GPU box)")
@pytest.mark.parametrize("path", FLASH_FILES, ids=os.path.basename)
def test_tile_loop_restatement_is_bit_exact_vs_live_reference(path):
    """Same host, same inputs: the restatement equals the reference's own
    flash_attention_forward bit for bit (checker validation only)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_ref_ch06_flash", REF_FLASH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g, dt, (q, k, v) = flash_case(path)
    tq, tk, tv = (torch.from_numpy(a).to(TDT[dt]) for a in (q, k, v))
    ours = oatt.flash_tile_loop_torch(tq, tk, tv).float().numpy()
    np.testing.assert_array_equal(ours, mod.flash_attention_forward(tq, tk, tv).float().numpy())


def test_reference_bf16_error_budget():
    """The reference's own bf16 output sits ~1e-2 from exact (bf16 statistics):
    the fixtures record it so the HIP tolerance is set against the f64 oracle."""
    g, dt, _ = flash_case(os.path.join(GOLDEN, "flash_b1h2n256d128_bf16.npz"))
    err = np.abs(ref_flash_values(g, dt) - g["ref_naive_f64"]).max()
    assert 1e-3 < err < 2e-2


def test_online_softmax_oracle():
    g = load_golden("softmax.npz")
    x1 = np.array([1.0, 2.0, 3.0, 4.0, 5.0], dtype=np.float32)
    x2 = np.array([1000.0, 1001.0, 1002.0], dtype=np.float32)
    x3 = seeded_normal((4, 8, 64), 21)
    assert array_hash(x3) == str(g["hash_x3"])
    for key, x in (("x1", x1), ("x2", x2), ("x3", x3)):
        np.testing.assert_allclose(oatt.online_softmax(x), g[f"{key}_online"], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(oatt.standard_softmax(x), g[f"{key}_standard"], rtol=1e-12, atol=1e-14)
    x4, v4 = seeded_normal((2, 4, 32), 22), seeded_normal((2, 4, 32, 16), 23)
    o, d = oatt.online_softmax_with_output(x4, v4)
    np.testing.assert_allclose(o, g["x4_o"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(d, g["x4_d"], rtol=1e-10, atol=1e-12)


def test_mha_oracle_matches_reference():
    """oracle.multi_head_attention (f64) vs the reference module's fp32 output,
    with weights rebuilt under the same seed by this build's MultiHeadAttention."""
    from ch01 import MultiHeadAttention
    g = load_golden("mha.npz")
    torch.manual_seed(0)
    mha = MultiHeadAttention(512, 8)
    names = [n for n, _ in mha.named_parameters()]
    assert names == [str(s) for s in g["param_order"]]
    for n, p in mha.named_parameters():
        assert array_hash(p.detach().numpy()) == str(g[f"hash_{n}"]), n
    x = seeded_normal((1, 128, 512), 31)
    w = [getattr(mha, f"{c}_proj").weight.detach().numpy() for c in "qkvo"]
    for causal, key in ((True, "y_causal"), (False, "y_noncausal")):
        y = oatt.multi_head_attention(x, *w, num_heads=8, causal=causal)
        np.testing.assert_allclose(y, g[key], rtol=1e-4, atol=1e-5)


def test_analytic_fixture_is_loadable():
    with open(os.path.join(GOLDEN, "analytic.json")) as f:
        a = json.load(f)
    assert {"gemm", "gemv", "roofline", "attn", "comm", "tp"} <= set(a)


def test_stress_fixture_matches_inputs():
    """stress_flash.npz (the reference's bf16 flash on tests/stress_cases.py
    inputs): its recorded error equals the recomputed |out - f64 oracle|."""
    from stress_cases import STRESS, stress_inputs
    g = load_golden("stress_flash.npz")
    for name in STRESS:
        assert np.isfinite(float(g[f"{name}_ref_err"])) and float(g[f"{name}_ref_err"]) > 0
        if f"{name}_ref_flash" not in g:  # large seam cases: error only (fixture size)
            continue
        q, k, v = stress_inputs(name)
        ref = oatt.naive_attention(q, k, v)
        out = bf16_from_bits(g[f"{name}_ref_flash"]).astype(np.float64)
        assert np.isclose(np.abs(out - ref).max(), float(g[f"{name}_ref_err"]), rtol=1e-9, atol=0)


def test_rms_linear_and_rms_swiglu_oracles_match_torch_f64():
    """oracle.linear.rms_linear / rms_swiglu against a direct torch float64
    evaluation of RMSNorm.forward (x / sqrt(mean(x^2) + eps) * weight) followed
    by F.linear (and F.silu(gate) * up), with and without the residual add."""
    import torch.nn.functional as F
    from oracle import linear as olin
    k, n = 72, 5
    x, r = seeded_normal((3, k), 41).astype(np.float64), seeded_normal((3, k), 42).astype(np.float64)
    g = 1 + 0.1 * seeded_normal((k,), 43).astype(np.float64)
    w, wu = (seeded_normal((n, k), 44 + i).astype(np.float64) * k ** -0.5 for i in range(2))
    tw, twu, tg = torch.from_numpy(w), torch.from_numpy(wu), torch.from_numpy(g)
    for eps in (1e-6, 0.0, 0.5):
        for res in (None, r):
            h = torch.from_numpy(x if res is None else x + res)
            y = h / torch.sqrt(torch.mean(h ** 2, dim=-1, keepdim=True) + eps) * tg
            np.testing.assert_allclose(olin.rms_linear(x, g, eps, w, residual=res), F.linear(y, tw).numpy(),
                                       rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(olin.rms_swiglu(x, g, eps, w, wu, residual=res),
                                       (F.silu(F.linear(y, tw)) * F.linear(y, twu)).numpy(), rtol=1e-12, atol=1e-14)
