"""ch02.Fp8WeightModel's fp8_activations option on the CPU: off (the default) it is bitwise the model without the
option; on, exactly the linears of calls with more than 16 rows take the W8A8 mirror (quantise the rows, fp32 matmul
over the decoded codes, both scales after the sum), and calls of at most 16 rows -- decode steps after such a prefill
among them -- are bitwise the W8A16 model's."""
from __future__ import annotations

import inspect

import pytest
import torch

import fp8a_cases as fc

CFG = dict(vocab_size=64, hidden_dim=64, num_layers=2, num_heads=4, num_kv_heads=2, intermediate_dim=128)


@pytest.fixture(scope="module")
def models(built_lib):
    from ch02 import CachedTransformerModel, Fp8WeightModel
    torch.manual_seed(12)
    model = CachedTransformerModel(**CFG).to(torch.bfloat16).eval()
    return Fp8WeightModel.from_model(model), Fp8WeightModel(model, fp8_activations=False), \
        Fp8WeightModel.from_model(model).with_fp8_activations()


def ids_of(B, S, seed):
    return torch.randint(0, CFG["vocab_size"], (B, S), generator=torch.Generator().manual_seed(seed))


def caches(m, B=2):
    return m.create_caches(B, 24, torch.device("cpu"), torch.bfloat16)


def test_signatures_and_threshold():
    from ch02 import Fp8WeightModel
    from ch02 import fp8_weight_model as fwm
    # from_model keeps its parameter list (tests/test_ch02_fp8w_fused_cpu.py pins it); the option is the
    # constructor's keyword and the with_fp8_activations switch, both off by default
    p = inspect.signature(Fp8WeightModel.__init__).parameters
    assert list(p) == ["self", "model", "pow2_scales", "fused_decode", "fp8_activations"]
    assert p["fp8_activations"].default is False
    p = inspect.signature(Fp8WeightModel.with_fp8_activations).parameters
    assert list(p) == ["self", "on"] and p["on"].default is True
    p = inspect.signature(fwm.Fp8Linear.__call__).parameters
    assert list(p) == ["self", "x", "workspace", "fp8_activations"]
    assert p["workspace"].default is None and p["fp8_activations"].default is False
    assert fwm.FP8A_ROWS == 16 == fc.MIN_M - 1, "the model's row threshold is the W8A8 GEMM's"


def test_off_is_bitwise_the_model_without_the_option(models):
    plain, off, _ = models
    assert off.fp8_activations is False and plain.fp8_activations is False
    ids = ids_of(2, 9, 3)
    with torch.no_grad():
        assert torch.equal(plain(ids), off(ids)), "no caches"
        ca, cb = caches(plain), caches(off)
        a, b = plain(ids, ca, 0), off(ids, cb, 0)
        assert torch.equal(a, b), "prefill"
        for step in range(3):
            tok = a[:, -1].argmax(-1, keepdim=True)
            a, b = plain(tok, ca, 9 + step), off(tok, cb, 9 + step)
            assert torch.equal(a, b), step


def test_on_changes_exactly_the_linears_with_more_than_16_rows(models, monkeypatch):
    from ch02 import fp8_weight_model as fwm
    plain, _, on = models
    calls = []
    real = fwm.linear_fp8a_cpu

    def spy(x, codes, scale):
        calls.append((x.shape[0], tuple(codes.shape)))
        return real(x, codes, scale)

    monkeypatch.setattr(fwm, "linear_fp8a_cpu", spy)
    shapes = [tuple(lin.codes.shape) for lin in on.linears()]
    with torch.no_grad():
        # 16 rows: nothing changes
        ids = ids_of(2, 8, 4)
        assert torch.equal(on(ids), plain(ids)) and calls == []
        # 18 rows: every linear, in the model's order, and the logits move
        ids = ids_of(2, 9, 5)
        ca, cb = caches(on), caches(plain)
        a, b = on(ids, ca, 0), plain(ids, cb, 0)
        assert calls == [(18, s) for s in shapes], calls
        assert bool(torch.isfinite(a.float()).all()) and not torch.equal(a, b)
        rel = float((a.float() - b.float()).norm() / b.float().norm())
        print(f"prefill logits, W8A8 against W8A16 on the CPU: rel. L2 {rel:.3e}")
        # decode steps (2 rows) after that prefill: the W8A16 path, bitwise, given the same cache contents
        calls.clear()
        for x, y in zip(ca, cb):
            y.k.copy_(x.k)
            y.v.copy_(x.v)
        for step in range(3):
            tok = a[:, -1].argmax(-1, keepdim=True)
            a, b = on(tok, ca, 9 + step), plain(tok, cb, 9 + step)
            assert torch.equal(a, b), step
        assert calls == []


def test_the_w8a8_linear_is_the_rule_of_the_header(models, built_lib):
    """quantise the rows as quantize_weight_fp8 does, sum the exact code products in fp32, sum * (x_scale * w_scale),
    one rounding"""
    import pli_hip
    _, _, on = models
    lin = on.layers[0].down
    x = torch.randn(3, 7, lin.in_features, generator=torch.Generator().manual_seed(6)).to(torch.bfloat16)
    got = lin(x, fp8_activations=True)
    assert got.shape == (3, 7, lin.out_features) and got.dtype == torch.bfloat16
    x8, xs = pli_hip.quantize_weight_fp8(x.reshape(21, -1))
    want = ((x8.float() @ lin.codes.float().t()) * (xs[:, None] * lin.scale[None, :])).to(torch.bfloat16)
    assert torch.equal(got.reshape(21, -1), want)
    # 16 rows or fewer: the W8A16 linear, whatever the flag says
    x = x[:2]
    assert torch.equal(lin(x, fp8_activations=True), lin(x))
    # within the case list's bound (a) of the float64 value over the dequantised operands
    ref = (fc.DECODE[x8.view(torch.uint8).numpy()] * xs.double().numpy()[:, None]) @ \
        (fc.DECODE[lin.codes.view(torch.uint8).numpy()] * lin.scale.double().numpy()[:, None]).T
    err = (want.double().numpy() - ref)
    assert bool((abs(err) <= 1e-2 * (abs(ref) + 1)).all())


def test_fp32_activations_are_refused(built_lib):
    import pli_hip
    from ch02 import CachedTransformerModel, Fp8WeightModel
    torch.manual_seed(13)
    on = Fp8WeightModel(CachedTransformerModel(**CFG).eval(), fp8_activations=True)
    with torch.no_grad():
        on(ids_of(2, 8, 1))  # 16 rows: the W8A16 path takes any dtype on the CPU
        with pytest.raises(pli_hip.PliError, match="fp16 or bf16"):
            on(ids_of(2, 9, 1))
