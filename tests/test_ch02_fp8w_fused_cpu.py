"""ch02.Fp8WeightModel.from_model(..., fused_decode=True) on the CPU: the switch
selects device launches only, so a CPU model gives the same logits with and
without it, and the default is off."""
from __future__ import annotations

import inspect

import torch


def _models(dtype):
    from ch02 import CachedTransformerModel, Fp8WeightModel
    torch.manual_seed(21)
    model = CachedTransformerModel(1000, 64, 2, 4, 2, 128).to(dtype).eval()
    return Fp8WeightModel.from_model(model), Fp8WeightModel.from_model(model, fused_decode=True)


def test_default_is_unfused():
    from ch02 import Fp8WeightModel
    sig = inspect.signature(Fp8WeightModel.from_model)
    assert list(sig.parameters) == ["model", "pow2_scales", "fused_decode"]
    assert sig.parameters["pow2_scales"].default is False and sig.parameters["fused_decode"].default is False
    plain, fused = _models(torch.float32)
    assert plain.fused_decode is False and fused.fused_decode is True


def test_cpu_logits_do_not_depend_on_the_switch():
    for dtype in (torch.float32, torch.bfloat16):
        plain, fused = _models(dtype)
        for a, b in zip(plain.linears(), fused.linears()):
            assert torch.equal(a.codes.view(torch.uint8), b.codes.view(torch.uint8)) and torch.equal(a.scale, b.scale)
        ids = torch.randint(0, 1000, (2, 7), generator=torch.Generator().manual_seed(3))
        with torch.no_grad():
            ca = plain.create_caches(2, 16, torch.device("cpu"), dtype)
            cb = fused.create_caches(2, 16, torch.device("cpu"), dtype)
            a, b = plain(ids, ca, 0), fused(ids, cb, 0)
            assert torch.equal(a, b)
            for step in range(3):  # decode steps: one token per sequence, the shape the device switch acts on
                tok = a[:, -1].argmax(-1, keepdim=True)
                a, b = plain(tok, ca, 7 + step), fused(tok, cb, 7 + step)
                assert a.shape == (2, 1, 1000) and torch.equal(a, b), step
            assert torch.equal(plain(ids), fused(ids))  # no caches
