"""ch02.Fp8WeightModel on the CPU: the wrapper over a small fp32 model returns logits torch.equal to a
CachedTransformerModel whose Linear weights were overwritten with the dequantised values, the quantised matrices occupy
n k + 4 n bytes, and no 16-bit (or wider) copy of a quantised weight is reachable from the module."""
from __future__ import annotations

import copy

import pytest
import torch
import torch.nn as nn

CFG = dict(vocab_size=64, hidden_dim=64, num_layers=2, num_heads=4, num_kv_heads=2, intermediate_dim=128)


@pytest.fixture(scope="module")
def models(built_lib):
    import pli_hip
    from ch02 import CachedTransformerModel, Fp8WeightModel
    torch.manual_seed(11)
    model = CachedTransformerModel(**CFG).eval()
    ref = copy.deepcopy(model)
    with torch.no_grad():
        for mod in ref.modules():
            if isinstance(mod, nn.Linear):
                codes, scale = pli_hip.quantize_weight_fp8(mod.weight)
                mod.weight.copy_(codes.float() * scale[:, None])
    return Fp8WeightModel.from_model(model), ref


def test_logits_equal_the_dequantised_model(models):
    fq, ref = models
    ids = torch.randint(0, CFG["vocab_size"], (2, 9), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        assert torch.equal(fq(ids), ref(ids)), "no caches"
        ca, cb = (m.create_caches(2, 16, torch.device("cpu"), torch.float32) for m in (fq, ref))
        a, b = fq(ids, ca, 0), ref(ids, cb, 0)
        assert torch.equal(a, b), "prefill"
        for step in range(3):
            tok = b[:, -1].argmax(-1, keepdim=True)
            a, b = fq(tok, ca, 9 + step), ref(tok, cb, 9 + step)
            assert torch.equal(a, b), step
        assert ca[0].seq_len == cb[0].seq_len == 12
        assert all(torch.equal(x.k, y.k) and torch.equal(x.v, y.v) for x, y in zip(ca, cb))


def test_quantised_bytes_and_no_wide_copy(models):
    fq, _ = models
    hd, inter, V = CFG["hidden_dim"], CFG["intermediate_dim"], CFG["vocab_size"]
    head = hd // CFG["num_heads"]
    shapes = [((CFG["num_heads"] + 2 * CFG["num_kv_heads"]) * head, hd), (hd, hd), (inter, hd), (inter, hd), (hd, inter)]
    shapes = shapes * CFG["num_layers"] + [(V, hd)]
    lins = fq.linears()
    assert [tuple(l.codes.shape) for l in lins] == shapes
    for lin, (n, k) in zip(lins, shapes):
        assert lin.codes.dtype == torch.float8_e4m3fn and lin.scale.dtype == torch.float32
        assert lin.nbytes() == n * k + 4 * n
    assert fq.quantized_bytes() == sum(n * k + 4 * n for n, k in shapes)

    # every tensor reachable from the module: parameters, buffers and plain attributes, recursively
    seen, tensors = set(), []

    def walk(obj):
        if id(obj) in seen:
            return
        seen.add(id(obj))
        if isinstance(obj, torch.Tensor):
            tensors.append(obj)
        elif isinstance(obj, (list, tuple, set)):
            for o in obj:
                walk(o)
        elif isinstance(obj, dict):
            for o in obj.values():
                walk(o)
        elif hasattr(obj, "__dict__"):
            walk(vars(obj))
    walk(fq)
    assert len(tensors) >= 2 * len(lins) + 2
    wide = [tuple(t.shape) for t in tensors if t.dim() == 2 and t.dtype != torch.float8_e4m3fn]
    assert wide == [(V, hd)], f"only the embedding stays wide, found {wide}"
    assert not [n for n, _ in fq.named_parameters() if "proj" in n or "lm_head" in n]
