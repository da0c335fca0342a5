"""ch02.Sampler and the ``sampler=`` keyword of the generation loops on the CPU:
the CPU path of the sampler is the rule (equal to the float64 oracle on every
row of the case list), a sampled generation is a function of the seed with the
token at sequence position p drawn at offset p, and ``sampler=None`` is the old
softmax / multinomial path."""
from __future__ import annotations

import inspect

import numpy as np
import pytest
import torch

import sample_cases as sc
from ch02 import CachedTransformerModel, Sampler, cached_generate, naive_generate, sample_cpu
from ch02.sampling import philox_uniforms

TDT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def _tensor(logits: np.ndarray, dtype: str) -> torch.Tensor:
    return torch.from_numpy(logits).to(TDT[dtype])   # exact: the values are representable


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_cpu_sampler_equals_the_oracle(case):
    logits, u, want = sc.build(case)
    x = _tensor(logits, case.dtype)
    if case.uniforms is not None:
        got = sample_cpu(x, case.temperature, case.top_k, case.top_p, uniforms=torch.from_numpy(u))
    else:
        s = Sampler(case.temperature, case.top_k, case.top_p, seed=case.seed)
        od = None if case.offset_dev is None else torch.tensor([case.offset_dev], dtype=torch.int32)
        offset = case.offset_add if od is None else (od, case.offset_add)
        got = s(x, offset)
    assert got.dtype == torch.int64 and got.shape == (case.rows,)
    assert got.tolist() == want.tolist(), case


def test_cpu_sampler_shapes_offsets_and_out():
    x = torch.from_numpy(np.random.RandomState(0).standard_normal((2, 3, 40)).astype(np.float32))
    s = Sampler(0.7, top_k=10, top_p=0.9, seed=99)
    a = s(x, 5)
    assert a.shape == (2, 3)
    # rows are numbered through the leading dimensions; a device-style offset tensor and a pair mean the same
    assert a.reshape(-1).tolist() == s(x.reshape(6, 40), torch.tensor([5], dtype=torch.int32)).tolist()
    assert a.tolist() == s(x, (torch.tensor([2], dtype=torch.int32), 3)).tolist()
    buf = torch.full((2, 7), -7, dtype=torch.int64)
    assert s(x[:, 0], 5, out=buf[:, 3]) is not None and buf[:, 3].tolist() == s(x[:, 0], 5).tolist()
    assert (buf[:, :3] == -7).all() and (buf[:, 4:] == -7).all()
    assert np.array_equal(philox_uniforms(99, 5, 6), sc.philox_u(99, 5, np.arange(6)))
    for bad in (dict(temperature=-1.0), dict(top_p=-0.5), dict(temperature=float("nan"))):
        with pytest.raises(ValueError):
            Sampler(**bad)


def _tiny():
    torch.manual_seed(0)
    return CachedTransformerModel(vocab_size=61, hidden_dim=32, num_layers=2, num_heads=4, num_kv_heads=2,
                                  intermediate_dim=48).eval()


def test_cached_generate_with_a_sampler_is_a_function_of_the_seed():
    model = _tiny()
    ids = torch.tensor([[3, 1, 4, 1, 5], [9, 2, 6, 5, 3]])
    s = Sampler(0.9, top_k=20, top_p=0.95, seed=1234)
    torch.manual_seed(1)
    a, timings = cached_generate(model, ids, 6, sampler=s)
    torch.manual_seed(2)       # torch's generator plays no part
    b, _ = cached_generate(model, ids, 6, sampler=Sampler(0.9, top_k=20, top_p=0.95, seed=1234))
    assert a.shape == (2, 11) and torch.equal(a, b) and torch.equal(a[:, :5], ids)
    assert len(timings["decode_ms"]) == 5
    c, _ = cached_generate(model, ids, 6, sampler=Sampler(0.9, top_k=20, top_p=0.95, seed=1235))
    assert not torch.equal(a, c)
    # the token at sequence position p is the rule on the model's logits for it, drawn at offset p
    with torch.no_grad():
        for p in range(5, 11):
            logits = model(a[:, :p])[:, -1]
            u = sc.philox_u(1234, p, np.arange(2))
            want = [sc.oracle_row(logits[r].numpy(), 0.9, 20, 0.95, u[r]) for r in range(2)]
            if all(sc.check_row(w) for w in want):   # (recomputed logits differ from the cached ones in the last bits)
                assert a[:, p].tolist() == [w.token for w in want], p
    # greedy through the same keyword
    g, _ = cached_generate(model, ids, 4, sampler=Sampler(0.0))
    with torch.no_grad():
        for p in range(5, 9):
            assert g[:, p].tolist() == model(g[:, :p])[:, -1].argmax(-1).tolist()


def test_sampler_none_is_the_old_path(monkeypatch):
    model = _tiny()
    ids = torch.tensor([[3, 1, 4, 1, 5]])
    assert inspect.signature(cached_generate).parameters["sampler"].default is None
    assert list(inspect.signature(naive_generate).parameters) == ["model", "input_ids", "max_new_tokens", "temperature",
                                                                  "top_k"]
    calls = []
    real = torch.multinomial
    monkeypatch.setattr(torch, "multinomial", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    torch.manual_seed(7)
    a, _ = cached_generate(model, ids, 5, temperature=0.8)
    assert len(calls) == 5
    torch.manual_seed(7)
    b, _ = cached_generate(model, ids, 5, temperature=0.8, sampler=None)
    assert torch.equal(a, b) and len(calls) == 10
    # the chain itself: softmax(logits / T) -> multinomial, from torch's generator
    torch.manual_seed(7)
    with torch.no_grad():
        probs = torch.softmax(model(ids)[:, -1] / 0.8, dim=-1)
    assert real(probs, 1).item() == a[0, 5].item()
    cached_generate(model, ids, 3, sampler=Sampler(1.0, seed=3))
    assert len(calls) == 10   # with a sampler the chain is not run
