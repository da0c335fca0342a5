"""The sampler inside the captured decode step (ch08.DecodeStepGraph(sampler=...))
on a small ch02.CachedTransformerModel: every generated token is the float64
rule of tests/sample_cases.py applied to that step's own logits at the offset
of its sequence position, greedy sampling is the argmax loop over the existing
step(), and generation is a function of the seed."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import sample_cases as sc

pytestmark = pytest.mark.gpu

VOCAB, PROMPT, N, SEQ = 1000, 9, 8, 32


def _model():
    from ch02 import CachedTransformerModel
    torch.manual_seed(0)
    return CachedTransformerModel(VOCAB, 256, 2, 4, 2, 512).cuda().bfloat16().eval()


def _prompt(B):
    return torch.from_numpy(np.random.RandomState(B).randint(0, VOCAB, (B, PROMPT))).cuda()


def _expect(logits_row, t, k, p, seed, pos, row):
    """the rule on one row of logits at offset pos; the row has to meet the input condition"""
    u = sc.philox_u(seed, pos, [row])[0]
    pick = sc.oracle_row(logits_row.float().cpu().numpy(), t, k, p, u)
    assert sc.check_row(pick), ("input condition", pos, row, pick.margin_u, pick.margin_p)
    return pick.token


@pytest.mark.parametrize("B", [1, 3])
def test_generate_equals_the_rule_on_each_steps_logits(B):
    from ch02 import Sampler
    from ch08 import DecodeStepGraph
    t, k, p, seed = 0.8, 5, 0.9, 20240 + B
    model, ids = _model(), _prompt(B)
    g = DecodeStepGraph(model, B, SEQ, torch.bfloat16, sampler=Sampler(t, top_k=k, top_p=p, seed=seed))
    lg = g.prefill(ids, sample=True)
    first = g.static_ids.clone()
    assert first.shape == (B, 1) and first.dtype == torch.int64
    for r in range(B):   # the first token: eager, offset = its position
        assert int(first[r, 0]) == _expect(lg[r, -1], t, k, p, seed, PROMPT, r)
    toks, logits = g.generate(N, return_logits=True)
    assert toks.shape == (B, N) and logits.shape == (B, N, VOCAB)
    assert g.seq_len == PROMPT + N and int(g.pos.item()) == PROMPT + N
    assert torch.equal(g.static_ids[:, 0], toks[:, -1])
    for i in range(N):   # replay i consumed the token at position PROMPT + i and drew the one at PROMPT + i + 1
        for r in range(B):
            assert int(toks[r, i]) == _expect(logits[r, i], t, k, p, seed, PROMPT + i + 1, r), (i, r)

    # the same seed through step_sampled() on a second graph, and through a fresh generate(): the same tokens
    g2 = DecodeStepGraph(model, B, SEQ, torch.bfloat16, sampler=Sampler(t, top_k=k, top_p=p, seed=seed))
    g2.prefill(ids, sample=True)
    assert torch.equal(g2.static_ids, first)
    again = []
    for _ in range(N):
        out = g2.step_sampled()
        assert out is g2.static_ids
        again.append(out[:, 0].clone())
    assert torch.equal(torch.stack(again, dim=1), toks)
    g3 = DecodeStepGraph(model, B, SEQ, torch.bfloat16, sampler=Sampler(t, top_k=k, top_p=p, seed=seed + 1))
    g3.prefill(ids, sample=True)
    assert not torch.equal(torch.cat([g3.static_ids.clone(), g3.generate(N)], dim=1), torch.cat([first, toks], dim=1))


def _argmax_lowest(logits):
    """argmax with the lowest index on ties"""
    v = logits.float()
    idx = torch.arange(v.shape[-1], device=v.device).expand_as(v)
    return torch.where(v == v.max(-1, keepdim=True).values, idx, v.shape[-1]).min(-1).values


@pytest.mark.parametrize("B", [1, 3])
def test_greedy_equals_the_argmax_loop_over_step(B):
    from ch02 import Sampler
    from ch08 import DecodeStepGraph
    model, ids = _model(), _prompt(B)
    ref = DecodeStepGraph(model, B, SEQ, torch.bfloat16)
    lg = ref.prefill(ids)
    want, tok = [], _argmax_lowest(lg[:, -1])
    for _ in range(N + 1):
        want.append(tok.clone())
        if len(want) <= N:
            tok = _argmax_lowest(ref.step(tok.view(B, 1))[:, -1])
    g = DecodeStepGraph(model, B, SEQ, torch.bfloat16, sampler=Sampler(0.0))
    g.prefill(ids, sample=True)
    got = torch.cat([g.static_ids.clone(), g.generate(N)], dim=1)
    assert torch.equal(got, torch.stack(want, dim=1))


def test_sampled_steps_need_a_sampler_and_room():
    from ch02 import Sampler
    from ch08 import DecodeStepGraph
    model, ids = _model(), _prompt(1)
    plain = DecodeStepGraph(model, 1, SEQ, torch.bfloat16)
    with pytest.raises(RuntimeError):
        plain.prefill(ids, sample=True)
    with pytest.raises(RuntimeError):
        plain.step_sampled()
    g = DecodeStepGraph(model, 1, PROMPT + 2, torch.bfloat16, sampler=Sampler(1.0, top_k=4, seed=1))
    with pytest.raises(RuntimeError):
        g.step_sampled()      # before prefill
    g.prefill(ids, sample=True)
    with pytest.raises(RuntimeError):
        g.generate(3)         # two rows left in the cache
    assert g.generate(2).shape == (1, 2)
