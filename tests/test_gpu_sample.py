"""pli_sample on the GPU against the float64 rule of tests/sample_cases.py:
token equality on every row of every case (the cases meet the input condition,
so the rule has one answer), through padded and misaligned logits with NaN in
the padding, strided guarded outputs, a guarded workspace, repeated calls, the
route names, and capture + replay with the offset advanced on the device."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import sample_cases as sc

pytestmark = pytest.mark.gpu

TDT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
SENTINEL = -0x5151515151515151
WS_BYTES = 256


def padded_logits(logits: np.ndarray, dtype: str, pad: int = 5, lead: int = 1) -> torch.Tensor:
    """[rows, vocab] view (row stride vocab + pad, starting `lead` elements into the buffer, so rows are not
    16-byte aligned) of a NaN-filled device buffer"""
    rows, vocab = logits.shape
    buf = torch.full((rows, vocab + pad), float("nan"), dtype=TDT[dtype], device="cuda")
    view = buf[:, lead:lead + vocab]
    view.copy_(torch.from_numpy(logits).to(TDT[dtype]))
    return view


def run(case, x: torch.Tensor, u: np.ndarray, od=None, offset_add=None, stride: int = 3):
    """one pli_sample call straight through the C ABI: tokens strided through a sentinel-filled buffer, a
    sentinel-filled workspace; returns (tokens int64 [rows] on the host, the route)"""
    import pli_hip
    L = pli_hip.lib()
    rows, vocab = x.shape
    guard = torch.full((rows + 2, stride), SENTINEL, dtype=torch.int64, device="cuda")
    out = guard[1:rows + 1, 1]
    ws = torch.full((WS_BYTES,), 0xA5, dtype=torch.uint8, device="cuda")
    uni = torch.from_numpy(u).cuda() if case.uniforms is not None else None
    if od is None and case.offset_dev is not None:
        od = torch.tensor([case.offset_dev], dtype=torch.int32, device="cuda")
    rc = L.pli_sample(x.data_ptr(), x.stride(0), rows, vocab, sc.DTYPE_CODE[case.dtype], case.temperature, case.top_k,
                      case.top_p, None if uni is None else uni.data_ptr(), case.seed,
                      None if od is None else od.data_ptr(), case.offset_add if offset_add is None else offset_add,
                      out.data_ptr(), out.stride(0), ws.data_ptr(), WS_BYTES,
                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.pli_last_error()
    route = pli_hip.last_route()
    g = guard.cpu()
    mask = torch.ones_like(g, dtype=torch.bool)
    mask[1:rows + 1, 1] = False
    assert (g[mask] == SENTINEL).all(), "a token written outside its slot"
    assert (ws.cpu() == 0xA5).all(), "the workspace was written (its size is 0)"
    return g[1:rows + 1, 1].clone(), route


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_tokens_equal_the_oracle_on_every_row(case):
    logits, u, want = sc.build(case)
    x = padded_logits(logits, case.dtype)
    got, route = run(case, x, u)
    assert route == ("sample_greedy" if case.temperature == 0 else "sample_select")
    assert got.tolist() == want.tolist(), case
    for _ in range(2):   # the same inputs give the same tokens on every call
        again, _ = run(case, x, u)
        assert torch.equal(again, got)


@pytest.mark.parametrize("name", ["vocab1025_bf16", "kp_v257_k7_p0.9", "uniforms_fp16", "philox_4", "special_fp32_t1.0_k3_p0.5",
                                  "big32000_bf16_k50_p0.9"])
def test_binding_equals_the_oracle(name):
    """pli_hip.sample: leading dimensions, offset forms, a strided out, a non-unit inner stride"""
    import pli_hip
    case = next(c for c in sc.CASES if c.name == name)
    logits, u, want = sc.build(case)
    x = padded_logits(logits, case.dtype)
    kw = dict(seed=case.seed)
    if case.uniforms is not None:
        kw["uniforms"] = torch.from_numpy(u).cuda()
    elif case.offset_dev is not None:
        kw["offset"] = (torch.tensor([case.offset_dev], dtype=torch.int32, device="cuda"), case.offset_add)
    else:
        kw["offset"] = case.offset_add
    got = pli_hip.sample(x, case.temperature, case.top_k, case.top_p, **kw)
    assert got.dtype == torch.int64 and got.shape == (case.rows,) and got.tolist() == want.tolist()
    buf = torch.full((case.rows, 4), SENTINEL, dtype=torch.int64, device="cuda")
    assert pli_hip.sample(x, case.temperature, case.top_k, case.top_p, out=buf[:, 2], **kw).data_ptr() == buf[:, 2].data_ptr()
    assert buf[:, 2].tolist() == want.tolist() and (buf[:, [0, 1, 3]] == SENTINEL).all()
    xt = x.t().contiguous().t()   # inner stride != 1: copied first
    assert xt.stride(1) != 1 or case.rows == 1
    assert pli_hip.sample(xt, case.temperature, case.top_k, case.top_p, **kw).tolist() == want.tolist()
    x3 = x.contiguous().view(1, case.rows, case.vocab)
    assert pli_hip.sample(x3, case.temperature, case.top_k, case.top_p, **kw).shape == (1, case.rows)
    with pytest.raises(pli_hip.PliError):
        pli_hip.sample(x, -1.0)
    with pytest.raises(pli_hip.PliError):
        pli_hip.sample(x.cpu())


def _replay_inputs(rows, vocab, dtype, t, k, p, seed, offsets):
    """logits whose every row meets the input condition at every offset of the replay sequence"""
    logits = np.empty((rows, vocab), dtype=np.float32)
    want = np.empty((len(offsets), rows), dtype=np.int64)
    for r in range(rows):
        for attempt in range(400):
            x = sc.make_row("normal", vocab, dtype, 31337 + 1000 * r + attempt)
            picks = [sc.oracle_row(x, t, k, p, sc.philox_u(seed, o, [r])[0]) for o in offsets]
            if all(sc.check_row(pk) for pk in picks):
                break
        assert all(sc.check_row(pk) for pk in picks)
        logits[r], want[:, r] = x, [pk.token for pk in picks]
    return logits, want


@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_capture_and_replay_with_the_offset_bumped_on_the_device(dtype):
    """a captured pli_sample followed by offset_dev += 3 on the device: replay i draws with offset
    start + 3 i + offset_add, read by the kernel; the sequence wraps past 2^32"""
    import pli_hip
    rows, vocab, t, k, p, seed, add, n = 3, 257, 0.8, 40, 0.95, 0xC0FFEE1234567, 2 ** 32 - 20, 6
    start = 11
    offsets = [start + 3 * i + add for i in range(n)]   # 2^32 - 9 .. 2^32 + 6
    assert offsets[2] < 2 ** 32 <= offsets[3]
    logits, want = _replay_inputs(rows, vocab, dtype, t, k, p, seed, offsets)
    x = padded_logits(logits, dtype)
    od = torch.tensor([start], dtype=torch.int32, device="cuda")
    out = torch.full((rows,), SENTINEL, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        pli_hip.sample(x, t, k, p, seed=seed, offset=(od, add), out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pli_hip.sample(x, t, k, p, seed=seed, offset=(od, add), out=out)
        od.add_(3)
    od.fill_(start)
    got = []
    for _ in range(n):
        graph.replay()
        got.append(out.clone())
    torch.cuda.synchronize()
    assert int(od.item()) == start + 3 * n
    assert torch.stack(got).cpu().tolist() == want.tolist()


def test_rejects_before_launch_on_the_device():
    import pli_hip
    x = torch.zeros(2, 8, device="cuda")
    L = pli_hip.lib()
    tok = torch.zeros(2, dtype=torch.int64, device="cuda")
    rc = L.pli_sample(x.data_ptr(), 8, 2, 8, 0, float("nan"), 0, 1.0, None, 0, None, 0, tok.data_ptr(), 1, None, 0, None)
    assert rc == 1000 and pli_hip.last_route() == ""
    assert L.pli_sample(x.data_ptr(), 8, 0, 8, 0, 1.0, 0, 1.0, None, 0, None, 0, tok.data_ptr(), 1, None, 0, None) == 0
    assert pli_hip.last_route() == ""
    assert pli_hip.sample(torch.zeros(0, 8, device="cuda")).shape == (0,)
