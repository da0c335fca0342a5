"""Next-token sampling for the generation loops: temperature, top-k, top-p and
the draw of the reference's three samplers (``ch02/generation.py:23-31``,
``ch02/cached_generation.py:245,265``, ``ch10/engine.py:96-115``) as ONE rule
with a counter-based random stream, so a sequence is a function of the seed.

``Sampler`` on a ROCm device is one launch of ``pli_hip.sample`` (graph-
capturable: the per-step offset is read on the device).  Elsewhere
``sample_cpu`` runs the same rule in numpy with the kernel's arithmetic -- fp32
``exp((x - max) / temperature)``, weights as integers ``floor(w * 2^45)``,
integer sums -- and the same Philox4x32-10, so a CPU run and a GPU run of one
seed agree wherever no decision sits within the fp32 ``exp``'s error of its
threshold (DESIGN.md "Sampling").

The rule, per row: NaN counts as -inf, -0 as +0; no logit above -inf gives -1;
with a +inf in the row the +inf logits weigh 1, the rest 0; "before" is larger
value first, lower index first among equals; temperature 0 takes the first
token; top-k keeps the first ``top_k``; top-p keeps a token iff the weight
before it is <= ``top_p`` times the kept sum; the draw walks the kept tokens
in ascending index and takes the first whose running sum exceeds ``u`` times
their sum; ``u = (r0 >> 8) * 2^-24``, r0 the first Philox word for key
``{seed lo, seed hi}`` and counter ``{(uint32)offset, row, 0, 0}``.
"""
from __future__ import annotations

import numpy as np
import torch

_FRAC_BITS = 45
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 over arrays of 32-bit words (uint64 arithmetic): 4 counter words, 2 key words -> 4 words"""
    c = list(np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) & _M32 for v in counter]))
    k = [np.asarray(v, dtype=np.uint64) & _M32 for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _M32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & _M32, (k[1] + np.uint64(0xBB67AE85)) & _M32]
    return c


def philox_uniforms(seed: int, offset: int, rows: int) -> np.ndarray:
    """u of rows 0 .. rows - 1 as float32 (every value is exact in fp32)"""
    r0 = philox4x32_10((int(offset) & 0xFFFFFFFF, np.arange(rows, dtype=np.uint64), 0, 0),
                       (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))[0]
    return ((r0 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def _sample_row(x: np.ndarray, t: np.float32, top_k: int, p: np.float32, u: np.float32) -> int:
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x = np.where(np.isnan(x), np.float32(-np.inf), x).astype(np.float32) + np.float32(0.0)
        if not (x > -np.inf).any():
            return -1
        V = x.size
        order = np.lexsort((np.arange(V), -x))
        if t == 0:
            return int(order[0])
        m = x.max()
        if m == np.inf:
            w = (x == np.inf).astype(np.float32)
        else:
            w = np.exp((x - m) / t).astype(np.float32)
            w[x == -np.inf] = 0.0
        wfx = np.floor(w.astype(np.float64) * 2.0 ** _FRAC_BITS).astype(np.uint64)
        k1 = order if (top_k <= 0 or top_k >= V) else order[:top_k]
        k2 = k1
        if p < 1:
            wk = wfx[k1]
            run = np.cumsum(wk)
            limit = np.uint64(float(p) * float(int(run[-1])))
            k2 = k1[(run - wk) <= limit]
        ids = np.sort(k2)
        run = np.cumsum(wfx[ids])
        target = np.uint64(float(u) * float(int(run[-1])))
        return int(ids[np.nonzero(run > target)[0][0]])


def sample_cpu(logits: torch.Tensor, temperature: float = 1.0, top_k: int | None = None, top_p: float = 1.0, *,
               uniforms=None, seed: int = 0, offset=0, out: torch.Tensor | None = None) -> torch.Tensor:
    """``pli_hip.sample`` on CPU tensors, row by row in numpy (same signature, same rule, same random stream)"""
    if temperature < 0 or top_p < 0 or temperature != temperature or top_p != top_p:
        raise ValueError("sample: temperature and top_p must be >= 0")
    lead, V = tuple(logits.shape[:-1]), logits.shape[-1]
    x = logits.detach().reshape(-1, V).float().cpu().numpy()
    rows = x.shape[0]
    if uniforms is None:
        off_dev, off_add = (None, offset) if isinstance(offset, int) else offset if isinstance(offset, tuple) else (offset, 0)
        total = (int(off_dev.reshape(-1)[0]) if off_dev is not None else 0) + int(off_add)
        u = philox_uniforms(seed, total, rows)
    else:
        u = np.asarray(torch.as_tensor(uniforms).detach().cpu().numpy(), dtype=np.float32).reshape(rows)
    t, p = np.float32(temperature), np.float32(top_p)
    toks = [_sample_row(x[r], t, int(top_k or 0), p, u[r]) for r in range(rows)]
    res = torch.tensor(toks, dtype=torch.int64, device=logits.device).reshape(lead)
    if out is None:
        return res
    out.copy_(res)
    return out


class Sampler:
    """One temperature / top_k / top_p / seed (a captured graph holds one of each).

        s = Sampler(temperature=0.8, top_k=50, top_p=0.95, seed=1234)
        tok = s(logits[:, -1], offset=position)      # int64 [B]

    ``offset`` selects the random numbers of the call: the generation loops pass the sequence position of the
    token being drawn, so the sequence is a function of the seed alone, on any device and through any loop
    (eager, cached, graph-captured).  On a ROCm device it may be an int32 device tensor (read by the kernel) or
    a ``(tensor, add)`` pair."""

    def __init__(self, temperature: float = 1.0, top_k: int | None = None, top_p: float = 1.0, seed: int = 0):
        if temperature < 0 or top_p < 0 or temperature != temperature or top_p != top_p:
            raise ValueError("Sampler: temperature and top_p must be >= 0")
        self.temperature, self.top_k, self.top_p, self.seed = float(temperature), top_k, float(top_p), int(seed)

    def __call__(self, logits: torch.Tensor, offset=0, out: torch.Tensor | None = None) -> torch.Tensor:
        if logits.is_cuda:
            import pli_hip
            return pli_hip.sample(logits, self.temperature, self.top_k, self.top_p, seed=self.seed, offset=offset,
                                  out=out)
        return sample_cpu(logits, self.temperature, self.top_k, self.top_p, seed=self.seed, offset=offset, out=out)
