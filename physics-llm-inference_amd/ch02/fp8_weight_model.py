"""``Fp8WeightModel``: a ``CachedTransformerModel`` with fp8 e4m3 weights (W8A16).

``Fp8WeightModel.from_model(model)`` quantises every projection of the wrapped
model -- each layer's packed ``[Wq; Wk; Wv]``, ``o_proj``, gate, up, down and
``lm_head`` -- to one e4m3fn code per weight and one fp32 scale per output row
(``pli_hip.quantize_weight_fp8``), keeps the embedding and the norms in the
model's dtype, and keeps no 16-bit copy of a quantised weight.  ``forward`` and
``create_caches`` have the wrapped model's signatures, so
``ch08.DecodeStepGraph`` and a ``cached_generate``-style loop take it unchanged.

On a ROCm device a layer is the wrapped model's unfused device sequence with
the fp8 calls: ``pli_rmsnorm`` (+ residual) -> ``pli_linear_fp8w`` (packed qkv)
-> cache append -> decode / prefill attention -> ``pli_linear_fp8w`` (o_proj)
-> ``pli_rmsnorm`` (+ residual) -> ``pli_linear_swiglu_fp8w`` ->
``pli_linear_fp8w`` (down): 7 launches against the 16-bit model's 5.  Prompt-sized
calls without a fast fp8 kernel go through the widen + GEMM route over one
workspace, grown outside any capture.  On the CPU the weights are dequantised
and the wrapped model's own CPU math runs.

``from_model(model, fused_decode=True)`` takes the 16-bit model's fused decode
step over the fp8 weights: a call that passes ``CachedTransformerModel``'s
``_fused_decode_ok`` conditions (at most 4 rows, a device-resident cache
length) and has ``hidden % 16 == 0`` runs, per layer, 5 launches --
``pli_rms_gemm_nt_fp8w`` (input norm + the pending residual add + q / k / v
over the row blocks of the packed codes and scales, k / v straight into the
cache) -> ``pli_attn_decode_dev`` -> ``pli_linear_fp8w`` (o_proj) ->
``pli_rms_gemm_nt_fp8w`` (post-attention norm + residual + gate / up / silu *
mul) -> ``pli_linear_fp8w`` (down) -- and the final norm inside the ``lm_head``
launch.  The fused launch is bitwise ``pli_rmsnorm`` followed by the vec route
of ``pli_linear_fp8w``, so a batch-1 step gives the unfused path's logits bit
for bit.  Every other call (prefill, more rows, no device length, the CPU)
takes the path above; the default is ``fused_decode=False``, and it is the
faster path wherever the two were measured (the fused step is
level at batch 1 of the 0.85B shape and slower elsewhere).

Build it from a model that already sits on its device: the quantised tensors
are plain attributes, which ``Module.to`` does not move.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

import pli_hip

from .cached_generation import CachedTransformerModel, LayerKVCache, RMSNorm, _device_len_ok, _device_len_ok_shape
from .kv_cache import attend_cached


def _pow2_scale(w: torch.Tensor) -> torch.Tensor:
    """the smallest power of two >= absmax / 448 per row (1 for a zero row): the dequantised values are then bf16
    and fp16 values"""
    amax = w.detach().float().abs().amax(dim=1)
    return torch.where(amax > 0, torch.exp2(torch.ceil(torch.log2(amax.clamp_min(1e-30) / 448.0))), torch.ones_like(amax))


class Fp8Linear:
    """codes [n, k] e4m3fn + scale fp32 [n] of one bias-free projection (not a Module: nothing casts or moves it)"""

    def __init__(self, weight: torch.Tensor, pow2_scales: bool = False):
        self.codes, self.scale = pli_hip.quantize_weight_fp8(weight, scale=_pow2_scale(weight) if pow2_scales else None)
        self.out_features, self.in_features = self.codes.shape

    def nbytes(self) -> int:
        return self.codes.numel() * self.codes.element_size() + self.scale.numel() * self.scale.element_size()

    def dequantized(self, dtype: torch.dtype, rows: slice = slice(None)) -> torch.Tensor:
        return (self.codes[rows].float() * self.scale[rows, None]).to(dtype)

    def __call__(self, x: torch.Tensor, workspace: torch.Tensor | None = None) -> torch.Tensor:
        if not x.is_cuda:
            return F.linear(x, self.dequantized(x.dtype))
        lead = x.shape[:-1]
        y = pli_hip.linear_fp8w(x.reshape(-1, x.shape[-1]), self.codes, self.scale, workspace=workspace)
        return y.view(*lead, self.out_features)


class Fp8Block(nn.Module):
    def __init__(self, block, pow2_scales: bool):
        super().__init__()
        at, ffn = block.attn, block.ffn
        self.num_heads, self.num_kv_heads, self.head_dim = at.num_heads, at.num_kv_heads, at.head_dim
        self.hidden_dim = at.hidden_dim
        self.input_norm, self.post_attn_norm = block.input_norm, block.post_attn_norm
        with torch.no_grad():
            self.qkv = Fp8Linear(torch.cat([at.q_proj.weight, at.k_proj.weight, at.v_proj.weight]), pow2_scales)
        self.o_proj = Fp8Linear(at.o_proj.weight, pow2_scales)
        self.gate = Fp8Linear(ffn.gate_proj.weight, pow2_scales)
        self.up = Fp8Linear(ffn.up_proj.weight, pow2_scales)
        self.down = Fp8Linear(ffn.down_proj.weight, pow2_scales)

    def linears(self) -> list[Fp8Linear]:
        return [self.qkv, self.o_proj, self.gate, self.up, self.down]

    # ---- the wrapped model's CPU math over the dequantised weights
    def forward_cpu(self, x: torch.Tensor, cache: LayerKVCache | None) -> torch.Tensor:
        h = x + self._attn_cpu(self.input_norm(x), cache)
        n2 = self.post_attn_norm(h)
        g = F.silu(self.gate(n2)) * self.up(n2)
        return h + self.down(g)

    def _attn_cpu(self, x: torch.Tensor, cache: LayerKVCache | None) -> torch.Tensor:
        B, S, _ = x.shape
        nq, nk = self.num_heads * self.head_dim, self.num_kv_heads * self.head_dim
        q = F.linear(x, self.qkv.dequantized(x.dtype, slice(0, nq))).view(B, S, self.num_heads, self.head_dim)
        k = F.linear(x, self.qkv.dequantized(x.dtype, slice(nq, nq + nk))).view(B, S, self.num_kv_heads, self.head_dim)
        v = F.linear(x, self.qkv.dequantized(x.dtype, slice(nq + nk, None))).view(B, S, self.num_kv_heads, self.head_dim)
        if cache is not None:
            cache.update(k, v)
            k_buf, v_buf, n_kv = cache.k, cache.v, cache.seq_len
        else:
            k_buf, v_buf, n_kv = k, v, S
        return self.o_proj(attend_cached(q, k_buf, v_buf, n_kv).reshape(B, S, self.hidden_dim))

    # ---- device path: (x, pending FFN output) -> (residual stream, pending FFN output)
    def forward_gpu(self, x: torch.Tensor, pending: torch.Tensor | None, cache: LayerKVCache | None,
                    ws: torch.Tensor | None) -> tuple[torch.Tensor, torch.Tensor]:
        B, S, _ = x.shape
        if pending is None:
            n1 = pli_hip.rmsnorm(x, self.input_norm.weight, self.input_norm.eps)
        else:
            x, n1 = pli_hip.rmsnorm(pending, self.input_norm.weight, self.input_norm.eps, residual=x)
        nq, nk = self.num_heads * self.head_dim, self.num_kv_heads * self.head_dim
        qkv = self.qkv(n1, ws)
        q = qkv[..., :nq].unflatten(-1, (self.num_heads, self.head_dim))
        k = qkv[..., nq:nq + nk].unflatten(-1, (self.num_kv_heads, self.head_dim))
        v = qkv[..., nq + nk:].unflatten(-1, (self.num_kv_heads, self.head_dim))
        if cache is not None:
            cache.update(k, v)
            if cache.pos is not None and _device_len_ok(q, cache):
                o = pli_hip.attn_decode_dev(q, cache.k, cache.v, cache.pos, n_kv_add=S, causal=S > 1)
            else:
                o = attend_cached(q, cache.k, cache.v, cache.seq_len)
        else:
            o = attend_cached(q, k, v, S)
        a = self.o_proj(o.reshape(B, S, self.hidden_dim), ws)
        h, n2 = pli_hip.rmsnorm(a, self.post_attn_norm.weight, self.post_attn_norm.eps, residual=x)
        g = pli_hip.linear_swiglu_fp8w(n2.reshape(B * S, -1), self.gate.codes, self.gate.scale, self.up.codes,
                                       self.up.scale, workspace=ws)
        return h, self.down(g, ws).view(B, S, self.hidden_dim)

    # ---- fused decode step (CachedTransformerBlock.decode_fused over the fp8 weights): 5 launches
    def decode_fused(self, x: torch.Tensor, pending: torch.Tensor | None, cache: LayerKVCache
                     ) -> tuple[torch.Tensor, torch.Tensor]:
        B, S, hd = x.shape
        nq, nk = self.num_heads * self.head_dim, self.num_kv_heads * self.head_dim
        codes, scale = self.qkv.codes, self.qkv.scale
        # q / k / v: row blocks of the packed codes and scales, used in place
        wq, wk, wv = ((codes[a:b], scale[a:b]) for a, b in ((0, nq), (nq, nq + nk), (nq + nk, nq + 2 * nk)))
        cache.reserve(S)
        q = torch.empty(B, S, nq, device=x.device, dtype=x.dtype)
        norm = self.input_norm
        if pending is None:
            pli_hip.rms_qkv_into_cache_fp8w(x, norm.weight, norm.eps, wq, wk, wv, q, cache.k, cache.v, cache.pos)
        else:
            h = torch.empty_like(x)
            pli_hip.rms_qkv_into_cache_fp8w(pending, norm.weight, norm.eps, wq, wk, wv, q, cache.k, cache.v,
                                            cache.pos, residual=x, h_out=h)
            x = h
        cache.seq_len += S
        o = pli_hip.attn_decode_dev(q.view(B, S, self.num_heads, self.head_dim), cache.k, cache.v, cache.pos,
                                    n_kv_add=S, causal=S > 1)
        a = self.o_proj(o.reshape(B, S, hd))
        h2 = torch.empty_like(x)
        g = pli_hip.rms_swiglu_fp8w(a, self.post_attn_norm.weight, self.post_attn_norm.eps, self.gate.codes,
                                    self.gate.scale, self.up.codes, self.up.scale, residual=x, h_out=h2)
        return h2, self.down(g)


class Fp8WeightModel(nn.Module):
    """See the module docstring.  Construct with ``from_model``."""

    def __init__(self, model: CachedTransformerModel, pow2_scales: bool = False, fused_decode: bool = False):
        super().__init__()
        self.fused_decode = bool(fused_decode)
        self.embed, self.norm = model.embed, model.norm
        self.layers = nn.ModuleList([Fp8Block(b, pow2_scales) for b in model.layers])
        self.lm_head = Fp8Linear(model.lm_head.weight, pow2_scales)
        self.hidden_dim, self.num_layers = model.hidden_dim, model.num_layers
        self.num_kv_heads, self.head_dim = model.num_kv_heads, model.head_dim
        self._ws: torch.Tensor | None = None

    @classmethod
    def from_model(cls, model: CachedTransformerModel, pow2_scales: bool = False, fused_decode: bool = False
                   ) -> "Fp8WeightModel":
        """``pow2_scales``: power-of-two row scales (a 16-bit model can then hold the identical dequantised
        weights); default absmax / 448.  ``fused_decode``: decode steps of at most 4 rows over a device-resident
        cache length run the 5-launch layer of ``pli_rms_gemm_nt_fp8w`` (module docstring); default the
        unfused 7-launch layer"""
        return cls(model, pow2_scales, fused_decode)

    # the 16-bit model's conditions over this model's layers (they carry num_heads / num_kv_heads / head_dim)
    def _fused_decode_ok(self, x: torch.Tensor, caches) -> bool:
        if not self.fused_decode or caches is None or caches[0].pos is None or not len(self.layers):
            return False
        B, S, hd = x.shape
        b0 = self.layers[0]
        # pli_rms_gemm_nt_fp8w's rules (include/pli.h): 1 <= m <= 4 rows, k % 16 == 0, k <= 8192
        return (B * S <= 4 and hd % 16 == 0 and hd <= 8192 and B * S * hd * 2 <= 65536
                and _device_len_ok_shape(x, S, b0.num_heads, b0.num_kv_heads, b0.head_dim))

    create_caches = CachedTransformerModel.create_caches

    def linears(self) -> list[Fp8Linear]:
        return [lin for b in self.layers for lin in b.linears()] + [self.lm_head]

    def quantized_bytes(self) -> int:
        return sum(lin.nbytes() for lin in self.linears())

    def _workspace(self, m: int, dtype: torch.dtype, device: torch.device) -> torch.Tensor | None:
        """one workspace for every projection of an m-row call (None when every one has a fast route); grown on
        first use, which for prompt sizes is the eager prefill, outside any capture"""
        need = 0
        for b in self.layers:
            need = max(need, *(pli_hip.linear_fp8w_workspace_bytes(m, lin.out_features, lin.in_features, dtype)
                               for lin in (b.qkv, b.o_proj, b.down)),
                       pli_hip.linear_fp8w_workspace_bytes(m, b.gate.out_features, b.gate.in_features, dtype, swiglu=True))
        need = max(need, pli_hip.linear_fp8w_workspace_bytes(m, self.lm_head.out_features, self.lm_head.in_features, dtype))
        if need == 0:
            return None
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws

    def forward(self, input_ids: torch.Tensor, caches: list[LayerKVCache] | None = None, start_pos: int = 0
                ) -> torch.Tensor:
        x = self.embed(input_ids)
        if not x.is_cuda:
            for i, layer in enumerate(self.layers):
                x = layer.forward_cpu(x, caches[i] if caches is not None else None)
            return self.lm_head(self.norm(x))
        if self._fused_decode_ok(x, caches):
            pending = None
            for i, layer in enumerate(self.layers):
                x, pending = layer.decode_fused(x, pending, caches[i])
            caches[0].pos.add_(input_ids.shape[1])
            return pli_hip.rms_linear_fp8w(pending, self.norm.weight, self.norm.eps, self.lm_head.codes,
                                           self.lm_head.scale, residual=x)
        ws = self._workspace(x.shape[0] * x.shape[1], x.dtype, x.device)
        pending = None
        for i, layer in enumerate(self.layers):
            x, pending = layer.forward_gpu(x, pending, caches[i] if caches is not None else None, ws)
        if caches is not None and caches[0].pos is not None:
            caches[0].pos.add_(input_ids.shape[1])  # one length shared by every layer
        if pending is None:  # no layers
            xn = pli_hip.rmsnorm(x, self.norm.weight, self.norm.eps)
        else:
            _, xn = pli_hip.rmsnorm(pending, self.norm.weight, self.norm.eps, residual=x)
        return self.lm_head(xn, ws)
