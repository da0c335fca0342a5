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

``from_model(model).with_fp8_activations()`` gives the calls with more than 16
rows (prefill, large batches) fp8 activations as well (W8A8): every linear
quantises its input rows to e4m3 (``pli_quantize_rows_fp8``) and multiplies
codes by codes on the block-scaled MFMA (``pli_gemm_fp8``) in place of widen +
the 16-bit GEMM, with no workspace; the SwiGLU projection is one quantisation,
two GEMMs and the elementwise product.  Calls of at most 16 rows -- the decode
steps -- stay on the W8A16 kernels, bitwise.  On the CPU the same rule runs in
torch (``linear_fp8a_cpu``).  Default ``False``: every path as without it.  The
threshold of 16 rows is the W8A16 vec kernel's; it was not measured against
the small-M kernel between 17 and 128 rows.

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


# rows up to which a linear stays on the W8A16 decode kernels when fp8 activations are on (the W8A8 GEMM's
# threshold, csrc/fp8a_plan.h; not measured against the small-M kernel between 17 and 128 rows: DESIGN.md 3.3c)
FP8A_ROWS = 16


def linear_fp8a_cpu(x: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """the CPU mirror of ``pli_hip.linear_fp8a``: quantise the rows of x [m, k], fp32 matmul over the decoded codes
    of both operands, the two scales after the sum, one rounding to x's dtype"""
    x8, xs = pli_hip.quantize_rows_fp8(x)
    acc = x8.float() @ codes.float().t()
    return (acc * (xs[:, None] * scale[None, :])).to(x.dtype)


class Fp8Linear:
    """codes [n, k] e4m3fn + scale fp32 [n] of one bias-free projection (not a Module: nothing casts or moves it)"""

    def __init__(self, weight: torch.Tensor, pow2_scales: bool = False):
        self.codes, self.scale = pli_hip.quantize_weight_fp8(weight, scale=_pow2_scale(weight) if pow2_scales else None)
        self.out_features, self.in_features = self.codes.shape

    def nbytes(self) -> int:
        return self.codes.numel() * self.codes.element_size() + self.scale.numel() * self.scale.element_size()

    def dequantized(self, dtype: torch.dtype, rows: slice = slice(None)) -> torch.Tensor:
        return (self.codes[rows].float() * self.scale[rows, None]).to(dtype)

    def __call__(self, x: torch.Tensor, workspace: torch.Tensor | None = None, fp8_activations: bool = False
                 ) -> torch.Tensor:
        """``fp8_activations``: a call of more than FP8A_ROWS rows quantises its rows to e4m3 and runs the W8A8 GEMM
        (``pli_hip.linear_fp8a``; no workspace); fewer rows, and the default, take the W8A16 path"""
        lead = x.shape[:-1]
        if fp8_activations and x.numel() // max(x.shape[-1], 1) > FP8A_ROWS:
            x2 = x.reshape(-1, x.shape[-1])
            linear = pli_hip.linear_fp8a if x.is_cuda else linear_fp8a_cpu
            y = linear(x2, self.codes, self.scale)
            return y.view(*lead, self.out_features)
        if not x.is_cuda:
            return F.linear(x, self.dequantized(x.dtype))
        y = pli_hip.linear_fp8w(x.reshape(-1, x.shape[-1]), self.codes, self.scale, workspace=workspace)
        return y.view(*lead, self.out_features)


class Fp8Block(nn.Module):
    def __init__(self, block, pow2_scales: bool, fp8_activations: bool = False):
        super().__init__()
        self.fp8_activations = bool(fp8_activations)
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
        fa = self.fp8_activations
        h = x + self._attn_cpu(self.input_norm(x), cache)
        n2 = self.post_attn_norm(h)
        g = F.silu(self.gate(n2, fp8_activations=fa)) * self.up(n2, fp8_activations=fa)
        return h + self.down(g, fp8_activations=fa)

    def _attn_cpu(self, x: torch.Tensor, cache: LayerKVCache | None) -> torch.Tensor:
        B, S, _ = x.shape
        nq, nk = self.num_heads * self.head_dim, self.num_kv_heads * self.head_dim
        if self.fp8_activations and B * S > FP8A_ROWS:
            qkv = self.qkv(x, fp8_activations=True)
            q = qkv[..., :nq].reshape(B, S, self.num_heads, self.head_dim)
            k = qkv[..., nq:nq + nk].reshape(B, S, self.num_kv_heads, self.head_dim)
            v = qkv[..., nq + nk:].reshape(B, S, self.num_kv_heads, self.head_dim)
        else:
            q = F.linear(x, self.qkv.dequantized(x.dtype, slice(0, nq))).view(B, S, self.num_heads, self.head_dim)
            k = F.linear(x, self.qkv.dequantized(x.dtype, slice(nq, nq + nk))).view(B, S, self.num_kv_heads, self.head_dim)
            v = F.linear(x, self.qkv.dequantized(x.dtype, slice(nq + nk, None))).view(B, S, self.num_kv_heads, self.head_dim)
        if cache is not None:
            cache.update(k, v)
            k_buf, v_buf, n_kv = cache.k, cache.v, cache.seq_len
        else:
            k_buf, v_buf, n_kv = k, v, S
        return self.o_proj(attend_cached(q, k_buf, v_buf, n_kv).reshape(B, S, self.hidden_dim),
                           fp8_activations=self.fp8_activations)

    # ---- device path: (x, pending FFN output) -> (residual stream, pending FFN output)
    def forward_gpu(self, x: torch.Tensor, pending: torch.Tensor | None, cache: LayerKVCache | None,
                    ws: torch.Tensor | None) -> tuple[torch.Tensor, torch.Tensor]:
        B, S, _ = x.shape
        fa = self.fp8_activations and B * S > FP8A_ROWS  # W8A8: quantise + gemm_fp8 per linear, no workspace
        if pending is None:
            n1 = pli_hip.rmsnorm(x, self.input_norm.weight, self.input_norm.eps)
        else:
            x, n1 = pli_hip.rmsnorm(pending, self.input_norm.weight, self.input_norm.eps, residual=x)
        nq, nk = self.num_heads * self.head_dim, self.num_kv_heads * self.head_dim
        qkv = self.qkv(n1, ws, fa)
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
        a = self.o_proj(o.reshape(B, S, self.hidden_dim), ws, fa)
        h, n2 = pli_hip.rmsnorm(a, self.post_attn_norm.weight, self.post_attn_norm.eps, residual=x)
        if fa:
            # one quantisation of the rows, two GEMMs, the elementwise product (no fused SwiGLU epilogue here)
            n8, ns = pli_hip.quantize_rows_fp8(n2.reshape(B * S, -1))
            gate = pli_hip.gemm_fp8(n8, ns, self.gate.codes, self.gate.scale, out_dtype=x.dtype)
            up = pli_hip.gemm_fp8(n8, ns, self.up.codes, self.up.scale, out_dtype=x.dtype)
            return h, self.down(F.silu(gate) * up, ws, True).view(B, S, self.hidden_dim)
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

    def __init__(self, model: CachedTransformerModel, pow2_scales: bool = False, fused_decode: bool = False,
                 fp8_activations: bool = False):
        super().__init__()
        self.fused_decode = bool(fused_decode)
        self.fp8_activations = bool(fp8_activations)
        self.embed, self.norm = model.embed, model.norm
        self.layers = nn.ModuleList([Fp8Block(b, pow2_scales, self.fp8_activations) for b in model.layers])
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
        unfused 7-launch layer.  fp8 activations: ``from_model(...).with_fp8_activations()``"""
        return cls(model, pow2_scales, fused_decode)

    def with_fp8_activations(self, on: bool = True) -> "Fp8WeightModel":
        """Switch the W8A8 option (also the constructor's ``fp8_activations``) and return the model: when on, every
        linear of a call with more than 16 rows (prefill, large batches) quantises its input rows to e4m3 and runs
        the W8A8 GEMM on the scaled MFMA (``pli_hip.linear_fp8a``) in place of widen + the 16-bit GEMM, and needs no
        workspace; calls of at most 16 rows are untouched.  Off, the default, every path is as without the option."""
        self.fp8_activations = bool(on)
        for b in self.layers:
            b.fp8_activations = self.fp8_activations
        return self

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
            return self.lm_head(self.norm(x), fp8_activations=self.fp8_activations)
        if self._fused_decode_ok(x, caches):
            pending = None
            for i, layer in enumerate(self.layers):
                x, pending = layer.decode_fused(x, pending, caches[i])
            caches[0].pos.add_(input_ids.shape[1])
            return pli_hip.rms_linear_fp8w(pending, self.norm.weight, self.norm.eps, self.lm_head.codes,
                                           self.lm_head.scale, residual=x)
        rows = x.shape[0] * x.shape[1]
        fa = self.fp8_activations and rows > FP8A_ROWS
        ws = None if fa else self._workspace(rows, x.dtype, x.device)
        pending = None
        for i, layer in enumerate(self.layers):
            x, pending = layer.forward_gpu(x, pending, caches[i] if caches is not None else None, ws)
        if caches is not None and caches[0].pos is not None:
            caches[0].pos.add_(input_ids.shape[1])  # one length shared by every layer
        if pending is None:  # no layers
            xn = pli_hip.rmsnorm(x, self.norm.weight, self.norm.eps)
        else:
            _, xn = pli_hip.rmsnorm(pending, self.norm.weight, self.norm.eps, residual=x)
        return self.lm_head(xn, ws, fa)
