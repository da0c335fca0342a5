"""MoE layer over MXFP4 expert weights (W4A8) -- the quantised sibling of ``ch09/moe_layer.py``'s ``MoELayer``.

``Mxfp4MoELayer.from_layer(moe_layer)`` quantises every expert's w1 / w3 / w2 with ``quantize_weight_mxfp4`` (4.25
bits per weight) and keeps the router as it is.  On a ROCm device the forward pass is

1. router logits on ``pli_gemm`` and ``pli_moe_route`` (as ``MoELayer``);
2. ``quantize_rows_fp8(x)``: one e4m3 row and one fp32 scale per token;
3. ``pli_gemm_grouped_mxfp4`` with the W1 / W3 tables: silu(x W1^T) * (x W3^T) per expert, the token rows read
   through the gather table;
4. ``quantize_rows_fp8(h)``;
5. ``pli_gemm_grouped_mxfp4`` with the W2 tables;
6. ``pli_moe_combine``.

On the CPU, and for shapes the grouped kernel's route does not take, the same arithmetic runs in torch over
``dequantize_weight_mxfp4`` and the torch form of the row quantiser: fp32 sums, the row scale after the sum, SiLU and
product in fp32, one rounding per stage.  ``MoELayer`` itself is unchanged.

``from_layer(..., split_decode=True)`` is for decode: with at most 32 sorted rows (16 tokens at top-2) both grouped
calls get one cached workspace and run ``pli_gemm_grouped_mxfp4_ws``, which splits every expert's K over workgroups.
Above 32 rows, on the CPU and with the option off (the default) nothing changes.

``from_layer(..., activations="mxfp4")`` (W4A4, an explicit opt-in for prefill-sized batches) replaces steps 2-5 with
``quantize_rows_mxfp4(x)`` -> ``pli_gemm_grouped_mxfp4_a4`` with the W1 / W3 tables -> ``quantize_rows_mxfp4(h)`` ->
``pli_gemm_grouped_mxfp4_a4`` with the W2 tables; it needs hidden_dim and expert_dim to be multiples of 256, and the
torch form runs the same arithmetic through ``_quantize_rows_mxfp4_torch``.  ``split_decode`` applies to the fp8 path
only: with ``"mxfp4"`` a call of at most 32 rows runs the plain W4A4 kernel.  The default ``"fp8"`` is the path above.
"""
from __future__ import annotations

import torch
import torch.nn as nn

import pli_hip

from .moe_layer import MoEConfig, MoELayer, Router


class Mxfp4MoELayer(nn.Module):
    def __init__(self, config: MoEConfig, router: Router, w1, w3, w2):
        """w1 / w3 / w2: per expert (codes uint8 [n, k / 2], exps uint8 [n, k / 32])"""
        super().__init__()
        self.config = config
        self.router = router
        for name, ws in (("w1", w1), ("w3", w3), ("w2", w2)):
            for e, (codes, exps) in enumerate(ws):
                self.register_buffer(f"{name}_codes_{e}", codes)
                self.register_buffer(f"{name}_exps_{e}", exps)
        self._tables = None  # (pointer key, w1 tables, w3 tables, w2 tables)
        self.split_decode = False  # up to SPLIT_ROWS sorted rows: both grouped calls split K over a cached workspace
        self._workspace = None
        self.activations = "fp8"  # "mxfp4": both grouped calls take MXFP4 rows (W4A4)

    SPLIT_ROWS = 32  # pli_gemm_grouped_mxfp4_ws's row bound

    @classmethod
    def from_layer(cls, layer: MoELayer, dtype: torch.dtype = torch.bfloat16, split_decode: bool = False,
                   activations: str = "fp8") -> "Mxfp4MoELayer":
        """``activations``: "fp8" (W4A8, the default) or "mxfp4" (W4A4); ``split_decode`` applies to "fp8" only: with
        "mxfp4" a call of at most SPLIT_ROWS rows runs the plain W4A4 kernel"""
        if activations not in ("fp8", "mxfp4"):
            raise ValueError(f"activations must be 'fp8' or 'mxfp4', got {activations!r}")
        q = lambda lin: pli_hip.quantize_weight_mxfp4(lin.weight, dtype)  # noqa: E731
        new = cls(layer.config, layer.router, [q(e.w1) for e in layer.experts], [q(e.w3) for e in layer.experts],
                  [q(e.w2) for e in layer.experts])
        new.split_decode = split_decode
        new.activations = activations
        return new

    def _split_workspace(self, rows: int, device) -> torch.Tensor | None:
        """one workspace for both grouped calls, sized for SPLIT_ROWS rows over the larger of the two; None above
        SPLIT_ROWS rows and with the option off: the plain calls"""
        if not self.split_decode or rows > self.SPLIT_ROWS:
            return None
        if self._workspace is None or self._workspace.device != device:
            c = self.config
            need = max(pli_hip.gemm_grouped_mxfp4_workspace_bytes(c.num_experts, self.SPLIT_ROWS, n, k, swiglu=sw)
                       for n, k, sw in ((c.expert_dim, c.hidden_dim, True), (c.hidden_dim, c.expert_dim, False)))
            self._workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=device)
        return self._workspace

    def _weights(self, name: str):
        return [(getattr(self, f"{name}_codes_{e}"), getattr(self, f"{name}_exps_{e}"))
                for e in range(self.config.num_experts)]

    def _weight_tables(self):
        ws = [self._weights(n) for n in ("w1", "w3", "w2")]
        key = tuple(t.data_ptr() for w in ws for pair in w for t in pair)
        if self._tables is None or self._tables[0] != key:
            self._tables = (key, *(pli_hip.mxfp4_weight_tables(w) for w in ws))
        return self._tables[1:]

    def _grouped_ok(self, x: torch.Tensor) -> bool:
        c = self.config
        step = 256 if self.activations == "mxfp4" else 128  # the K-step of the grouped kernel's route
        return (x.dtype in (torch.bfloat16, torch.float16) and c.hidden_dim % step == 0 and c.expert_dim % step == 0
                and c.num_experts <= 64 and c.num_experts_per_tok <= 8 and c.num_experts % 8 == 0)

    def _forward_hip(self, x_flat: torch.Tensor) -> torch.Tensor:
        c = self.config
        T, k = x_flat.shape[0], c.num_experts_per_tok
        logits = self.router._logits(x_flat)
        w, _, pos, gather, offsets = pli_hip.moe_route(logits, k, c.normalize_expert_weights)
        t1, t3, t2 = self._weight_tables()
        rows = T * k
        if self.activations == "mxfp4":
            h = pli_hip.gemm_grouped_mxfp4_a4(*pli_hip.quantize_rows_mxfp4(x_flat), gather, t1, offsets, rows,
                                              c.expert_dim, c.hidden_dim, up_tables=t3, out_dtype=x_flat.dtype)
            y = pli_hip.gemm_grouped_mxfp4_a4(*pli_hip.quantize_rows_mxfp4(h), None, t2, offsets, rows, c.hidden_dim,
                                              c.expert_dim, out_dtype=x_flat.dtype)
            return pli_hip.moe_combine(y, pos, w, T)
        ws = self._split_workspace(rows, x_flat.device)
        x8, xs = pli_hip.quantize_rows_fp8(x_flat)
        h = pli_hip.gemm_grouped_mxfp4(x8, xs, gather, t1, offsets, rows, c.expert_dim, c.hidden_dim, up_tables=t3,
                                       out_dtype=x_flat.dtype, workspace=ws)
        h8, hs = pli_hip.quantize_rows_fp8(h)
        y = pli_hip.gemm_grouped_mxfp4(h8, hs, None, t2, offsets, rows, c.hidden_dim, c.expert_dim,
                                       out_dtype=x_flat.dtype, workspace=ws)
        return pli_hip.moe_combine(y, pos, w, T)

    def _route_torch(self, x_flat: torch.Tensor):
        """pli_moe_route's rule in torch ops: fp32 softmax of the logits, top-k with ties to the lowest expert,
        fp32 renormalisation"""
        c = self.config
        probs = torch.softmax(self.router.gate(x_flat).float(), dim=-1)
        top, idx = torch.sort(probs, dim=-1, descending=True, stable=True)
        top, idx = top[:, :c.num_experts_per_tok], idx[:, :c.num_experts_per_tok]
        return (top / top.sum(dim=-1, keepdim=True) if c.normalize_expert_weights else top), idx

    def _forward_torch(self, x_flat: torch.Tensor, trace: list | None = None) -> torch.Tensor:
        """the device path's arithmetic in torch ops, per (token, slot) instead of per sorted row; ``trace`` collects
        per (slot, expert) the token rows, their routing weights, the dequantised h, the dequantised W2 and y"""
        c, dt = self.config, x_flat.dtype
        weights, indices = self._route_torch(x_flat)
        deq = pli_hip.dequantize_weight_mxfp4

        def lin(codes8, scale, pair):  # fp32 sum of the exact products, the row scale after it
            return (codes8.float() @ deq(*pair).t()) * scale[:, None]

        if self.activations == "mxfp4":  # the rows' values with their block scales, the row scale kept apart
            def quant(t):
                codes, exps, scale = pli_hip._quantize_rows_mxfp4_torch(t)
                return deq(codes, exps), scale
        else:
            quant = pli_hip._quantize_rows_fp8_torch
        x8, xs = quant(x_flat)
        w1, w3, w2 = (self._weights(n) for n in ("w1", "w3", "w2"))
        out = torch.zeros(x_flat.shape, dtype=torch.float32, device=x_flat.device)
        for kk in range(c.num_experts_per_tok):  # pli_moe_combine's order: fp32 fma over the slots in turn
            y = torch.zeros_like(out)
            for e in range(c.num_experts):
                rows = (indices[:, kk] == e).nonzero().flatten()
                if rows.numel() == 0:
                    continue
                g, u = lin(x8[rows], xs[rows], w1[e]), lin(x8[rows], xs[rows], w3[e])
                h8, hs = quant((g / (1 + torch.exp(-g)) * u).to(dt))
                y[rows] = lin(h8, hs, w2[e]).to(dt).float()
                if trace is not None:
                    trace.append((rows, weights[rows, kk], h8.float() * hs[:, None], deq(*w2[e]), y[rows]))
            out = torch.addcmul(out, weights[:, kk:kk + 1], y)
        return out.to(dt)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        batch_size, seq_len, hidden_dim = x.shape
        x_flat = x.reshape(-1, hidden_dim)
        if x.is_cuda and self._grouped_ok(x):
            y = self._forward_hip(x_flat.contiguous())
        else:
            y = self._forward_torch(x_flat)
        return y.view(batch_size, seq_len, hidden_dim)


if __name__ == "__main__":
    cfg = MoEConfig(hidden_dim=256, expert_dim=512, num_experts=8, num_experts_per_tok=2)
    moe = MoELayer(cfg).bfloat16()
    x = torch.randn(2, 16, 256).bfloat16()
    if torch.cuda.is_available():
        moe, x = moe.cuda(), x.cuda()
    y = moe(x).float()
    for act in ("fp8", "mxfp4"):
        yq = Mxfp4MoELayer.from_layer(moe, activations=act)(x).float()
        print(f"bf16 layer vs MXFP4 experts, {act} rows: rms {float((y - yq).pow(2).mean().sqrt()):.4f} of "
              f"{float(y.pow(2).mean().sqrt()):.4f}")
