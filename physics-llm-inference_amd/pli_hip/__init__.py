"""ctypes binding of ``libpli_hip.so`` (the C ABI declared in ``include/pli.h``).

Every wrapper takes torch tensors that already live on a ROCm device, passes
raw ``data_ptr()`` values plus sizes/strides and the current HIP stream across
the C ABI, and raises ``PliError`` on a non-zero status.  There is no CPU or
torch fallback in here: if the library is missing or a tensor is not on the
GPU, the call fails loudly.
"""
from __future__ import annotations

import ctypes
import os

import torch

__all__ = [
    "PliError", "lib", "library_path", "available", "DTYPE_CODE",
    "flash_attn_fwd", "gemv", "gemm", "gemm_f32out", "scale_copy", "mfma_probe", "hbm_read_probe", "softmax_rows",
    "online_softmax_with_output", "sample",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
# PLI_HIP_LIB: an alternate in-tree build (A/B tooling); default the package .so
_LIB_PATH = os.environ.get("PLI_HIP_LIB") or os.path.join(_HERE, "libpli_hip.so")
_lib = None

DTYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}

_c_int, _c_i64, _c_f32, _vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p

# name -> argtypes, mirroring include/pli.h
_SIGS = {
    "pli_version": [],
    "pli_last_error": [],
    "pli_last_route": [],
    "pli_debug_sync": [_c_int],
    "pli_flash_attn_fwd": [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                           ctypes.POINTER(_c_i64), _c_f32, _c_int, _c_int, _vp],
    "pli_gemv": [_vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _vp],
    "pli_gemm": [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _c_int,
                 _c_int, _vp],
    "pli_gemm_workspace_size": [_c_int, _c_int, _c_int, _c_int, _c_int],
    "pli_gemm_ws": [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _c_int,
                    _c_int, _vp, ctypes.c_size_t, _vp],
    "pli_gemm_swiglu_workspace_size": [_c_int, _c_int, _c_int, _c_int],
    "pli_gemm_swiglu_ws": [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_i64, _c_i64, _c_i64,
                           _c_i64, _c_int, _vp, ctypes.c_size_t, _vp],
    "pli_gemm_swiglu_ws_variant": [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_i64, _c_i64,
                                   _c_i64, _c_i64, _c_int, _vp, ctypes.c_size_t, _vp, _c_int],
    "pli_gemm_swiglu": [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_i64, _c_i64, _c_i64,
                        _c_i64, _c_int, _vp],
    "pli_rmsnorm": [_vp, _vp, _vp, _vp, _vp, _c_i64, _c_int, _c_i64, _c_i64, _c_i64, _c_i64,
                    _c_f32, _c_int, _vp],
    "pli_gemm_multi_nt": [_vp, _c_i64, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                          _vp, _c_int, _c_int, _vp],
    "pli_rms_gemm_nt": [_vp, _c_i64, _vp, _c_i64, _vp, _c_f32, _vp, _c_i64, _c_int, _c_int, _c_int,
                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _vp],
    "pli_moe_route": [_vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp,
                      _vp, _vp, _vp],
    "pli_gemm_grouped": [_vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_i64,
                         _c_i64, _c_i64, _c_int, _vp],
    "pli_gemm_grouped_variant": [_vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int,
                                 _c_i64, _c_i64, _c_i64, _c_int, _vp, _c_int],
    "pli_moe_combine": [_vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _vp],
    "pli_scale_copy": [_vp, _vp, _c_i64, _c_int, _vp],
    "pli_gemm_naive": [_vp, _vp, _vp, _c_int, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _vp],
    "pli_gemm_f32out": [_vp, _vp, _vp, _c_int, _c_int, _c_int, _c_i64, _c_i64, _c_int, _vp],
    "pli_mfma_probe": [_vp, _vp, _c_int, _c_int, _c_int, _vp],
    "pli_hbm_read_probe": [_vp, _c_i64, _vp, _c_int, _c_int, _vp],
    "pli_softmax_rows": [_vp, _vp, _c_i64, _c_int, _c_int, _vp],
    "pli_online_softmax_with_output": [_vp, _vp, _vp, _vp, _c_i64, _c_int, _c_int, _c_int, _vp],
    "pli_attn_decode_workspace_size": [_c_int] * 6,
    "pli_kv_append": [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int,
                      ctypes.POINTER(_c_i64), _vp, _c_int, _vp],
    "pli_attn_decode_dev": [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                            ctypes.POINTER(_c_i64), _c_f32, _c_int, _vp, _c_int, _vp,
                            ctypes.c_size_t, _c_int, _vp],
    "pli_attn_decode": [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                        ctypes.POINTER(_c_i64), _c_f32, _c_int, _vp, ctypes.c_size_t, _c_int, _vp],
    "pli_attn_decode_paged_workspace_size": [_c_int] * 6,
    "pli_attn_decode_paged": [_vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int,
                              _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_i64), _c_f32, _c_int,
                              _c_int, _vp, ctypes.c_size_t, _c_int, _vp],
    "pli_kv_append_paged": [_vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int,
                            _c_int, _c_int, ctypes.POINTER(_c_i64), _c_int, _vp],
    "pli_attn_varlen_paged": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int,
                              _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_i64), _c_f32, _c_int, _c_int,
                              _vp],
    "pli_kv_append_varlen_paged": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int,
                                   _c_int, _c_int, ctypes.POINTER(_c_i64), _c_int, _vp],
    # 1-byte (fp8 e4m3) pools: the 16-bit signatures plus k_scale, v_scale after seq_lens
    "pli_attn_decode_paged_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int,
                                  _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_i64), _c_f32, _c_int,
                                  _c_int, _vp, ctypes.c_size_t, _c_int, _vp],
    "pli_kv_append_paged_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int,
                                _c_int, _c_int, ctypes.POINTER(_c_i64), _c_int, _vp],
    "pli_attn_varlen_paged_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int,
                                  _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_i64), _c_f32, _c_int,
                                  _c_int, _vp],
    "pli_kv_append_varlen_paged_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int,
                                       _c_int, _c_int, _c_int, ctypes.POINTER(_c_i64), _c_int, _vp],
    # split-K packed calls: the plain signatures plus split_keys, workspace, workspace_bytes before the stream
    "pli_attn_varlen_paged_workspace_size": [_c_int] * 7,
    "pli_attn_varlen_paged_split_plan": [_c_int] * 7 + [ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)],
    "pli_attn_varlen_paged_ws": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int,
                                 _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_i64), _c_f32, _c_int, _c_int,
                                 _c_int, _vp, ctypes.c_size_t, _vp],
    "pli_attn_varlen_paged_fp8_ws": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int,
                                     _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_i64), _c_f32, _c_int,
                                     _c_int, _c_int, _vp, ctypes.c_size_t, _vp],
    # weight-only fp8 linear (W8A16): codes + one fp32 scale per output row
    "pli_gemv_fp8w": [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _vp],
    "pli_linear_fp8w_workspace_size": [_c_int] * 4,
    "pli_linear_fp8w": [_vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _c_int, _vp,
                        ctypes.c_size_t, _vp],
    "pli_linear_swiglu_fp8w_workspace_size": [_c_int] * 4,
    "pli_linear_swiglu_fp8w": [_vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _c_i64,
                               _c_int, _vp, ctypes.c_size_t, _vp],
    # pli_rms_gemm_nt with (w8, w_scale, wu8, wu_scale) pointer arrays in place of (w, w_up)
    "pli_rms_gemm_nt_fp8w": [_vp, _c_i64, _vp, _c_i64, _vp, _c_f32, _vp, _c_i64, _c_int, _c_int, _c_int,
                             _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _vp],
    # fp8 activations (W8A8): the row quantiser and the codes x codes NT GEMM
    "pli_quantize_rows_fp8": [_vp, _c_i64, _vp, _c_i64, _vp, _c_int, _c_int, _c_int, _vp],
    "pli_gemm_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _c_int, _vp],
    # next-token sampling: logits, ld, rows, vocab, dtype, temperature, top_k, top_p, uniforms, seed, offset_dev,
    # offset_add, tokens, ld_tokens, workspace, workspace_bytes, stream
    "pli_sample_workspace_size": [_c_int] * 3,
    "pli_sample": [_vp, _c_i64, _c_int, _c_int, _c_int, _c_f32, _c_int, _c_f32, _vp, ctypes.c_uint64, _vp, _c_i64,
                   _vp, _c_i64, _vp, ctypes.c_size_t, _vp],
    # tuning entry points (include/pli.h tuning section): explicit kernel variant
    "pli_flash_attn_fwd_variant": [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int,
                                   _c_int, ctypes.POINTER(_c_i64), _c_f32, _c_int, _c_int, _vp,
                                   _c_int],
    "pli_gemv_variant": [_vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _vp, _c_int],
    "pli_gemm_variant": [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_i64, _c_i64, _c_i64,
                         _c_int, _c_int, _vp, _c_int],
    "pli_gemm_ws_variant": [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_i64, _c_i64, _c_i64,
                            _c_int, _c_int, _vp, ctypes.c_size_t, _vp, _c_int],
    "pli_attn_decode_variant": [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                                ctypes.POINTER(_c_i64), _c_f32, _c_int, _vp, ctypes.c_size_t,
                                _c_int, _vp, _c_int, _c_int],
}


class PliError(RuntimeError):
    """A libpli_hip entry point returned a non-zero status."""


def library_path() -> str:
    return _LIB_PATH


def lib() -> ctypes.CDLL:
    """Load libpli_hip.so (after torch, so both share torch's HIP runtime)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise PliError(
                f"{_LIB_PATH} is not built; run `python physics-llm-inference_amd/build.py` "
                "(or __graft_entry__.build())")
        L = ctypes.CDLL(_LIB_PATH)
        for name, argtypes in _SIGS.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = (ctypes.c_char_p if name in ("pli_version", "pli_last_error", "pli_last_route") else
                          ctypes.c_size_t if name.endswith("_workspace_size") else _c_int)
        _lib = L
    return _lib


def available() -> bool:
    """True when the library loads AND a ROCm device is visible."""
    try:
        lib()
    except (PliError, OSError):
        return False
    return torch.cuda.is_available()


def last_route() -> str:
    """the kernels this thread's last library call launched ('+'-separated;
    pli_last_route)"""
    return lib().pli_last_route().decode()


def debug_sync(mode: int = -1) -> bool:
    """the library's synchronous debug mode (pli_debug_sync; PLI_SYNC=1 in the
    environment turns it on at load): mode 1 / 0 sets it, -1 only queries;
    returns the previous state.  When on, every launch is synchronised and
    checked, and a failing kernel's name is in the raised PliError."""
    return bool(lib().pli_debug_sync(int(mode)))


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().pli_last_error().decode(errors="replace")
        raise PliError(f"{what} failed with status {rc}: {msg}")


def _dtype_code(t: torch.Tensor) -> int:
    try:
        return DTYPE_CODE[t.dtype]
    except KeyError:
        raise PliError(f"unsupported dtype {t.dtype} (HIP path supports fp32/fp16/bf16)") from None


def _require_gpu(*ts: torch.Tensor) -> torch.device:
    dev = ts[0].device
    for t in ts:
        if not t.is_cuda:
            raise PliError("HIP path called with a CPU tensor")
        if t.device != dev:
            raise PliError(f"tensors on different devices: {t.device} vs {dev}")
        if t.dtype != ts[0].dtype:
            raise PliError(f"mixed dtypes {t.dtype} vs {ts[0].dtype}")
    return dev


def _check_out(out: torch.Tensor, ref: torch.Tensor, shape: tuple, what: str) -> None:
    """A caller-supplied output: same device and dtype as ``ref``, exactly
    ``shape``, unit inner stride, rows not overlapping (the kernels write
    ``shape[0]`` rows of ``shape[-1]`` elements at the row stride)."""
    _require_gpu(ref, out)
    if tuple(out.shape) != tuple(shape):
        raise PliError(f"{what}: out has shape {tuple(out.shape)}, expected {tuple(shape)}")
    if out.dim() > 0 and out.stride(-1) != 1:
        raise PliError(f"{what}: out needs a unit inner stride, got strides {out.stride()}")
    if out.dim() == 2 and out.shape[0] > 1 and out.stride(0) < out.shape[1]:
        raise PliError(f"{what}: out rows overlap (row stride {out.stride(0)} < {out.shape[1]})")


def _stream(dev: torch.device) -> int:
    # raw hipStream_t of the current stream (cheaper than building a Stream object)
    return torch._C._cuda_getCurrentRawStream(dev.index)


class _on_device:
    """Device guard that costs nothing when ``dev`` is already current."""

    __slots__ = ("dev", "prev")

    def __init__(self, dev: torch.device):
        self.dev, self.prev = dev, None

    def __enter__(self):
        cur = torch.cuda.current_device()
        if self.dev.index is not None and cur != self.dev.index:
            self.prev = cur
            torch.cuda.set_device(self.dev.index)

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)


def _ptr(t: torch.Tensor | None):
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------ attention
def flash_attn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float | None = None,
                   causal: bool = False, out: torch.Tensor | None = None,
                   variant: int | None = None) -> torch.Tensor:
    """O = softmax(Q K^T * scale [+ causal]) V on [B, H, N, D] tensors (any
    strides with a unit head_dim stride); K/V may have fewer (GQA) heads."""
    dev = _require_gpu(q, k, v)
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise PliError("flash_attn_fwd expects [B, H, N, D] tensors")
    B, H, Nq, D = q.shape
    Bk, Hkv, Nk, Dk = k.shape
    if (Bk, Dk) != (B, D) or tuple(v.shape) != tuple(k.shape):
        raise PliError(f"shape mismatch q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)}")
    if H % Hkv != 0:
        raise PliError(f"heads {H} not a multiple of kv heads {Hkv}")
    q, k, v = (t if t.stride(-1) == 1 else t.contiguous() for t in (q, k, v))
    if out is None:
        out = torch.empty_like(q, memory_format=torch.contiguous_format)
    _require_gpu(q, out)
    if tuple(out.shape) != tuple(q.shape) or out.stride(-1) != 1:
        raise PliError("bad output tensor")
    if scale is None:
        scale = D ** -0.5
    st = (_c_i64 * 12)(*(int(x) for t in (q, k, v, out) for x in t.stride()[:3]))
    args = (_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, H, Hkv, Nq, Nk, D, st, float(scale),
            int(bool(causal)), _dtype_code(q), _stream(dev))
    with _on_device(dev):
        if variant is None:
            rc = lib().pli_flash_attn_fwd(*args)
        else:
            rc = lib().pli_flash_attn_fwd_variant(*args, int(variant))
    _check(rc, "pli_flash_attn_fwd")
    return out


# ------------------------------------------------------- decode attention
def attn_decode_workspace_bytes(B: int, H: int, Hkv: int, Sq: int, n_kv: int, D: int) -> int:
    return int(lib().pli_attn_decode_workspace_size(B, H, Hkv, Sq, n_kv, D))


def attn_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, n_kv: int,
                scale: float | None = None, causal: bool = True,
                out: torch.Tensor | None = None, variant: int | None = None,
                target_wgs: int = 0) -> torch.Tensor:
    """Attention of the new tokens over a KV cache, in the cache layout of
    ch02/kv_cache.py:25-35: q [B, Sq, Hq, D], k/v caches [B, S_max, Hkv, D]
    of which the first n_kv positions are valid (the current token's K/V
    already appended).  Returns [B, Sq, Hq, D].  causal masks bottom-right
    (ch02/kv_cache.py:91-95); with Sq == 1 it changes nothing."""
    dev = _require_gpu(q, k_cache, v_cache)
    if q.dim() != 4 or k_cache.dim() != 4 or v_cache.dim() != 4:
        raise PliError("attn_decode expects q [B, Sq, Hq, D] and caches [B, S, Hkv, D]")
    B, Sq, H, D = q.shape
    Bk, S_max, Hkv, Dk = k_cache.shape
    if (Bk, Dk) != (B, D) or tuple(v_cache.shape) != tuple(k_cache.shape):
        raise PliError(f"shape mismatch q{tuple(q.shape)} k{tuple(k_cache.shape)} "
                       f"v{tuple(v_cache.shape)}")
    if H % Hkv != 0:
        raise PliError(f"heads {H} not a multiple of kv heads {Hkv}")
    if not 0 <= n_kv <= S_max:
        raise PliError(f"n_kv {n_kv} outside the cache [0, {S_max}]")
    q, k_cache, v_cache = (t if t.stride(-1) == 1 else t.contiguous() for t in (q, k_cache, v_cache))
    if out is None:
        out = torch.empty((B, Sq, H, D), device=q.device, dtype=q.dtype)
    _require_gpu(q, out)
    if tuple(out.shape) != (B, Sq, H, D) or out.stride(-1) != 1:
        raise PliError("bad output tensor")
    if scale is None:
        scale = D ** -0.5
    # [b, h, n] strides of the [B, N, H, D] tensors
    st = (_c_i64 * 12)(*(int(x) for t in (q, k_cache, v_cache, out)
                         for x in (t.stride(0), t.stride(2), t.stride(1))))
    ws_bytes = int(lib().pli_attn_decode_workspace_size(B, H, Hkv, Sq, n_kv, D))
    if target_wgs:  # tuning: room for the finest split (one 128-key chunk per block)
        ws_bytes = B * Hkv * -(-n_kv // 128) * Sq * (H // Hkv) * (D + 2) * 4
    ws = torch.empty(max(ws_bytes // 4, 1), device=q.device, dtype=torch.float32)
    args = (_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(out), B, H, Hkv, Sq, int(n_kv), D, st,
            float(scale), int(bool(causal)), _ptr(ws), ws_bytes, _dtype_code(q), _stream(dev))
    with _on_device(dev):
        if variant is None and not target_wgs:
            rc = lib().pli_attn_decode(*args)
        else:
            rc = lib().pli_attn_decode_variant(*args, -1 if variant is None else int(variant),
                                               int(target_wgs))
    _check(rc, "pli_attn_decode")
    return out


def kv_append(k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor,
              v_cache: torch.Tensor, pos: torch.Tensor) -> None:
    """Write [B, T, Hkv, D] K/V into [B, S, Hkv, D] caches at rows pos[0] +
    (0..T-1), pos an int32 device tensor (graph-replayable KVCache.update)."""
    dev = _require_gpu(k_new, v_new, k_cache, v_cache)
    if pos.dtype != torch.int32 or not pos.is_cuda:
        raise PliError("pos must be an int32 device tensor")
    B, T, Hkv, D = k_new.shape
    if tuple(v_new.shape) != tuple(k_new.shape) or k_cache.shape[0] != B or \
            tuple(k_cache.shape[2:]) != (Hkv, D) or tuple(v_cache.shape) != tuple(k_cache.shape):
        raise PliError(f"kv_append shape mismatch new{tuple(k_new.shape)} cache{tuple(k_cache.shape)}")
    st = (_c_i64 * 12)(*(int(x) for t in (k_new, k_cache, v_cache, v_new)
                         for x in (t.stride(0), t.stride(2), t.stride(1))))
    with _on_device(dev):
        rc = lib().pli_kv_append(_ptr(k_new), _ptr(v_new), _ptr(k_cache), _ptr(v_cache), B, T, Hkv,
                                 D, k_cache.shape[1], st, _ptr(pos), _dtype_code(k_new), _stream(dev))
    _check(rc, "pli_kv_append")


def attn_decode_dev(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                    n_kv_dev: torch.Tensor, n_kv_add: int = 0, n_kv_max: int | None = None,
                    scale: float | None = None, causal: bool = True,
                    out: torch.Tensor | None = None, workspace: torch.Tensor | None = None
                    ) -> torch.Tensor:
    """attn_decode with the valid length n_kv_dev[0] + n_kv_add read on the
    device (graph-replayable); the grid is planned for n_kv_max (default: the
    cache capacity)."""
    dev = _require_gpu(q, k_cache, v_cache)
    B, Sq, H, D = q.shape
    Hkv = k_cache.shape[2]
    n_max = k_cache.shape[1] if n_kv_max is None else int(n_kv_max)
    if out is None:
        out = torch.empty((B, Sq, H, D), device=q.device, dtype=q.dtype)
    if scale is None:
        scale = D ** -0.5
    st = (_c_i64 * 12)(*(int(x) for t in (q, k_cache, v_cache, out)
                         for x in (t.stride(0), t.stride(2), t.stride(1))))
    ws_bytes = int(lib().pli_attn_decode_workspace_size(B, H, Hkv, Sq, n_max, D))
    if workspace is None or workspace.numel() * 4 < ws_bytes:
        workspace = torch.empty(max(ws_bytes // 4, 1), device=q.device, dtype=torch.float32)
    with _on_device(dev):
        rc = lib().pli_attn_decode_dev(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(out), B, H, Hkv,
                                       Sq, n_max, D, st, float(scale), int(bool(causal)),
                                       _ptr(n_kv_dev), int(n_kv_add), _ptr(workspace), ws_bytes,
                                       _dtype_code(q), _stream(dev))
    _check(rc, "pli_attn_decode_dev")
    return out


# ------------------------------------------------------ paged KV cache
def attn_decode_paged_workspace_bytes(B: int, H: int, Hkv: int, Sq: int, max_kv: int, D: int) -> int:
    """fp32 split-K workspace of attn_decode_paged for sequences of up to max_kv keys"""
    return int(lib().pli_attn_decode_paged_workspace_size(B, H, Hkv, Sq, max_kv, D))


def _check_paged(what: str, x: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                 block_table: torch.Tensor, seq_lens: torch.Tensor):
    """shared checks of the paged calls: x is q or k_new [B, S, H, D], the pools
    [num_blocks, block_size, Hkv, D] views (any page stride), block_table int32
    [B, max_blocks], seq_lens int32 [B]; returns the device"""
    dev = _require_gpu(x, k_pool, v_pool)
    for name, t in (("block_table", block_table), ("seq_lens", seq_lens)):
        if not t.is_cuda or t.device != dev or t.dtype != torch.int32 or not t.is_contiguous():
            raise PliError(f"{what}: {name} must be a contiguous int32 tensor on {dev}")
    if x.dim() != 4 or k_pool.dim() != 4 or tuple(v_pool.shape) != tuple(k_pool.shape):
        raise PliError(f"{what} expects [B, S, H, D] tokens and [num_blocks, block_size, Hkv, D] pools, got "
                       f"{tuple(x.shape)} k{tuple(k_pool.shape)} v{tuple(v_pool.shape)}")
    B, D = x.shape[0], x.shape[3]
    if k_pool.shape[3] != D or block_table.dim() != 2 or block_table.shape[0] != B or tuple(seq_lens.shape) != (B,):
        raise PliError(f"{what}: shape mismatch tokens{tuple(x.shape)} pool{tuple(k_pool.shape)} "
                       f"table{tuple(block_table.shape)} seq_lens{tuple(seq_lens.shape)}")
    if any(t.stride(-1) != 1 for t in (x, k_pool, v_pool) if t.numel()):
        raise PliError(f"{what}: a unit head_dim stride is required (the pools are used in place)")
    return dev


def attn_decode_paged(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                      block_table: torch.Tensor, seq_lens: torch.Tensor, *, scale: float | None = None,
                      causal: bool = True, n_kv_add: int = 0, max_kv: int | None = None,
                      out: torch.Tensor | None = None, workspace: torch.Tensor | None = None
                      ) -> torch.Tensor:
    """Decode attention straight over a paged pool (the PagedKVCache of
    ch07/paged_memory.py:16-51): q [B, Sq, Hq, D]; k_pool / v_pool
    [num_blocks, block_size, Hkv, D] views such as k_cache[:, layer], used in
    place; block_table int32 [B, max_blocks] of page indices; sequence b
    attends over its first clamp(seq_lens[b] + n_kv_add, 0, max_kv) tokens,
    read on the device (graph-replayable).  max_kv: a host bound on every
    length, default max_blocks * block_size.  causal masks bottom-right per
    sequence.  Returns [B, Sq, Hq, D]; a row that sees no key is 0."""
    dev = _check_paged("attn_decode_paged", q, k_pool, v_pool, block_table, seq_lens)
    B, Sq, H, D = q.shape
    num_blocks, bs, Hkv, _ = k_pool.shape
    max_blocks = block_table.shape[1]
    if Hkv == 0 or H % Hkv != 0:
        raise PliError(f"heads {H} not a multiple of kv heads {Hkv}")
    cap = max_blocks * bs
    max_kv = cap if max_kv is None else int(max_kv)
    if not 0 <= max_kv <= cap:
        raise PliError(f"max_kv {max_kv} outside the table row [0, {cap}]")
    if out is None:
        out = torch.empty((B, Sq, H, D), device=q.device, dtype=q.dtype)
    _require_gpu(q, out)
    if tuple(out.shape) != (B, Sq, H, D) or (out.numel() and out.stride(-1) != 1):
        raise PliError("bad output tensor")
    if scale is None:
        scale = D ** -0.5
    st = (_c_i64 * 12)(*(int(x) for x in (q.stride(0), q.stride(2), q.stride(1),
                                          k_pool.stride(0), k_pool.stride(1), k_pool.stride(2),
                                          v_pool.stride(0), v_pool.stride(1), v_pool.stride(2),
                                          out.stride(0), out.stride(2), out.stride(1))))
    ws_bytes = int(lib().pli_attn_decode_paged_workspace_size(B, H, Hkv, Sq, max_kv, D))
    if workspace is None or workspace.numel() * workspace.element_size() < ws_bytes:
        workspace = torch.empty(max(ws_bytes // 4, 1), device=q.device, dtype=torch.float32)
    with _on_device(dev):
        rc = lib().pli_attn_decode_paged(_ptr(q), _ptr(k_pool), _ptr(v_pool), _ptr(out), _ptr(block_table),
                                         _ptr(seq_lens), B, H, Hkv, Sq, D, bs, num_blocks, max_blocks, max_kv,
                                         st, float(scale), int(bool(causal)), int(n_kv_add), _ptr(workspace),
                                         ws_bytes, _dtype_code(q), _stream(dev))
    _check(rc, "pli_attn_decode_paged")
    return out


def kv_append_paged(k_new: torch.Tensor, v_new: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                    block_table: torch.Tensor, seq_lens: torch.Tensor) -> None:
    """Write token t of k_new / v_new [B, T, Hkv, D] of sequence b to logical
    position seq_lens[b] + t of the paged pools, through block_table (positions
    past the table row are dropped).  seq_lens is not advanced: the caller adds
    T on the device (seq_lens.add_(T)), which a graph capture records too."""
    dev = _check_paged("kv_append_paged", k_new, k_pool, v_pool, block_table, seq_lens)
    _require_gpu(k_new, v_new)
    B, T, Hkv, D = k_new.shape
    if tuple(v_new.shape) != tuple(k_new.shape) or k_pool.shape[2] != Hkv or (v_new.numel() and v_new.stride(-1) != 1):
        raise PliError(f"kv_append_paged shape mismatch new{tuple(k_new.shape)} v{tuple(v_new.shape)} "
                       f"pool{tuple(k_pool.shape)}")
    num_blocks, bs = k_pool.shape[0], k_pool.shape[1]
    st = (_c_i64 * 12)(*(int(x) for x in (k_new.stride(0), k_new.stride(2), k_new.stride(1),
                                          k_pool.stride(0), k_pool.stride(1), k_pool.stride(2),
                                          v_pool.stride(0), v_pool.stride(1), v_pool.stride(2),
                                          v_new.stride(0), v_new.stride(2), v_new.stride(1))))
    with _on_device(dev):
        rc = lib().pli_kv_append_paged(_ptr(k_new), _ptr(v_new), _ptr(k_pool), _ptr(v_pool), _ptr(block_table),
                                       _ptr(seq_lens), B, T, Hkv, D, bs, num_blocks, block_table.shape[1], st,
                                       _dtype_code(k_new), _stream(dev))
    _check(rc, "pli_kv_append_paged")


# ------------------------------------- packed variable-length paged attention
def _check_varlen(what: str, x: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                  block_table: torch.Tensor, seq_lens: torch.Tensor, cu_seqlens_q: torch.Tensor):
    """the checks of _check_paged for packed tokens: x is q or k_new
    [max_tokens, H, D], cu_seqlens_q int32 [B + 1]; returns the device"""
    dev = _require_gpu(x, k_pool, v_pool)
    for name, t in (("block_table", block_table), ("seq_lens", seq_lens), ("cu_seqlens_q", cu_seqlens_q)):
        if not t.is_cuda or t.device != dev or t.dtype != torch.int32 or not t.is_contiguous():
            raise PliError(f"{what}: {name} must be a contiguous int32 tensor on {dev}")
    if x.dim() != 3 or k_pool.dim() != 4 or tuple(v_pool.shape) != tuple(k_pool.shape):
        raise PliError(f"{what} expects packed [tokens, H, D] rows and [num_blocks, block_size, Hkv, D] pools, got "
                       f"{tuple(x.shape)} k{tuple(k_pool.shape)} v{tuple(v_pool.shape)}")
    B, D = seq_lens.shape[0] if seq_lens.dim() == 1 else -1, x.shape[2]
    if (k_pool.shape[3] != D or block_table.dim() != 2 or block_table.shape[0] != B or
            tuple(cu_seqlens_q.shape) != (B + 1,)):
        raise PliError(f"{what}: shape mismatch tokens{tuple(x.shape)} pool{tuple(k_pool.shape)} "
                       f"table{tuple(block_table.shape)} seq_lens{tuple(seq_lens.shape)} "
                       f"cu_seqlens_q{tuple(cu_seqlens_q.shape)}")
    if any(t.stride(-1) != 1 for t in (x, k_pool, v_pool) if t.numel()):
        raise PliError(f"{what}: a unit head_dim stride is required (the pools are used in place)")
    return dev


def attn_varlen_paged_workspace_bytes(batch: int, max_tokens: int, heads: int, kv_heads: int, max_kv: int,
                                      head_dim: int, split_keys: int = 0) -> int:
    """bytes of workspace the split-K packed calls (attn_varlen_paged / attn_varlen_paged_fp8 with workspace=)
    need for these host arguments (pli_attn_varlen_paged_workspace_size); 0: the call is the plain call"""
    return int(lib().pli_attn_varlen_paged_workspace_size(int(batch), int(max_tokens), int(heads), int(kv_heads),
                                                          int(max_kv), int(head_dim), int(split_keys)))


def attn_varlen_paged_split_plan(batch: int, max_tokens: int, heads: int, kv_heads: int, max_kv: int, head_dim: int,
                                 split_keys: int = 0) -> tuple:
    """(span, splits_max) of the split-K packed calls for these host arguments (pli_attn_varlen_paged_split_plan)"""
    span, splits = _c_int(0), _c_int(0)
    rc = lib().pli_attn_varlen_paged_split_plan(int(batch), int(max_tokens), int(heads), int(kv_heads), int(max_kv),
                                                int(head_dim), int(split_keys), ctypes.byref(span),
                                                ctypes.byref(splits))
    _check(rc, "pli_attn_varlen_paged_split_plan")
    return span.value, splits.value


def _varlen_workspace(what: str, workspace, split_keys: int, q, k_pool, block_table, max_kv) -> int:
    """checks of the workspace= keyword, made on shapes alone and before the operands' own: a contiguous fp32
    tensor of at least the bytes the call needs, on a GPU; returns those bytes"""
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.float32 or not workspace.is_contiguous():
        raise PliError(f"{what}: workspace must be a contiguous torch.float32 tensor")
    split_keys = int(split_keys)
    if split_keys < 0 or split_keys % 64:
        raise PliError(f"{what}: split_keys {split_keys} must be 0 or a positive multiple of 64")
    if q.dim() != 3 or k_pool.dim() != 4 or block_table.dim() != 2:
        raise PliError(f"{what}: shape mismatch tokens{tuple(q.shape)} pool{tuple(k_pool.shape)} "
                       f"table{tuple(block_table.shape)}")
    cap = block_table.shape[1] * k_pool.shape[1]
    need = attn_varlen_paged_workspace_bytes(block_table.shape[0], q.shape[0], q.shape[1], k_pool.shape[2],
                                             cap if max_kv is None else int(max_kv), q.shape[2], split_keys)
    have = workspace.numel() * workspace.element_size()
    if have < need:
        raise PliError(f"{what}: workspace of {need} bytes needed, {have} given")
    if not workspace.is_cuda:
        raise PliError(f"{what}: workspace is a CPU tensor")
    if workspace.device != q.device:
        raise PliError(f"{what}: workspace on {workspace.device}, q on {q.device}")
    return need


def attn_varlen_paged(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor,
                      seq_lens: torch.Tensor, cu_seqlens_q: torch.Tensor, max_kv: int | None = None,
                      scale: float | None = None, causal: bool = True,
                      out: torch.Tensor | None = None, workspace: torch.Tensor | None = None,
                      split_keys: int = 0) -> torch.Tensor:
    """Attention of a packed, mixed batch straight over a paged pool: q
    [max_tokens, Hq, D], sequence b owning rows cu_seqlens_q[b] ..
    cu_seqlens_q[b+1] - 1 (any count, 0 included); k_pool / v_pool
    [num_blocks, block_size, Hkv, D] views used in place; block_table int32
    [B, max_blocks]; seq_lens int32 [B], each sequence's kv length with this
    step's tokens already appended (clamped to max_kv, default max_blocks *
    block_size).  causal masks bottom-right per sequence.  The three int32
    tensors are read on the device (graph-replayable).  Returns [max_tokens, Hq,
    D]; a row that sees no key is 0, rows past cu_seqlens_q[B] are not written.
    workspace: None makes the plain call; a float32 device tensor of at least
    attn_varlen_paged_workspace_bytes(...) bytes makes the split-K call
    (pli_attn_varlen_paged_ws), which cuts every tile's key range into chunks
    of split_keys keys (a multiple of 64; 0: the plan's choice)."""
    if workspace is not None:
        _varlen_workspace("attn_varlen_paged", workspace, split_keys, q, k_pool, block_table, max_kv)
    dev = _check_varlen("attn_varlen_paged", q, k_pool, v_pool, block_table, seq_lens, cu_seqlens_q)
    T, H, D = q.shape
    num_blocks, bs, Hkv, _ = k_pool.shape
    B, max_blocks = block_table.shape
    if Hkv == 0 or H % Hkv != 0:
        raise PliError(f"heads {H} not a multiple of kv heads {Hkv}")
    cap = max_blocks * bs
    max_kv = cap if max_kv is None else int(max_kv)
    if not 0 <= max_kv <= cap:
        raise PliError(f"max_kv {max_kv} outside the table row [0, {cap}]")
    if out is None:
        out = torch.empty((T, H, D), device=q.device, dtype=q.dtype)
    _require_gpu(q, out)
    if tuple(out.shape) != (T, H, D) or (out.numel() and out.stride(-1) != 1):
        raise PliError("bad output tensor")
    if scale is None:
        scale = D ** -0.5
    st = (_c_i64 * 10)(*(int(x) for x in (q.stride(0), q.stride(1),
                                          k_pool.stride(0), k_pool.stride(1), k_pool.stride(2),
                                          v_pool.stride(0), v_pool.stride(1), v_pool.stride(2),
                                          out.stride(0), out.stride(1))))
    with _on_device(dev):
        if workspace is not None:
            rc = lib().pli_attn_varlen_paged_ws(_ptr(q), _ptr(k_pool), _ptr(v_pool), _ptr(out), _ptr(cu_seqlens_q),
                                                _ptr(block_table), _ptr(seq_lens), B, T, H, Hkv, D, bs, num_blocks,
                                                max_blocks, max_kv, st, float(scale), int(bool(causal)),
                                                _dtype_code(q), int(split_keys), _ptr(workspace),
                                                workspace.numel() * workspace.element_size(), _stream(dev))
            _check(rc, "pli_attn_varlen_paged_ws")
            return out
        rc = lib().pli_attn_varlen_paged(_ptr(q), _ptr(k_pool), _ptr(v_pool), _ptr(out), _ptr(cu_seqlens_q),
                                         _ptr(block_table), _ptr(seq_lens), B, T, H, Hkv, D, bs, num_blocks,
                                         max_blocks, max_kv, st, float(scale), int(bool(causal)), _dtype_code(q),
                                         _stream(dev))
    _check(rc, "pli_attn_varlen_paged")
    return out


def kv_append_varlen_paged(k_new: torch.Tensor, v_new: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                           block_table: torch.Tensor, seq_lens: torch.Tensor, cu_seqlens_q: torch.Tensor) -> None:
    """Write packed row cu_seqlens_q[b] + i of k_new / v_new [max_tokens, Hkv,
    D] to logical position seq_lens[b] - q_len(b) + i of sequence b in the paged
    pools (negative positions and positions past the table row are dropped):
    seq_lens already counts the new tokens, so this call and attn_varlen_paged
    take the same three device tensors."""
    dev = _check_varlen("kv_append_varlen_paged", k_new, k_pool, v_pool, block_table, seq_lens, cu_seqlens_q)
    _require_gpu(k_new, v_new)
    T, Hkv, D = k_new.shape
    if tuple(v_new.shape) != tuple(k_new.shape) or k_pool.shape[2] != Hkv or (v_new.numel() and v_new.stride(-1) != 1):
        raise PliError(f"kv_append_varlen_paged shape mismatch new{tuple(k_new.shape)} v{tuple(v_new.shape)} "
                       f"pool{tuple(k_pool.shape)}")
    num_blocks, bs = k_pool.shape[0], k_pool.shape[1]
    st = (_c_i64 * 10)(*(int(x) for x in (k_new.stride(0), k_new.stride(1),
                                          k_pool.stride(0), k_pool.stride(1), k_pool.stride(2),
                                          v_pool.stride(0), v_pool.stride(1), v_pool.stride(2),
                                          v_new.stride(0), v_new.stride(1))))
    with _on_device(dev):
        rc = lib().pli_kv_append_varlen_paged(_ptr(k_new), _ptr(v_new), _ptr(k_pool), _ptr(v_pool),
                                              _ptr(cu_seqlens_q), _ptr(block_table), _ptr(seq_lens),
                                              block_table.shape[0], T, Hkv, D, bs, num_blocks, block_table.shape[1],
                                              st, _dtype_code(k_new), _stream(dev))
    _check(rc, "pli_kv_append_varlen_paged")


# ------------------------------------------- 1-byte (fp8 e4m3) paged KV cache
FP8_POOL_DTYPES = (torch.float8_e4m3fn, torch.uint8)


def _check_fp8(what: str, x: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_scale, v_scale,
               ints: dict):
    """shared checks of the fp8 calls: x (q or k_new) fp32 / fp16 / bf16 with D last, the pools
    [num_blocks, block_size, Hkv, D] views of torch.float8_e4m3fn or torch.uint8 (any page stride), the scales
    fp32 [Hkv] on the device or None (all ones), the named int32 tensors contiguous; returns the device"""
    dev = _require_gpu(x)
    _dtype_code(x)
    for name, t in (("k_pool", k_pool), ("v_pool", v_pool)):
        if not t.is_cuda or t.device != dev or t.dtype not in FP8_POOL_DTYPES or t.dtype != k_pool.dtype:
            raise PliError(f"{what}: {name} must be a torch.float8_e4m3fn or torch.uint8 tensor on {dev}, "
                           f"got {t.dtype} on {t.device}")
    for name, t in ints.items():
        if not t.is_cuda or t.device != dev or t.dtype != torch.int32 or not t.is_contiguous():
            raise PliError(f"{what}: {name} must be a contiguous int32 tensor on {dev}")
    if k_pool.dim() != 4 or tuple(v_pool.shape) != tuple(k_pool.shape) or k_pool.shape[3] != x.shape[-1]:
        raise PliError(f"{what} expects [num_blocks, block_size, Hkv, D] pools with the tokens' D, got "
                       f"{tuple(x.shape)} k{tuple(k_pool.shape)} v{tuple(v_pool.shape)}")
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if t is not None and (not t.is_cuda or t.device != dev or t.dtype != torch.float32 or
                              tuple(t.shape) != (k_pool.shape[2],) or not t.is_contiguous()):
            raise PliError(f"{what}: {name} must be None or a contiguous fp32 [{k_pool.shape[2]}] tensor on {dev}")
    if any(t.stride(-1) != 1 for t in (x, k_pool, v_pool) if t.numel()):
        raise PliError(f"{what}: a unit head_dim stride is required (the pools are used in place)")
    return dev


def attn_decode_paged_fp8(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                          block_table: torch.Tensor, seq_lens: torch.Tensor, k_scale: torch.Tensor | None = None,
                          v_scale: torch.Tensor | None = None, *, scale: float | None = None,
                          causal: bool = True, n_kv_add: int = 0, max_kv: int | None = None,
                          out: torch.Tensor | None = None, workspace: torch.Tensor | None = None
                          ) -> torch.Tensor:
    """attn_decode_paged over 1-byte pools of fp8 e4m3fn codes (torch.float8_e4m3fn or torch.uint8 views), an
    element's value being code * scale[kv head]: k_scale / v_scale fp32 [Hkv] device tensors read on the device
    (graph-replayable), None for all ones.  q and the output are bf16 / fp16 (MFMA kernel) or fp32."""
    dev = _check_fp8("attn_decode_paged_fp8", q, k_pool, v_pool, k_scale, v_scale,
                     {"block_table": block_table, "seq_lens": seq_lens})
    if q.dim() != 4 or block_table.dim() != 2 or block_table.shape[0] != q.shape[0] or \
            tuple(seq_lens.shape) != (q.shape[0],):
        raise PliError(f"attn_decode_paged_fp8: shape mismatch q{tuple(q.shape)} table{tuple(block_table.shape)} "
                       f"seq_lens{tuple(seq_lens.shape)}")
    B, Sq, H, D = q.shape
    num_blocks, bs, Hkv, _ = k_pool.shape
    max_blocks = block_table.shape[1]
    if Hkv == 0 or H % Hkv != 0:
        raise PliError(f"heads {H} not a multiple of kv heads {Hkv}")
    cap = max_blocks * bs
    max_kv = cap if max_kv is None else int(max_kv)
    if not 0 <= max_kv <= cap:
        raise PliError(f"max_kv {max_kv} outside the table row [0, {cap}]")
    if out is None:
        out = torch.empty((B, Sq, H, D), device=q.device, dtype=q.dtype)
    _require_gpu(q, out)
    if tuple(out.shape) != (B, Sq, H, D) or (out.numel() and out.stride(-1) != 1):
        raise PliError("bad output tensor")
    if scale is None:
        scale = D ** -0.5
    st = (_c_i64 * 12)(*(int(x) for x in (q.stride(0), q.stride(2), q.stride(1),
                                          k_pool.stride(0), k_pool.stride(1), k_pool.stride(2),
                                          v_pool.stride(0), v_pool.stride(1), v_pool.stride(2),
                                          out.stride(0), out.stride(2), out.stride(1))))
    ws_bytes = int(lib().pli_attn_decode_paged_workspace_size(B, H, Hkv, Sq, max_kv, D))
    if workspace is None or workspace.numel() * workspace.element_size() < ws_bytes:
        workspace = torch.empty(max(ws_bytes // 4, 1), device=q.device, dtype=torch.float32)
    with _on_device(dev):
        rc = lib().pli_attn_decode_paged_fp8(_ptr(q), _ptr(k_pool), _ptr(v_pool), _ptr(out), _ptr(block_table),
                                             _ptr(seq_lens), _ptr(k_scale), _ptr(v_scale), B, H, Hkv, Sq, D, bs,
                                             num_blocks, max_blocks, max_kv, st, float(scale), int(bool(causal)),
                                             int(n_kv_add), _ptr(workspace), ws_bytes, _dtype_code(q), _stream(dev))
    _check(rc, "pli_attn_decode_paged_fp8")
    return out


def kv_append_paged_fp8(k_new: torch.Tensor, v_new: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                        block_table: torch.Tensor, seq_lens: torch.Tensor, k_scale: torch.Tensor | None = None,
                        v_scale: torch.Tensor | None = None) -> None:
    """kv_append_paged into 1-byte pools: k_new / v_new [B, T, Hkv, D] (fp32 / fp16 / bf16) are stored as
    e4m3fn(clamp(x / scale[kv head], -448, 448)), round to nearest even, NaN kept."""
    dev = _check_fp8("kv_append_paged_fp8", k_new, k_pool, v_pool, k_scale, v_scale,
                     {"block_table": block_table, "seq_lens": seq_lens})
    _require_gpu(k_new, v_new)
    if k_new.dim() != 4 or tuple(v_new.shape) != tuple(k_new.shape) or k_pool.shape[2] != k_new.shape[2] or \
            (v_new.numel() and v_new.stride(-1) != 1) or block_table.dim() != 2 or \
            block_table.shape[0] != k_new.shape[0] or tuple(seq_lens.shape) != (k_new.shape[0],):
        raise PliError(f"kv_append_paged_fp8 shape mismatch new{tuple(k_new.shape)} v{tuple(v_new.shape)} "
                       f"pool{tuple(k_pool.shape)} table{tuple(block_table.shape)} seq_lens{tuple(seq_lens.shape)}")
    B, T, Hkv, D = k_new.shape
    num_blocks, bs = k_pool.shape[0], k_pool.shape[1]
    st = (_c_i64 * 12)(*(int(x) for x in (k_new.stride(0), k_new.stride(2), k_new.stride(1),
                                          k_pool.stride(0), k_pool.stride(1), k_pool.stride(2),
                                          v_pool.stride(0), v_pool.stride(1), v_pool.stride(2),
                                          v_new.stride(0), v_new.stride(2), v_new.stride(1))))
    with _on_device(dev):
        rc = lib().pli_kv_append_paged_fp8(_ptr(k_new), _ptr(v_new), _ptr(k_pool), _ptr(v_pool), _ptr(block_table),
                                           _ptr(seq_lens), _ptr(k_scale), _ptr(v_scale), B, T, Hkv, D, bs,
                                           num_blocks, block_table.shape[1], st, _dtype_code(k_new), _stream(dev))
    _check(rc, "pli_kv_append_paged_fp8")


def _check_varlen_fp8(what: str, x: torch.Tensor, k_pool, v_pool, k_scale, v_scale, block_table, seq_lens,
                      cu_seqlens_q):
    dev = _check_fp8(what, x, k_pool, v_pool, k_scale, v_scale,
                     {"block_table": block_table, "seq_lens": seq_lens, "cu_seqlens_q": cu_seqlens_q})
    B = seq_lens.shape[0] if seq_lens.dim() == 1 else -1
    if x.dim() != 3 or block_table.dim() != 2 or block_table.shape[0] != B or tuple(cu_seqlens_q.shape) != (B + 1,):
        raise PliError(f"{what}: shape mismatch tokens{tuple(x.shape)} table{tuple(block_table.shape)} "
                       f"seq_lens{tuple(seq_lens.shape)} cu_seqlens_q{tuple(cu_seqlens_q.shape)}")
    return dev


def attn_varlen_paged_fp8(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor,
                          seq_lens: torch.Tensor, cu_seqlens_q: torch.Tensor, k_scale: torch.Tensor | None = None,
                          v_scale: torch.Tensor | None = None, max_kv: int | None = None,
                          scale: float | None = None, causal: bool = True,
                          out: torch.Tensor | None = None, workspace: torch.Tensor | None = None,
                          split_keys: int = 0) -> torch.Tensor:
    """attn_varlen_paged over 1-byte pools of fp8 e4m3fn codes; pools and scales as for attn_decode_paged_fp8;
    workspace / split_keys as for attn_varlen_paged (pli_attn_varlen_paged_fp8_ws)."""
    if workspace is not None:
        _varlen_workspace("attn_varlen_paged_fp8", workspace, split_keys, q, k_pool, block_table, max_kv)
    dev = _check_varlen_fp8("attn_varlen_paged_fp8", q, k_pool, v_pool, k_scale, v_scale, block_table, seq_lens,
                            cu_seqlens_q)
    T, H, D = q.shape
    num_blocks, bs, Hkv, _ = k_pool.shape
    B, max_blocks = block_table.shape
    if Hkv == 0 or H % Hkv != 0:
        raise PliError(f"heads {H} not a multiple of kv heads {Hkv}")
    cap = max_blocks * bs
    max_kv = cap if max_kv is None else int(max_kv)
    if not 0 <= max_kv <= cap:
        raise PliError(f"max_kv {max_kv} outside the table row [0, {cap}]")
    if out is None:
        out = torch.empty((T, H, D), device=q.device, dtype=q.dtype)
    _require_gpu(q, out)
    if tuple(out.shape) != (T, H, D) or (out.numel() and out.stride(-1) != 1):
        raise PliError("bad output tensor")
    if scale is None:
        scale = D ** -0.5
    st = (_c_i64 * 10)(*(int(x) for x in (q.stride(0), q.stride(1),
                                          k_pool.stride(0), k_pool.stride(1), k_pool.stride(2),
                                          v_pool.stride(0), v_pool.stride(1), v_pool.stride(2),
                                          out.stride(0), out.stride(1))))
    with _on_device(dev):
        if workspace is not None:
            rc = lib().pli_attn_varlen_paged_fp8_ws(_ptr(q), _ptr(k_pool), _ptr(v_pool), _ptr(out),
                                                    _ptr(cu_seqlens_q), _ptr(block_table), _ptr(seq_lens),
                                                    _ptr(k_scale), _ptr(v_scale), B, T, H, Hkv, D, bs, num_blocks,
                                                    max_blocks, max_kv, st, float(scale), int(bool(causal)),
                                                    _dtype_code(q), int(split_keys), _ptr(workspace),
                                                    workspace.numel() * workspace.element_size(), _stream(dev))
            _check(rc, "pli_attn_varlen_paged_fp8_ws")
            return out
        rc = lib().pli_attn_varlen_paged_fp8(_ptr(q), _ptr(k_pool), _ptr(v_pool), _ptr(out), _ptr(cu_seqlens_q),
                                             _ptr(block_table), _ptr(seq_lens), _ptr(k_scale), _ptr(v_scale), B, T,
                                             H, Hkv, D, bs, num_blocks, max_blocks, max_kv, st, float(scale),
                                             int(bool(causal)), _dtype_code(q), _stream(dev))
    _check(rc, "pli_attn_varlen_paged_fp8")
    return out


def kv_append_varlen_paged_fp8(k_new: torch.Tensor, v_new: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                               block_table: torch.Tensor, seq_lens: torch.Tensor, cu_seqlens_q: torch.Tensor,
                               k_scale: torch.Tensor | None = None, v_scale: torch.Tensor | None = None) -> None:
    """kv_append_varlen_paged into 1-byte pools; quantisation as for kv_append_paged_fp8."""
    dev = _check_varlen_fp8("kv_append_varlen_paged_fp8", k_new, k_pool, v_pool, k_scale, v_scale, block_table,
                            seq_lens, cu_seqlens_q)
    _require_gpu(k_new, v_new)
    T, Hkv, D = k_new.shape
    if tuple(v_new.shape) != tuple(k_new.shape) or k_pool.shape[2] != Hkv or (v_new.numel() and v_new.stride(-1) != 1):
        raise PliError(f"kv_append_varlen_paged_fp8 shape mismatch new{tuple(k_new.shape)} v{tuple(v_new.shape)} "
                       f"pool{tuple(k_pool.shape)}")
    num_blocks, bs = k_pool.shape[0], k_pool.shape[1]
    st = (_c_i64 * 10)(*(int(x) for x in (k_new.stride(0), k_new.stride(1),
                                          k_pool.stride(0), k_pool.stride(1), k_pool.stride(2),
                                          v_pool.stride(0), v_pool.stride(1), v_pool.stride(2),
                                          v_new.stride(0), v_new.stride(1))))
    with _on_device(dev):
        rc = lib().pli_kv_append_varlen_paged_fp8(_ptr(k_new), _ptr(v_new), _ptr(k_pool), _ptr(v_pool),
                                                  _ptr(cu_seqlens_q), _ptr(block_table), _ptr(seq_lens),
                                                  _ptr(k_scale), _ptr(v_scale), block_table.shape[0], T, Hkv, D, bs,
                                                  num_blocks, block_table.shape[1], st, _dtype_code(k_new),
                                                  _stream(dev))
    _check(rc, "pli_kv_append_varlen_paged_fp8")


# ---------------------------------------------------------------------- MoE
def moe_route(logits: torch.Tensor, top_k: int, normalize: bool = True):
    """Router tail of ch09/moe_layer.py:24-33 on the device: returns
    (weights [T, k] fp32, expert_idx [T, k] int32, pos [T, k] int32,
    gather [T*k] int32, offsets [E+1] int32)."""
    dev = _require_gpu(logits)
    T, E = logits.shape
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    i32 = dict(device=logits.device, dtype=torch.int32)
    weights = torch.empty(T, top_k, device=logits.device, dtype=torch.float32)
    idx = torch.empty(T, top_k, **i32)
    pos = torch.empty(T, top_k, **i32)
    gather = torch.empty(max(T * top_k, 1), **i32)
    offsets = torch.empty(E + 1, **i32)
    ws = torch.empty(E + T * top_k, **i32)
    with _on_device(dev):
        rc = lib().pli_moe_route(_ptr(logits), logits.stride(0), T, E, int(top_k), int(bool(normalize)),
                                 _dtype_code(logits), _ptr(weights), _ptr(idx), _ptr(pos),
                                 _ptr(gather), _ptr(offsets), _ptr(ws), _stream(dev))
    _check(rc, "pli_moe_route")
    return weights, idx, pos, gather, offsets


def weight_table(weights: list[torch.Tensor]) -> torch.Tensor:
    """Device int64 array of the weights' data pointers (for pli_gemm_grouped)."""
    return torch.tensor([w.data_ptr() for w in weights], dtype=torch.int64,
                        device=weights[0].device)


def gemm_grouped(x: torch.Tensor, gather: torch.Tensor | None, w_table: torch.Tensor,
                 offsets: torch.Tensor, rows: int, n: int, k: int, ldw: int,
                 wu_table: torch.Tensor | None = None, out: torch.Tensor | None = None,
                 variant: int | None = None) -> torch.Tensor:
    """Per-expert NT GEMM over expert-sorted rows (see include/pli.h).
    `rows` is the host bound rows_bound >= offsets[experts], the number of sorted rows
    (tokens * top_k after moe_route); `out`, if given, holds that many rows."""
    dev = _require_gpu(x)
    E = offsets.numel() - 1
    if out is None:
        out = torch.empty(max(rows, 1), n, device=x.device, dtype=x.dtype)
    args = (_ptr(x), _ptr(gather), _ptr(w_table), _ptr(wu_table), _ptr(out), _ptr(offsets), E,
            int(rows), int(n), int(k), x.stride(0), int(ldw), out.stride(0), _dtype_code(x), _stream(dev))
    with _on_device(dev):
        if variant is None:
            rc = lib().pli_gemm_grouped(*args)
        else:
            rc = lib().pli_gemm_grouped_variant(*args, int(variant))
    _check(rc, "pli_gemm_grouped")
    return out


def moe_combine(y: torch.Tensor, pos: torch.Tensor, weights: torch.Tensor, tokens: int,
                out: torch.Tensor | None = None) -> torch.Tensor:
    dev = _require_gpu(y)
    H = y.shape[1]
    k = pos.shape[1]
    if out is None:
        out = torch.empty(tokens, H, device=y.device, dtype=y.dtype)
    with _on_device(dev):
        rc = lib().pli_moe_combine(_ptr(y), y.stride(0), _ptr(pos), _ptr(weights), _ptr(out),
                                   out.stride(0), tokens, k, H, _dtype_code(y), _stream(dev))
    _check(rc, "pli_moe_combine")
    return out


# ----------------------------------------------------------------- sampling
def sample(logits: torch.Tensor, temperature: float = 1.0, top_k: int | None = None, top_p: float = 1.0, *,
           uniforms: torch.Tensor | None = None, seed: int = 0, offset=0,
           out: torch.Tensor | None = None) -> torch.Tensor:
    """Next token of every row of ``logits`` [..., vocab] (pli_sample, include/pli.h: temperature, top-k, top-p and
    the draw in one launch): int64 of shape ``logits.shape[:-1]``, -1 for a row with no logit above -inf.
    ``temperature`` 0 is greedy; ``top_k`` None / <= 0 / >= vocab keeps every token; ``top_p`` >= 1 keeps all of
    top-k's.  The uniform of row r is ``uniforms[r]`` (device fp32, in [0, 1)) when given, else Philox4x32-10 of
    (``seed``, offset, r); ``offset`` is an int, an int32 device tensor the KERNEL reads (so a captured call
    replays while it changes), or a ``(tensor, add)`` pair.  ``out`` may be a strided view (e.g. a column of an
    id buffer).  A non-unit inner stride of ``logits`` is copied first, as moe_route does."""
    dev = _require_gpu(logits)
    if logits.dim() < 1 or logits.shape[-1] < 1:
        raise PliError(f"sample: logits need a last dimension of at least 1, got shape {tuple(logits.shape)}")
    lead, V = tuple(logits.shape[:-1]), logits.shape[-1]
    x = logits.reshape(-1, V)
    rows = x.shape[0]
    if x.stride(1) != 1 or (rows > 1 and x.stride(0) < V):
        x = x.contiguous()
    if out is None:
        out = torch.empty(lead, device=logits.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or out.device != logits.device or tuple(out.shape) != lead:
        raise PliError(f"sample: out must be int64 {lead} on {logits.device}, got {out.dtype} {tuple(out.shape)} "
                       f"on {out.device}")
    try:
        flat = out if out.dim() == 1 else out.view(-1)
    except RuntimeError:
        raise PliError(f"sample: out (strides {out.stride()}) does not flatten to one row stride") from None
    ld_tokens = flat.stride(0) if rows > 1 else 1
    off_dev, off_add = (None, offset) if isinstance(offset, int) else offset if isinstance(offset, tuple) else (offset, 0)
    if off_dev is not None and (off_dev.dtype != torch.int32 or off_dev.device != logits.device or off_dev.numel() < 1):
        raise PliError("sample: the offset tensor must be int32 on the logits' device")
    if uniforms is not None:
        if uniforms.dtype != torch.float32 or uniforms.device != logits.device or uniforms.numel() != rows:
            raise PliError(f"sample: uniforms must be float32 [{rows}] on the logits' device")
        uniforms = uniforms.contiguous()
    with _on_device(dev):
        rc = lib().pli_sample(_ptr(x), x.stride(0) if rows > 1 else V, rows, V, _dtype_code(x), float(temperature),
                              int(top_k or 0), float(top_p), _ptr(uniforms), int(seed) & (2 ** 64 - 1),
                              _ptr(off_dev), int(off_add), _ptr(flat), ld_tokens, None, 0, _stream(dev))
    _check(rc, "pli_sample")
    return out


# ------------------------------------------------------------------ RMSNorm
def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6,
            residual: torch.Tensor | None = None, out: torch.Tensor | None = None):
    """y = h / sqrt(mean(h^2) + eps) * weight over the last dim, h = x (+ residual).
    Returns y, or (h, y) when a residual is given (h = x + residual in x.dtype)."""
    dev = _require_gpu(x, weight)
    n = x.shape[-1]
    if weight.shape != (n,):
        raise PliError(f"weight {tuple(weight.shape)} for rows of {n}")
    x2 = x.reshape(-1, n)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    r2 = None
    if residual is not None:
        _require_gpu(x, residual)
        if residual.shape != x.shape:
            raise PliError("residual shape mismatch")
        r2 = residual.reshape(-1, n)
        if r2.stride(-1) != 1:
            r2 = r2.contiguous()
    weight = weight.contiguous()
    if out is not None:
        _check_out(out, x, tuple(x.shape), "rmsnorm")
        if not out.is_contiguous():
            raise PliError("rmsnorm: out must be contiguous")
    y = torch.empty_like(x2) if out is None else out.view(-1, n)
    h = torch.empty_like(x2) if residual is not None else None
    rows = x2.shape[0]
    with _on_device(dev):
        rc = lib().pli_rmsnorm(_ptr(x2), _ptr(r2), _ptr(weight), _ptr(y), _ptr(h), rows, n,
                               x2.stride(0), r2.stride(0) if r2 is not None else n, y.stride(0),
                               h.stride(0) if h is not None else n, float(eps), _dtype_code(x),
                               _stream(dev))
    _check(rc, "pli_rmsnorm")
    y = y.view(x.shape)
    return y if residual is None else (h.view(x.shape), y)


def qkv_into_cache(x: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor,
                   q_out: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                   pos: torch.Tensor) -> torch.Tensor:
    """Decode-step projections in one launch (pli_gemm_multi_nt): x [B, S, hidden]
    (B*S <= 128; above 16 rows hidden % 128 == 0) -> q_out [B, S, Hq*D]; k / v
    rows written into [B, S_max, Hkv, D] caches at rows pos[0] + s.  Returns
    q_out."""
    dev = _require_gpu(x, wq, wk, wv, q_out, k_cache, v_cache)
    B, S, hidden = x.shape
    x2 = x.reshape(B * S, hidden)
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    S_max, Hkv, D = k_cache.shape[1:]
    if pos.dtype != torch.int32 or not pos.is_cuda:
        raise PliError("pos must be an int32 device tensor")
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.shape[0] != B or t.stride(3) != 1 or t.stride(2) != D:
            raise PliError(f"{name} must be [B, S_max, Hkv, D] with contiguous (Hkv, D) rows")
    if tuple(v_cache.shape) != tuple(k_cache.shape):
        raise PliError("k_cache / v_cache shape mismatch")
    if wk.shape[0] != Hkv * D or wv.shape[0] != Hkv * D or q_out.shape[-1] != wq.shape[0]:
        raise PliError("projection widths do not match the cache / output")
    if q_out.dim() != 3 or tuple(q_out.shape[:2]) != (B, S) or q_out.stride(2) != 1:
        raise PliError("q_out must be [B, S, Hq*D] with unit inner stride")
    if any(w.stride(1) != 1 or w.shape[1] != hidden for w in (wq, wk, wv)):
        raise PliError("weights must be [n, hidden] with unit inner stride")
    P = ctypes.c_void_p
    w = (P * 3)(*(t.data_ptr() for t in (wq, wk, wv)))
    c = (P * 3)(q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr())
    n = (_c_int * 3)(wq.shape[0], wk.shape[0], wv.shape[0])
    ldw = (_c_i64 * 3)(wq.stride(0), wk.stride(0), wv.stride(0))
    sb = (_c_i64 * 3)(q_out.stride(0), k_cache.stride(0), v_cache.stride(0))
    stok = (_c_i64 * 3)(q_out.stride(1), k_cache.stride(1), v_cache.stride(1))
    ro = (P * 3)(None, pos.data_ptr(), pos.data_ptr())
    cap = (_c_int * 3)(S, S_max, S_max)
    with _on_device(dev):
        rc = lib().pli_gemm_multi_nt(_ptr(x2), x2.stride(0), B * S, hidden, S, w, c, n, ldw, sb, stok,
                                     ro, cap, 3, _dtype_code(x), _stream(dev))
    _check(rc, "pli_gemm_multi_nt")
    return q_out


def _rows(t: torch.Tensor) -> torch.Tensor:
    t2 = t.reshape(-1, t.shape[-1])
    return t2 if t2.stride(1) == 1 and t2.stride(0) % 8 == 0 else t2.contiguous()


def _rms_gemm(a: torch.Tensor, norm_weight: torch.Tensor, eps: float, groups: list,
              residual: torch.Tensor | None, h_out: torch.Tensor | None, tokens_per_batch: int,
              swiglu: bool) -> None:
    """pli_rms_gemm_nt.  groups: (w, w_up | None, c, n, stride_batch, stride_token,
    pos | None, capacity) with c the output base tensor."""
    dev = _require_gpu(a, norm_weight, *(g[0] for g in groups))
    a2 = _rows(a)
    r2 = _rows(residual) if residual is not None else None
    if h_out is not None and (h_out.stride(-1) != 1 or tuple(h_out.shape[-1:]) != (a2.shape[1],)):
        raise PliError("h_out must have unit inner stride and the hidden width")
    h2 = h_out.view(-1, h_out.shape[-1]) if h_out is not None else None
    m, k = a2.shape
    ng = len(groups)
    P = ctypes.c_void_p
    w = (P * ng)(*(g[0].data_ptr() for g in groups))
    wu = (P * ng)(*(g[1].data_ptr() for g in groups)) if swiglu else None
    c = (P * ng)(*(g[2].data_ptr() for g in groups))
    n = (_c_int * ng)(*(int(g[3]) for g in groups))
    ldw = (_c_i64 * ng)(*(g[0].stride(0) for g in groups))
    sb = (_c_i64 * ng)(*(int(g[4]) for g in groups))
    stok = (_c_i64 * ng)(*(int(g[5]) for g in groups))
    ro = (P * ng)(*((g[6].data_ptr() if g[6] is not None else None) for g in groups))
    cap = (_c_int * ng)(*(int(g[7]) for g in groups))
    for g in groups:
        if g[0].stride(1) != 1 or (g[1] is not None and (g[1].stride(1) != 1 or g[1].stride(0) != g[0].stride(0))):
            raise PliError("weights must be [n, k] with unit inner stride (up weight: same ldw)")
    with _on_device(dev):
        rc = lib().pli_rms_gemm_nt(_ptr(a2), a2.stride(0), _ptr(r2), r2.stride(0) if r2 is not None else 0,
                                   _ptr(norm_weight), float(eps), _ptr(h2),
                                   h2.stride(0) if h2 is not None else 0, m, k, int(tokens_per_batch),
                                   w, wu, c, n, ldw, sb, stok, ro, cap, ng, _dtype_code(a), _stream(dev))
    _check(rc, "pli_rms_gemm_nt")


def rms_linear(a: torch.Tensor, norm_weight: torch.Tensor, eps: float, w: torch.Tensor,
               residual: torch.Tensor | None = None, h_out: torch.Tensor | None = None,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """rmsnorm(a (+ residual)) @ w^T in one launch (decode: <= 4 rows)."""
    a2 = a.reshape(-1, a.shape[-1])
    if out is None:
        out = torch.empty(a2.shape[0], w.shape[0], device=a.device, dtype=a.dtype)
    # one token per "batch": row bb lands at out + bb * stride(0)
    _rms_gemm(a, norm_weight, eps, [(w, None, out, w.shape[0], out.stride(0), 0, None, 1 << 30)],
              residual, h_out, 1, False)
    return out.view(*a.shape[:-1], w.shape[0])


def rms_swiglu(a: torch.Tensor, norm_weight: torch.Tensor, eps: float, wg: torch.Tensor,
               wu: torch.Tensor, residual: torch.Tensor | None = None,
               h_out: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """silu(y wg^T) * (y wu^T) with y = rmsnorm(a (+ residual)), one launch."""
    a2 = a.reshape(-1, a.shape[-1])
    if out is None:
        out = torch.empty(a2.shape[0], wg.shape[0], device=a.device, dtype=a.dtype)
    _rms_gemm(a, norm_weight, eps, [(wg, wu, out, wg.shape[0], out.stride(0), 0, None, 1 << 30)],
              residual, h_out, 1, True)
    return out.view(*a.shape[:-1], wg.shape[0])


def rms_qkv_into_cache(a: torch.Tensor, norm_weight: torch.Tensor, eps: float,
                       wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor, q_out: torch.Tensor,
                       k_cache: torch.Tensor, v_cache: torch.Tensor, pos: torch.Tensor,
                       residual: torch.Tensor | None = None,
                       h_out: torch.Tensor | None = None) -> torch.Tensor:
    """qkv_into_cache on rmsnorm(a (+ residual)), one launch; a [B, S, hidden]."""
    B, S, _ = a.shape
    S_max, Hkv, D = k_cache.shape[1:]
    if pos.dtype != torch.int32 or not pos.is_cuda:
        raise PliError("pos must be an int32 device tensor")
    for t in (k_cache, v_cache):
        if t.shape[0] != B or t.stride(3) != 1 or t.stride(2) != D:
            raise PliError("caches must be [B, S_max, Hkv, D] with contiguous (Hkv, D) rows")
    if q_out.dim() != 3 or tuple(q_out.shape[:2]) != (B, S) or q_out.stride(2) != 1:
        raise PliError("q_out must be [B, S, Hq*D] with unit inner stride")
    groups = [(wq, None, q_out, wq.shape[0], q_out.stride(0), q_out.stride(1), None, S),
              (wk, None, k_cache, wk.shape[0], k_cache.stride(0), k_cache.stride(1), pos, S_max),
              (wv, None, v_cache, wv.shape[0], v_cache.stride(0), v_cache.stride(1), pos, S_max)]
    _rms_gemm(a, norm_weight, eps, groups, residual, h_out, S, False)
    return q_out


# ------------------------------------------------------------ fused SwiGLU
def gemm_swiglu(x: torch.Tensor, w_gate: torch.Tensor, w_up: torch.Tensor,
                out: torch.Tensor | None = None, split_k: bool = True,
                variant: int | None = None) -> torch.Tensor:
    """h = silu(x W_gate^T) * (x W_up^T) in one launch; x [m, k], W_* [n, k]
    (unit column stride; any row stride, e.g. the two halves of a fused
    gate_up weight)."""
    dev = _require_gpu(x, w_gate, w_up)
    if x.dim() != 2 or w_gate.dim() != 2 or tuple(w_up.shape) != tuple(w_gate.shape) \
            or w_gate.shape[1] != x.shape[1]:
        raise PliError(f"gemm_swiglu shape mismatch x{tuple(x.shape)} wg{tuple(w_gate.shape)} "
                       f"wu{tuple(w_up.shape)}")
    x, w_gate, w_up = (t if t.stride(1) == 1 else t.contiguous() for t in (x, w_gate, w_up))
    m, k = x.shape
    n = w_gate.shape[0]
    if out is None:
        out = torch.empty(m, n, device=x.device, dtype=x.dtype)
    _require_gpu(x, out)
    if tuple(out.shape) != (m, n) or out.stride(1) != 1:
        raise PliError("bad output tensor")
    head = (_ptr(x), _ptr(w_gate), _ptr(w_up), _ptr(out), m, n, k, x.stride(0), w_gate.stride(0),
            w_up.stride(0), out.stride(0), _dtype_code(x))
    with _on_device(dev):
        wsb = lib().pli_gemm_swiglu_workspace_size(m, n, k, _dtype_code(x)) if split_k else 0
        if variant is not None:  # an explicit route (A/B, tests); no workspace when none is needed
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
            rc = lib().pli_gemm_swiglu_ws_variant(*head, _ptr(ws), wsb, _stream(dev), int(variant))
        elif wsb:
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            rc = lib().pli_gemm_swiglu_ws(*head, _ptr(ws), wsb, _stream(dev))
        else:
            rc = lib().pli_gemm_swiglu(*head, _stream(dev))
    _check(rc, "pli_gemm_swiglu")
    return out


# ------------------------------------------- weight-only fp8 linear (W8A16)
FP8_E4M3_MAX = 448.0


def quantize_weight_fp8(w: torch.Tensor, scale: torch.Tensor | None = None):
    """Per-output-row e4m3fn quantisation of a weight [n, k] (torch ops only; CPU or GPU):
    ``(codes, scale)`` with codes ``torch.float8_e4m3fn`` [n, k] and scale fp32 [n], value = code * scale[row].
    scale[j] = absmax(row j) / 448 in fp32 (1.0 for an all-zero row), or the given ``scale``;
    codes = (w.float() * (1.0f / scale)).clamp(-448, 448) cast to e4m3fn (round to nearest even): the rule of the
    quantising KV appends.  Non-finite weights raise ``ValueError``."""
    if w.dim() != 2:
        raise ValueError(f"quantize_weight_fp8 expects a [n, k] weight, got {tuple(w.shape)}")
    wf = w.detach().float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_weight_fp8: non-finite weight")
    n = wf.shape[0]
    if scale is None:
        amax = wf.abs().amax(dim=1) if wf.shape[1] else torch.zeros(n, dtype=torch.float32, device=wf.device)
        scale = torch.where(amax > 0, amax / FP8_E4M3_MAX, torch.ones_like(amax))
    else:
        scale = scale.detach().to(device=wf.device, dtype=torch.float32)
        if tuple(scale.shape) != (n,) or not bool((torch.isfinite(scale) & (scale > 0)).all()):
            raise ValueError(f"quantize_weight_fp8: scale must be {n} finite positive values")
    scale = scale.contiguous()
    inv = 1.0 / scale
    codes = (wf * inv[:, None]).clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX).to(torch.float8_e4m3fn)
    return codes, scale


def _check_fp8w(what: str, x: torch.Tensor, weights) -> torch.device:
    """x [m, k] fp16 / bf16 on a device; each (codes, scale): codes [n, k] float8_e4m3fn / uint8 with a unit column
    stride, scale None or contiguous fp32 [n], all on x's device"""
    dev = _require_gpu(x)
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise PliError(f"{what}: activations must be fp16 or bf16, got {x.dtype}")
    n = weights[0][0].shape[0] if weights[0][0].dim() == 2 else -1
    for codes, scale in weights:
        if not codes.is_cuda:
            raise PliError("HIP path called with a CPU tensor")
        if codes.device != dev or codes.dtype not in FP8_POOL_DTYPES:
            raise PliError(f"{what}: codes must be a torch.float8_e4m3fn or torch.uint8 tensor on {dev}, "
                           f"got {codes.dtype} on {codes.device}")
        if codes.dim() != 2 or codes.shape[0] != n or codes.shape[1] != x.shape[-1]:
            raise PliError(f"{what} shape mismatch: x{tuple(x.shape)} codes{tuple(codes.shape)}")
        if codes.numel() and codes.stride(1) != 1:
            raise PliError(f"{what}: codes need a unit column stride (they are used in place)")
        if scale is not None and (not scale.is_cuda or scale.device != dev or scale.dtype != torch.float32 or
                                  tuple(scale.shape) != (n,) or not scale.is_contiguous()):
            raise PliError(f"{what}: scale must be None or a contiguous fp32 [{n}] tensor on {dev}")
    return dev


def _fp8w_workspace(what: str, workspace, dev):
    if workspace is None:
        return None, 0
    if not workspace.is_cuda or workspace.device != dev or not workspace.is_contiguous():
        raise PliError(f"{what}: workspace must be a contiguous tensor on {dev}")
    return workspace.data_ptr(), workspace.numel() * workspace.element_size()


def _ldw(codes: torch.Tensor) -> int:
    return max(codes.stride(0), codes.shape[1]) if codes.shape[0] > 1 else codes.shape[1]


def linear_fp8w_workspace_bytes(m: int, n: int, k: int, dtype: torch.dtype = torch.bfloat16,
                                swiglu: bool = False) -> int:
    """bytes of workspace linear_fp8w (linear_swiglu_fp8w with ``swiglu``) wants for [m, k] x [n, k]^T; 0: none"""
    fn = lib().pli_linear_swiglu_fp8w_workspace_size if swiglu else lib().pli_linear_fp8w_workspace_size
    return int(fn(int(m), int(n), int(k), DTYPE_CODE.get(dtype, -1)))


def linear_fp8w(x: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor | None, bias: torch.Tensor | None = None,
                out: torch.Tensor | None = None, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """C = x W^T (+ bias) over fp8 weights: x [m, k] fp16 / bf16, codes [n, k] e4m3fn (or uint8) used in place
    (any row stride), scale fp32 [n] or None (ones); W = decode(codes) * scale[:, None].  ``workspace`` (bytes from
    linear_fp8w_workspace_bytes) lets m > 16 shapes without a fast kernel run widen + the 16-bit GEMM."""
    if x.dim() != 2:
        raise PliError(f"linear_fp8w expects a 2-D x, got {tuple(x.shape)}")
    dev = _check_fp8w("linear_fp8w", x, [(codes, scale)])
    if x.stride(1) != 1:
        x = x.contiguous()
    m, k = x.shape
    n = codes.shape[0]
    if bias is not None:
        _require_gpu(x, bias)
        bias = bias.contiguous()
        if tuple(bias.shape) != (n,):
            raise PliError(f"bias must be [{n}]")
    if out is None:
        out = torch.empty((m, n), dtype=x.dtype, device=dev)
    else:
        _check_out(out, x, (m, n), "linear_fp8w")
    wsp, wsb = _fp8w_workspace("linear_fp8w", workspace, dev)
    with _on_device(dev):
        rc = lib().pli_linear_fp8w(_ptr(x), _ptr(codes), _ptr(scale), _ptr(bias), _ptr(out), m, n, k,
                                   max(x.stride(0), k) if m > 1 else k, _ldw(codes), max(out.stride(0), n),
                                   _dtype_code(x), wsp, wsb, _stream(dev))
    _check(rc, "pli_linear_fp8w")
    return out


def gemv_fp8w(codes: torch.Tensor, scale: torch.Tensor | None, x: torch.Tensor,
              out: torch.Tensor | None = None) -> torch.Tensor:
    """y = W x over fp8 weights (torch.mv semantics): codes [m, k], scale fp32 [m] or None, x [k] fp16 / bf16"""
    if x.dim() != 1:
        raise PliError(f"gemv_fp8w expects a 1-D x, got {tuple(x.shape)}")
    dev = _check_fp8w("gemv_fp8w", x, [(codes, scale)])
    x = x.contiguous()
    m, k = codes.shape
    if out is None:
        out = torch.empty(m, dtype=x.dtype, device=dev)
    else:
        _check_out(out, x, (m,), "gemv_fp8w")
    with _on_device(dev):
        rc = lib().pli_gemv_fp8w(_ptr(codes), _ptr(scale), _ptr(x), _ptr(out), m, k, _ldw(codes), _dtype_code(x),
                                 _stream(dev))
    _check(rc, "pli_gemv_fp8w")
    return out


def linear_swiglu_fp8w(x: torch.Tensor, g_codes: torch.Tensor, g_scale: torch.Tensor | None, u_codes: torch.Tensor,
                       u_scale: torch.Tensor | None, out: torch.Tensor | None = None,
                       workspace: torch.Tensor | None = None) -> torch.Tensor:
    """h = silu(x Wg^T) * (x Wu^T) over fp8 gate / up weights in one launch (neither gate nor up is written)"""
    if x.dim() != 2:
        raise PliError(f"linear_swiglu_fp8w expects a 2-D x, got {tuple(x.shape)}")
    dev = _check_fp8w("linear_swiglu_fp8w", x, [(g_codes, g_scale), (u_codes, u_scale)])
    if x.stride(1) != 1:
        x = x.contiguous()
    m, k = x.shape
    n = g_codes.shape[0]
    if out is None:
        out = torch.empty((m, n), dtype=x.dtype, device=dev)
    else:
        _check_out(out, x, (m, n), "linear_swiglu_fp8w")
    wsp, wsb = _fp8w_workspace("linear_swiglu_fp8w", workspace, dev)
    with _on_device(dev):
        rc = lib().pli_linear_swiglu_fp8w(_ptr(x), _ptr(g_codes), _ptr(g_scale), _ptr(u_codes), _ptr(u_scale),
                                          _ptr(out), m, n, k, max(x.stride(0), k) if m > 1 else k, _ldw(g_codes),
                                          _ldw(u_codes), max(out.stride(0), n), _dtype_code(x), wsp, wsb,
                                          _stream(dev))
    _check(rc, "pli_linear_swiglu_fp8w")
    return out


# ------------------------------------------------- fp8 activations (W8A8)
FP8A_MIN_ROWS = 17  # csrc/fp8a_plan.h kFp8aMinM: fewer rows stay on the W8A16 decode kernels


def _quantize_rows_fp8_torch(x: torch.Tensor):
    """the rule of pli_quantize_rows_fp8 in torch ops (any device): quantize_weight_fp8 per row, with the
    non-finite rule a device call needs (NaN -> 0x7F, +-inf -> +-448, neither enters the absmax)"""
    xf = x.detach().float()
    m = xf.shape[0]
    finite = torch.isfinite(xf)
    amax = (torch.where(finite, xf.abs(), torch.zeros_like(xf)).amax(dim=1) if xf.shape[1]
            else torch.zeros(m, dtype=torch.float32, device=xf.device))
    scale = torch.where(amax > 0, amax / FP8_E4M3_MAX, torch.ones_like(amax)).contiguous()
    inv = 1.0 / scale
    nan = torch.isnan(xf)
    y = torch.where(nan, torch.zeros_like(xf), xf) * inv[:, None]
    codes = y.clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX).to(torch.float8_e4m3fn)
    if bool(nan.any()):
        codes.view(torch.uint8)[nan] = 0x7F
    return codes, scale


def quantize_rows_fp8(x: torch.Tensor, out: tuple | None = None):
    """Per-row e4m3fn quantisation of activations x [m, k] fp16 / bf16: ``(codes, scale)`` with codes
    ``torch.float8_e4m3fn`` [m, k] and scale fp32 [m], value = code * scale[row].  The rule is quantize_weight_fp8's
    per row (bitwise for finite rows); a NaN element gets code 0x7F, +-inf the code of +-448, and neither enters the
    absmax.  On a device tensor this is the quant_rows_fp8 kernel, on a CPU tensor torch ops.  ``out``: a
    (codes, scale) pair to write into (device path; codes float8_e4m3fn / uint8 with a unit column stride)."""
    if x.dim() != 2:
        raise PliError(f"quantize_rows_fp8 expects a 2-D x, got {tuple(x.shape)}")
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise PliError(f"quantize_rows_fp8: activations must be fp16 or bf16, got {x.dtype}")
    if not x.is_cuda:
        if out is not None:
            raise PliError("quantize_rows_fp8: out is for the device path")
        return _quantize_rows_fp8_torch(x)
    dev = x.device
    if x.numel() and x.stride(1) != 1:
        x = x.contiguous()
    m, k = x.shape
    if out is None:
        codes = torch.empty((m, k), dtype=torch.float8_e4m3fn, device=dev)
        scale = torch.empty((m,), dtype=torch.float32, device=dev)
    else:
        codes, scale = out
        if (not codes.is_cuda or codes.device != dev or codes.dtype not in FP8_POOL_DTYPES or
                tuple(codes.shape) != (m, k) or (codes.numel() and codes.stride(1) != 1)):
            raise PliError(f"quantize_rows_fp8: out codes must be float8_e4m3fn / uint8 [{m}, {k}] on {dev} with a "
                           "unit column stride")
        if (not scale.is_cuda or scale.device != dev or scale.dtype != torch.float32 or tuple(scale.shape) != (m,) or
                not scale.is_contiguous()):
            raise PliError(f"quantize_rows_fp8: out scale must be a contiguous fp32 [{m}] tensor on {dev}")
    with _on_device(dev):
        rc = lib().pli_quantize_rows_fp8(_ptr(x), max(x.stride(0), k) if m > 1 else k, _ptr(codes), _ldw(codes),
                                         _ptr(scale), m, k, _dtype_code(x), _stream(dev))
    _check(rc, "pli_quantize_rows_fp8")
    return codes, scale


def _check_fp8a(what: str, x8: torch.Tensor, x_scale, w8: torch.Tensor, w_scale) -> torch.device:
    if not x8.is_cuda or not w8.is_cuda:
        raise PliError("HIP path called with a CPU tensor")
    dev = x8.device
    if x8.dim() != 2 or w8.dim() != 2 or x8.shape[1] != w8.shape[1]:
        raise PliError(f"{what} shape mismatch: x8{tuple(x8.shape)} w8{tuple(w8.shape)}")
    for name, codes, scale in (("x", x8, x_scale), ("w", w8, w_scale)):
        if codes.device != dev or codes.dtype not in FP8_POOL_DTYPES:
            raise PliError(f"{what}: {name}8 must be a torch.float8_e4m3fn or torch.uint8 tensor on {dev}, "
                           f"got {codes.dtype} on {codes.device}")
        if codes.numel() and codes.stride(1) != 1:
            raise PliError(f"{what}: {name}8 needs a unit column stride (the codes are used in place)")
        rows = codes.shape[0]
        if scale is not None and (not scale.is_cuda or scale.device != dev or scale.dtype != torch.float32 or
                                  tuple(scale.shape) != (rows,) or not scale.is_contiguous()):
            raise PliError(f"{what}: {name}_scale must be None or a contiguous fp32 [{rows}] tensor on {dev}")
    return dev


def gemm_fp8(x8: torch.Tensor, x_scale: torch.Tensor | None, w8: torch.Tensor, w_scale: torch.Tensor | None,
             bias: torch.Tensor | None = None, out_dtype: torch.dtype = torch.bfloat16,
             out: torch.Tensor | None = None) -> torch.Tensor:
    """C = (x_scale[:, None] * decode(x8)) (w_scale[:, None] * decode(w8))^T (+ bias) over two operands of e4m3fn
    codes: x8 [m, k], w8 [n, k] (float8_e4m3fn or uint8, any row stride, used in place), scales fp32 [m] / [n] or None
    (ones), C and bias ``out_dtype`` (bf16 / fp16).  fp32 sum, scales and bias after the sum, one rounding."""
    dev = _check_fp8a("gemm_fp8", x8, x_scale, w8, w_scale)
    if out_dtype not in (torch.float16, torch.bfloat16):
        raise PliError(f"gemm_fp8: out_dtype must be fp16 or bf16, got {out_dtype}")
    m, k = x8.shape
    n = w8.shape[0]
    if bias is not None:
        if not bias.is_cuda or bias.device != dev or bias.dtype != out_dtype or tuple(bias.shape) != (n,):
            raise PliError(f"gemm_fp8: bias must be a {out_dtype} [{n}] tensor on {dev}")
        bias = bias.contiguous()
    if out is None:
        out = torch.empty((m, n), dtype=out_dtype, device=dev)
    else:
        if out.dtype != out_dtype:
            raise PliError(f"gemm_fp8: out is {out.dtype}, out_dtype {out_dtype}")
        _check_out(out, out, (m, n), "gemm_fp8")
        if out.device != dev:
            raise PliError(f"tensors on different devices: {out.device} vs {dev}")
    with _on_device(dev):
        rc = lib().pli_gemm_fp8(_ptr(x8), _ptr(x_scale), _ptr(w8), _ptr(w_scale), _ptr(bias), _ptr(out), m, n, k,
                                _ldw(x8), _ldw(w8), max(out.stride(0), n), DTYPE_CODE[out_dtype], _stream(dev))
    _check(rc, "pli_gemm_fp8")
    return out


def linear_fp8a(x: torch.Tensor, w8: torch.Tensor, w_scale: torch.Tensor | None, bias: torch.Tensor | None = None,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """x W^T (+ bias) with both operands in fp8: quantize_rows_fp8(x), then gemm_fp8 against the weight codes
    (W = decode(w8) * w_scale[:, None], as linear_fp8w takes them); the result has x's dtype.  Bitwise the two calls."""
    if not x.is_cuda:
        raise PliError("HIP path called with a CPU tensor")
    x8, x_scale = quantize_rows_fp8(x)
    return gemm_fp8(x8, x_scale, w8, w_scale, bias=bias, out_dtype=x.dtype, out=out)


def _rms_gemm_fp8w(a: torch.Tensor, norm_weight: torch.Tensor, eps: float, groups: list,
                   residual: torch.Tensor | None, h_out: torch.Tensor | None, tokens_per_batch: int,
                   swiglu: bool) -> None:
    """pli_rms_gemm_nt_fp8w.  groups: ((codes, scale), (up codes, up scale) | None, c, stride_batch,
    stride_token, pos | None, capacity) with c the output base tensor."""
    dev = _require_gpu(a, norm_weight)
    a2 = _rows(a)
    r2 = _rows(residual) if residual is not None else None
    if r2 is not None:
        _require_gpu(a2, r2)
    if h_out is not None and (h_out.stride(-1) != 1 or tuple(h_out.shape[-1:]) != (a2.shape[1],)):
        raise PliError("h_out must have unit inner stride and the hidden width")
    h2 = h_out.view(-1, h_out.shape[-1]) if h_out is not None else None
    m, k = a2.shape
    for g in groups:
        _check_fp8w("rms_gemm_fp8w", a2, [g[0]] + ([g[1]] if swiglu else []))
        if swiglu and g[1][0].shape[0] > 1 and g[0][0].shape[0] > 1 and g[1][0].stride(0) != g[0][0].stride(0):
            raise PliError("rms_gemm_fp8w: the up codes need the gate codes' row stride")
        _require_gpu(a2, g[2])
    ng = len(groups)
    P = ctypes.c_void_p
    w = (P * ng)(*(g[0][0].data_ptr() for g in groups))
    ws = (P * ng)(*(_ptr(g[0][1]) for g in groups))
    wu = (P * ng)(*(g[1][0].data_ptr() for g in groups)) if swiglu else None
    wus = (P * ng)(*(_ptr(g[1][1]) for g in groups)) if swiglu else None
    c = (P * ng)(*(g[2].data_ptr() for g in groups))
    n = (_c_int * ng)(*(int(g[0][0].shape[0]) for g in groups))
    ldw = (_c_i64 * ng)(*(_ldw(g[0][0]) for g in groups))
    sb = (_c_i64 * ng)(*(int(g[3]) for g in groups))
    stok = (_c_i64 * ng)(*(int(g[4]) for g in groups))
    ro = (P * ng)(*(_ptr(g[5]) for g in groups))
    cap = (_c_int * ng)(*(int(g[6]) for g in groups))
    with _on_device(dev):
        rc = lib().pli_rms_gemm_nt_fp8w(_ptr(a2), a2.stride(0), _ptr(r2), r2.stride(0) if r2 is not None else 0,
                                        _ptr(norm_weight), float(eps), _ptr(h2),
                                        h2.stride(0) if h2 is not None else 0, m, k, int(tokens_per_batch),
                                        w, ws, wu, wus, c, n, ldw, sb, stok, ro, cap, ng, _dtype_code(a),
                                        _stream(dev))
    _check(rc, "pli_rms_gemm_nt_fp8w")


def rms_linear_fp8w(a: torch.Tensor, norm_weight: torch.Tensor, eps: float, codes: torch.Tensor,
                    scale: torch.Tensor | None, residual: torch.Tensor | None = None,
                    h_out: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """rmsnorm(a (+ residual)) @ W^T over fp8 weights in one launch (decode: <= 4 rows); codes [n, k] e4m3fn or
    uint8 used in place (any row stride % 16 == 0), scale fp32 [n] or None (ones)."""
    a2 = a.reshape(-1, a.shape[-1])
    n = codes.shape[0]
    if out is None:
        out = torch.empty(a2.shape[0], n, device=a.device, dtype=a.dtype)
    # one token per "batch": row bb lands at out + bb * stride(0)
    _rms_gemm_fp8w(a, norm_weight, eps, [((codes, scale), None, out, out.stride(0), 0, None, 1 << 30)],
                   residual, h_out, 1, False)
    return out.view(*a.shape[:-1], n)


def rms_swiglu_fp8w(a: torch.Tensor, norm_weight: torch.Tensor, eps: float, g_codes: torch.Tensor,
                    g_scale: torch.Tensor | None, u_codes: torch.Tensor, u_scale: torch.Tensor | None,
                    residual: torch.Tensor | None = None, h_out: torch.Tensor | None = None,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """silu(y Wg^T) * (y Wu^T) with y = rmsnorm(a (+ residual)) over fp8 gate / up weights, one launch."""
    a2 = a.reshape(-1, a.shape[-1])
    n = g_codes.shape[0]
    if out is None:
        out = torch.empty(a2.shape[0], n, device=a.device, dtype=a.dtype)
    _rms_gemm_fp8w(a, norm_weight, eps,
                   [((g_codes, g_scale), (u_codes, u_scale), out, out.stride(0), 0, None, 1 << 30)],
                   residual, h_out, 1, True)
    return out.view(*a.shape[:-1], n)


def rms_qkv_into_cache_fp8w(a: torch.Tensor, norm_weight: torch.Tensor, eps: float, q: tuple, k: tuple, v: tuple,
                            q_out: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: torch.Tensor,
                            residual: torch.Tensor | None = None,
                            h_out: torch.Tensor | None = None) -> torch.Tensor:
    """rms_qkv_into_cache over fp8 weights, one launch; a [B, S, hidden]; q / k / v are (codes, scale) pairs
    (row blocks of one packed [Wq; Wk; Wv] serve as they are)."""
    B, S, _ = a.shape
    S_max, Hkv, D = k_cache.shape[1:]
    if pos.dtype != torch.int32 or not pos.is_cuda:
        raise PliError("pos must be an int32 device tensor")
    for t in (k_cache, v_cache):
        if t.shape[0] != B or t.stride(3) != 1 or t.stride(2) != D:
            raise PliError("caches must be [B, S_max, Hkv, D] with contiguous (Hkv, D) rows")
    if q_out.dim() != 3 or tuple(q_out.shape[:2]) != (B, S) or q_out.stride(2) != 1:
        raise PliError("q_out must be [B, S, Hq*D] with unit inner stride")
    groups = [(q, None, q_out, q_out.stride(0), q_out.stride(1), None, S),
              (k, None, k_cache, k_cache.stride(0), k_cache.stride(1), pos, S_max),
              (v, None, v_cache, v_cache.stride(0), v_cache.stride(1), pos, S_max)]
    _rms_gemm_fp8w(a, norm_weight, eps, groups, residual, h_out, S, False)
    return q_out


# ---------------------------------------------------------------------- GEMV
def gemv(w: torch.Tensor, x: torch.Tensor, out: torch.Tensor | None = None,
         variant: int | None = None) -> torch.Tensor:
    """y = W x (torch.mv semantics), W [m, k] with unit column stride."""
    dev = _require_gpu(w, x)
    if w.dim() != 2 or x.dim() != 1 or w.shape[1] != x.shape[0]:
        raise PliError(f"gemv shape mismatch {tuple(w.shape)} x {tuple(x.shape)}")
    if w.stride(1) != 1:
        w = w.contiguous()
    x = x.contiguous()
    m, k = w.shape
    if out is None:
        out = torch.empty(m, dtype=w.dtype, device=dev)
    else:
        _check_out(out, w, (m,), "gemv")
    args = (_ptr(w), _ptr(x), _ptr(out), m, k, max(w.stride(0), k), _dtype_code(w), _stream(dev))
    with _on_device(dev):
        if variant is None:
            rc = lib().pli_gemv(*args)
        else:
            rc = lib().pli_gemv_variant(*args, int(variant))
    _check(rc, "pli_gemv")
    return out


# ---------------------------------------------------------------------- GEMM
def gemm(a: torch.Tensor, b: torch.Tensor, trans_b: bool = False,
         bias: torch.Tensor | None = None, out: torch.Tensor | None = None,
         variant: int | None = None) -> torch.Tensor:
    """C = A B (trans_b=False, torch.mm) or A B^T (+ bias) (trans_b=True, F.linear)."""
    ts = (a, b) if bias is None else (a, b, bias)
    dev = _require_gpu(*ts)
    if a.dim() != 2 or b.dim() != 2:
        raise PliError("gemm expects 2-D operands")
    m, k = a.shape
    n, kb = (b.shape if trans_b else (b.shape[1], b.shape[0]))
    if kb != k:
        raise PliError(f"gemm inner dims differ: {tuple(a.shape)} vs {tuple(b.shape)} trans_b={trans_b}")
    if a.stride(1) != 1:
        a = a.contiguous()
    if b.stride(1) != 1:
        b = b.contiguous()
    if bias is not None:
        bias = bias.contiguous()
        if bias.shape != (n,):
            raise PliError(f"bias must be [{n}]")
    if out is None:
        out = torch.empty((m, n), dtype=a.dtype, device=dev)
    else:
        _check_out(out, a, (m, n), "gemm")
    lda = a.stride(0) if m > 1 else k
    ldb = b.stride(0) if b.shape[0] > 1 else b.shape[1]
    head = (_ptr(a), _ptr(b), _ptr(out), _ptr(bias), m, n, k, max(lda, 1), max(ldb, 1),
            max(out.stride(0), n), int(bool(trans_b)), _dtype_code(a))
    with _on_device(dev):
        # decode-batch NT shapes split K over workgroups through a scratch
        # workspace from torch's caching allocator (pli_gemm_ws)
        wsb = lib().pli_gemm_workspace_size(m, n, k, int(bool(trans_b)), _dtype_code(a)) \
            if variant in (None, 0, 22, 24, 25, 26, 27, 28, 29) else 0
        if wsb:
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            if variant is None:
                rc = lib().pli_gemm_ws(*head, _ptr(ws), wsb, _stream(dev))
            else:
                rc = lib().pli_gemm_ws_variant(*head, _ptr(ws), wsb, _stream(dev), int(variant))
        elif variant is None:
            rc = lib().pli_gemm(*head, _stream(dev))
        else:
            rc = lib().pli_gemm_variant(*head, _stream(dev), int(variant))
    _check(rc, "pli_gemm")
    return out


def gemm_naive(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """C = A B for fp32 [M,K] x [K,N] with the ch05 naive kernel
    (pli_gemm_naive, one thread per output) -- the demo's contrast, not a
    production path."""
    dev = _require_gpu(a, b)
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.dim() != 2 or b.dim() != 2:
        raise PliError("gemm_naive expects 2-D fp32 operands")
    if a.shape[1] != b.shape[0]:
        raise PliError(f"gemm_naive inner dims differ: {tuple(a.shape)} vs {tuple(b.shape)}")
    a, b = a.contiguous(), b.contiguous()
    m, k = a.shape
    n = b.shape[1]
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=dev)
    else:
        _check_out(out, a, (m, n), "gemm_naive")
    with _on_device(dev):
        rc = lib().pli_gemm_naive(_ptr(a), _ptr(b), _ptr(out), m, n, k, max(k, 1), max(n, 1),
                                  max(out.stride(0), n), _stream(dev))
    _check(rc, "pli_gemm_naive")
    return out


# -------------------------------------------------------------- calibration
def scale_copy(inp: torch.Tensor, out: torch.Tensor, stride: int = 1) -> torch.Tensor:
    """out[i] = 2 * inp[i * stride] (fp32), the ch05/coalescing.cu probes."""
    dev = _require_gpu(inp, out)
    if inp.dtype != torch.float32 or not inp.is_contiguous() or not out.is_contiguous():
        raise PliError("scale_copy expects contiguous fp32 tensors")
    n_out = out.numel()
    if (n_out - 1) * stride >= inp.numel() and n_out > 0:
        raise PliError("scale_copy: input too short for stride")
    with _on_device(dev):
        rc = lib().pli_scale_copy(_ptr(inp), _ptr(out), n_out, int(stride), _stream(dev))
    _check(rc, "pli_scale_copy")
    return out


# ------------------------------------------------------------------ softmax
def gemm_f32out(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [m, n] = x [m, k] @ w [n, k]^T for bf16 / fp16 x, w (pli_gemm_f32out):
    the row-parallel partial kept unrounded for the all-reduce."""
    dev = _require_gpu(x, w)
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise PliError(f"gemm_f32out: x {tuple(x.shape)} and w {tuple(w.shape)} must be [m, k] and [n, k]")
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise PliError("gemm_f32out: bf16 / fp16 inputs only")
    x = x if x.stride(1) == 1 else x.contiguous()
    w = w if w.stride(1) == 1 else w.contiguous()
    m, k = x.shape
    n = w.shape[0]
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or tuple(out.shape) != (m, n) or not out.is_contiguous() or out.device != dev:
        raise PliError("gemm_f32out: out must be a contiguous fp32 [m, n] tensor on the inputs' device")
    with _on_device(dev):
        rc = lib().pli_gemm_f32out(_ptr(x), _ptr(w), _ptr(out), m, n, k, x.stride(0), w.stride(0),
                                   _dtype_code(x), _stream(dev))
    _check(rc, "pli_gemm_f32out")
    return out


def mfma_probe(out: torch.Tensor, blocks: int, iters: int, shape: int = 0,
               clocks: torch.Tensor | None = None) -> torch.Tensor:
    """Launch the MFMA calibration kernel (pli_mfma_probe): ``blocks`` x 256
    threads, one workgroup per CU, ``iters`` rounds of 262,144 bf16 MFMA FLOP
    per wave (shape 0: 8 x 32x32x16, 1: 16 x 16x16x32); FLOPs = blocks * 4 *
    iters * 262144.  ``clocks`` (int64, >= blocks * 8, optional) receives per
    wave the s_memtime and s_memrealtime (100 MHz) ticks around the loop."""
    dev = _require_gpu(out)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < blocks * 256:
        raise PliError("mfma_probe: out must be contiguous fp32 with >= blocks*256 elements")
    if clocks is not None:
        if _require_gpu(clocks) != dev:
            raise PliError("mfma_probe: clocks on another device")
        if clocks.dtype != torch.int64 or not clocks.is_contiguous() or clocks.numel() < blocks * 8:
            raise PliError("mfma_probe: clocks must be contiguous int64 with >= blocks*8 elements")
    with _on_device(dev):
        rc = lib().pli_mfma_probe(_ptr(out), _ptr(clocks), int(blocks), int(iters), int(shape), _stream(dev))
    _check(rc, "pli_mfma_probe")
    return out


def hbm_read_probe(buf: torch.Tensor, out: torch.Tensor, blocks: int, mode: int = 0) -> torch.Tensor:
    """Stream ``buf`` (contiguous, 16-byte multiple) with non-temporal 16-byte
    loads, ``blocks`` x 256 threads (pli_hbm_read_probe; mode 0 grid-stride,
    1 one contiguous slice per block); out: contiguous int32 >= blocks*256 on
    the same device."""
    dev = _require_gpu(buf)
    if _require_gpu(out) != dev:
        raise PliError("hbm_read_probe: out on another device")
    nbytes = buf.numel() * buf.element_size()
    if not buf.is_contiguous() or nbytes % 16:
        raise PliError("hbm_read_probe: buf must be contiguous with a multiple of 16 bytes")
    if out.dtype != torch.int32 or not out.is_contiguous() or out.numel() < blocks * 256:
        raise PliError("hbm_read_probe: out must be contiguous int32 with >= blocks*256 elements")
    with _on_device(dev):
        rc = lib().pli_hbm_read_probe(_ptr(buf), nbytes, _ptr(out), int(blocks), int(mode), _stream(dev))
    _check(rc, "pli_hbm_read_probe")
    return out


def softmax_rows(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Softmax over the last dim with the single-pass online (m, d) recurrence."""
    dev = _require_gpu(x)
    x = x.contiguous()
    n = x.shape[-1] if x.dim() > 0 else 1
    rows = x.numel() // max(n, 1)
    if out is None:
        out = torch.empty_like(x)
    with _on_device(dev):
        rc = lib().pli_softmax_rows(_ptr(x), _ptr(out), rows, n, _dtype_code(x), _stream(dev))
    _check(rc, "pli_softmax_rows")
    return out


def online_softmax_with_output(x: torch.Tensor, v: torch.Tensor):
    """(o, d): softmax(x)-weighted rows of v, and the denominator at the final max."""
    dev = _require_gpu(x, v)
    x, v = x.contiguous(), v.contiguous()
    n, dv = x.shape[-1], v.shape[-1]
    if tuple(v.shape[:-1]) != tuple(x.shape):
        raise PliError(f"v shape {tuple(v.shape)} does not match x {tuple(x.shape)}")
    rows = x.numel() // n
    o = torch.empty(x.shape[:-1] + (dv,), dtype=x.dtype, device=dev)
    d = torch.empty(x.shape[:-1], dtype=x.dtype, device=dev)
    with _on_device(dev):
        rc = lib().pli_online_softmax_with_output(_ptr(x), _ptr(v), _ptr(o), _ptr(d), rows, n, dv,
                                                  _dtype_code(x), _stream(dev))
    _check(rc, "pli_online_softmax_with_output")
    return o, d
