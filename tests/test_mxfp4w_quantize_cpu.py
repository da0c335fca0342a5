"""pli_hip.quantize_weight_mxfp4 / dequantize_weight_mxfp4 on CPU tensors: the OCP MX rule per block of 32 against a
brute-force nearest-of-16 in float64 over a spread of block magnitudes (every tie, an all-zero block, blocks past both
ends of each dtype's exponent range, where the clamp bites), the round trip, and ValueError on a non-finite weight."""
import numpy as np
import pytest
import torch

MAGS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
RANGE = {torch.bfloat16: (-125, 125), torch.float16: (-13, 13)}


def brute_force(w, dtype):
    """float64: e = floor(log2 amax) - 2 clamped (0 for a zero block), code nearest to clamp(w / 2^e, +-6), ties even"""
    n, k = w.shape
    blk = w.astype(np.float64).reshape(n, k // 32, 32)
    amax = np.abs(blk).max(axis=2)
    with np.errstate(divide="ignore"):
        e = np.where(amax > 0, np.floor(np.log2(amax)) - 2, 0.0).clip(*RANGE[dtype])
    d = np.abs(np.minimum(np.abs(blk) / np.exp2(e)[:, :, None], 6.0)[..., None] - MAGS)
    mag = np.argmin(d + 1e-9 * (np.arange(8) % 2), axis=-1)  # among (exactly) equal distances the even code wins
    return (mag | (np.signbit(blk) << 3)).reshape(n, k), e.astype(np.int64)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_against_brute_force_over_block_magnitudes(built_lib, dtype):
    import pli_hip as pli
    (lo, hi), rs, n, k = RANGE[dtype], np.random.RandomState(7), 24, 256
    p = rs.randint(-14, 17, size=(n, k // 32))  # fp16: block exponents past both ends of the range
    w = (rs.standard_normal((n, k)) * np.repeat(np.exp2(p), 32, axis=1)).astype(np.float32)
    w[0, :64] = 0                                                                   # block 1 of row 0: all zero
    w[0, :9] = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -5.0, 6.0]) * 8  # amax 48: e = 3, every tie
    w[1, :32] *= np.float32(2.0 ** (lo - 8 - p[1, 0]))             # below the range: e = lo
    w[1, 32:64] = np.float32(1.75 * 2.0 ** min(hi + 4, 127))       # at (bf16) / past (fp16) the top: e = hi, codes 6
    codes, exps = pli.quantize_weight_mxfp4(torch.from_numpy(w), dtype)
    want_code, want_e = brute_force(w, dtype)
    assert codes.dtype == exps.dtype == torch.uint8 and tuple(codes.shape) == (n, k // 2) and tuple(exps.shape) == (n, k // 32)
    assert want_e[0, 1] == 0 and want_e[1, 0] == lo and want_e[1, 1] == hi and (want_code[1, 32:64] == 7).all()
    assert np.array_equal(exps.numpy().astype(np.int64) - 127, want_e)
    assert np.array_equal(np.stack((codes.numpy() & 15, codes.numpy() >> 4), axis=2).reshape(n, k), want_code)
    deq = pli.dequantize_weight_mxfp4(codes, exps)
    assert np.array_equal(deq.double().numpy(),
                          np.where(want_code >= 8, -1.0, 1.0) * MAGS[want_code & 7] * np.repeat(np.exp2(want_e), 32, axis=1))
    again = pli.quantize_weight_mxfp4(deq, dtype)  # the round trip: dequantised weights quantise to themselves
    assert torch.equal(pli.dequantize_weight_mxfp4(*again), deq)
    exps[0, 1] = 0xFF
    assert bool(torch.isnan(pli.dequantize_weight_mxfp4(codes, exps)[0, 32:64]).all())
    for bad in (float("nan"), float("inf")):
        w[1, 5] = bad
        with pytest.raises(ValueError, match="non-finite"):
            pli.quantize_weight_mxfp4(torch.from_numpy(w), dtype)
