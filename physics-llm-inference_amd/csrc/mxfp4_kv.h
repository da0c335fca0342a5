// Device helpers of the MXFP4 KV pool (gfx950): the scaled hardware widening
// the fast decode kernel runs between its global loads and its LDS writes, and
// the exact block quantiser of the appends.  fp4_codec.h is the reference both
// are tested against (tests/test_gpu_mxfp4_kv.py); the encode is that of
// quant_mxfp4.hip without a row scale.
#pragma once

#include <type_traits>

#include "fp4_codec.h"
#include "pli_common.h"

namespace pli {

constexpr int kKv4Block = 32;               // elements under one E8M0 byte
constexpr int kKv4ExpLo = -13, kKv4ExpHi = 13;  // what the appends write: inside the fp16 and the bf16 read contract

// Byte SEL of w (two codes) -> one dword of two T, each decode(code) * sc:
// v_cvt_scalef32_pk_{bf16,f16}_fp4, exact while the product is a normal T.
template <typename T, int SEL> __device__ __forceinline__ int kv4_widen2(uint32_t w, float sc) {
    if constexpr (std::is_same<T, bf16_t>::value)
        return __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, SEL));
    else
        return __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, SEL));
}
template <typename T> __device__ __forceinline__ i32x4 kv4_widen8(uint32_t w, float sc) {
    return i32x4{kv4_widen2<T, 0>(w, sc), kv4_widen2<T, 1>(w, sc), kv4_widen2<T, 2>(w, sc), kv4_widen2<T, 3>(w, sc)};
}
// One block (a 16-byte load) at scale sc -> 32 T in element order, o[h] = elements 8 h .. 8 h + 7.
template <typename T> __device__ __forceinline__ void kv4_widen32(const i32x4& x, float sc, i32x4 (&o)[4]) {
    o[0] = kv4_widen8<T>((uint32_t)x.x, sc);
    o[1] = kv4_widen8<T>((uint32_t)x.y, sc);
    o[2] = kv4_widen8<T>((uint32_t)x.z, sc);
    o[3] = kv4_widen8<T>((uint32_t)x.w, sc);
}
// The fp32 operand of the conversion for scale byte s: 2^(s - 127), whose
// pattern is s << 23 for every byte of the read contract.  `bad` (a 0xFF byte
// in the key's K or V block) gives 1.0: the block's values stay finite and the
// NaN enters through the key's score alone (kv4_nan_pair), so it reaches
// exactly the rows that see the key.
__device__ __forceinline__ float kv4_scale_f32(uint32_t s, bool bad) {
    return __uint_as_float(bad ? 0x3f800000u : s << 23);
}
// What a bad K block's first widened pair becomes: a NaN in q . k poisons the
// key's score, hence P and every output element, of each row it is not masked for.
template <typename T> __device__ __forceinline__ int kv4_nan_pair(bool bad, int pair) {
    constexpr int kNaN2 = std::is_same<T, bf16_t>::value ? 0x7fc07fc0 : 0x7e007e00;
    return bad ? kNaN2 : pair;
}

// ---- the appends' quantiser ---------------------------------------------------
// 8 consecutive source elements of T (fp32 / fp16 / bf16, 16-byte aligned) as fp32
template <typename T> __device__ __forceinline__ void kv4_read8(const char* src, float (&x)[8]) {
    if constexpr (std::is_same<T, float>::value) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = a[i], x[4 + i] = b[i];
    } else {
        const i32x4 a = *reinterpret_cast<const i32x4*>(src);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = elem<T>::to_f32(T{(uint16_t)((uint32_t)a[i] & 0xffffu)});
            x[2 * i + 1] = elem<T>::to_f32(T{(uint16_t)((uint32_t)a[i] >> 16)});
        }
    }
}
// Block exponent of amax (>= 0, finite) given as its fp32 pattern:
// floor(log2(amax)) - 2 is the exponent field - 129; an fp32 subnormal lands
// below the clamp like everything under 2^-11; 0 for an all-zero block.
PLI_HD inline int kv4_block_exp(uint32_t amax_bits) {
    if (amax_bits == 0) return 0;
    const int e = (int)(amax_bits >> 23) - 129;
    return e < kKv4ExpLo ? kKv4ExpLo : (e > kKv4ExpHi ? kKv4ExpHi : e);
}
// One lane's quarter of a block: x are its 8 elements, the block is the four
// lanes tid & ~3 .. + 3 (all live together).  Returns the eight codes, element
// 0 in bits 3:0, and the block's scale byte in `byte`.  Every step is exact:
// integer arithmetic on the amax pattern, a power-of-two scaling
// (v_ldexp_f32; a result below 2^-126 encodes to 0 whether it is kept as a
// subnormal or not) and fp4_e2m1_encode's compare chain.
__device__ __forceinline__ uint32_t kv4_encode8(const float (&x)[8], uint32_t& byte) {
    float amax = 0.f;
    int nan = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float a = fabsf(x[i]);
        amax = fmaxf(amax, a < __builtin_inff() ? a : 0.f);  // the comparison is false for NaN and inf
        nan |= x[i] != x[i];
    }
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
        amax = fmaxf(amax, __shfl_xor(amax, o, 64));
        nan |= __shfl_xor(nan, o, 64);
    }
    const int e = kv4_block_exp(__float_as_uint(amax));
    byte = nan ? 0xffu : (uint32_t)(e + 127);
    uint32_t codes = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        codes |= (x[i] != x[i] ? 0u : (uint32_t)fp4_e2m1_encode(__builtin_ldexpf(x[i], -e))) << (4 * i);
    return codes;
}

}  // namespace pli
