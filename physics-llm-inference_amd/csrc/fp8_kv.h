// Device helpers of the fp8 e4m3 KV pool (gfx950): the hardware conversions
// the fast kernels and the quantising appends use.  fp8_codec.h is the
// reference they are tested against (tests/test_gpu_fp8_kv.py).
#pragma once

#include <type_traits>

#include "fp8_codec.h"
#include "pli_common.h"

namespace pli {

// Two codes (the low or the high half of w) -> one dword of two T, exact:
// v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.
template <typename T, bool HI> __device__ __forceinline__ uint32_t fp8_widen2(uint32_t w) {
    if constexpr (std::is_same<T, bf16_t>::value)
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
    else
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, HI));
}
// 16 codes (one 16-byte load) -> 16 T in element order: lo = elements 0..7, hi = 8..15
template <typename T> __device__ __forceinline__ void fp8_widen16(i32x4 x, i32x4& lo, i32x4& hi) {
    lo = i32x4{(int)fp8_widen2<T, false>(x.x), (int)fp8_widen2<T, true>(x.x), (int)fp8_widen2<T, false>(x.y),
               (int)fp8_widen2<T, true>(x.y)};
    hi = i32x4{(int)fp8_widen2<T, false>(x.z), (int)fp8_widen2<T, true>(x.z), (int)fp8_widen2<T, false>(x.w),
               (int)fp8_widen2<T, true>(x.w)};
}

// 8 codes (one 8-byte load) -> 8 T
template <typename T> __device__ __forceinline__ i32x4 fp8_widen8(i32x2 x) {
    return i32x4{(int)fp8_widen2<T, false>(x.x), (int)fp8_widen2<T, true>(x.x), (int)fp8_widen2<T, false>(x.y),
                 (int)fp8_widen2<T, true>(x.y)};
}

// fp8_e4m3_encode(x * inv) of four values into one dword (x0 in bits 0..7) by
// v_cvt_pk_fp8_f32.  The clamp to +-448 is explicit and keeps NaN (both
// comparisons are false for it); a NaN's code is then set by hand, so the
// result does not depend on what the instruction does with one.
__device__ __forceinline__ float fp8_clamp448(float y) {
    y = y > 448.f ? 448.f : y;
    return y < -448.f ? -448.f : y;
}
__device__ __forceinline__ uint32_t fp8_encode4(float x0, float x1, float x2, float x3, float inv) {
    const float y[4] = {fp8_clamp448(x0 * inv), fp8_clamp448(x1 * inv), fp8_clamp448(x2 * inv),
                        fp8_clamp448(x3 * inv)};
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w, true);
    uint32_t r = (uint32_t)w;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (y[i] != y[i]) r = (r & ~(0xffu << (8 * i))) | (((__float_as_uint(y[i]) >> 24) & 0x80u) | 0x7fu) << (8 * i);
    return r;
}

// 8 consecutive source elements of T (fp32 / fp16 / bf16, 16-byte aligned) -> 8 codes
template <typename T> __device__ __forceinline__ i32x2 fp8_encode8(const char* src, float inv) {
    float x[8];
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
    return i32x2{(int)fp8_encode4(x[0], x[1], x[2], x[3], inv), (int)fp8_encode4(x[4], x[5], x[6], x[7], inv)};
}

// The scales of a call: device fp32 [kv_heads], NULL means all ones.
struct Fp8Scales {
    const float *k, *v;
};
// scale[h] of one of them
__device__ __forceinline__ float fp8_scale_of(const float* __restrict__ s, int h) { return s ? s[h] : 1.f; }

}  // namespace pli
