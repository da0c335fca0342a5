// OCP fp8 e4m3fn (1 sign, 4 exponent bits with bias 7, 3 mantissa bits; no
// infinity, NaN = 0x7F / 0xFF, largest finite 448 = 0x7E) as pure C++17 (no
// HIP headers), integer arithmetic only.  The functions carry PLI_HD
// (paged_plan.h), so the same text runs in the generic fp8 kernels of
// paged_attn.hip / varlen_attn.hip and in tests/host/fp8_codec_check.cpp
// (tests/test_fp8_codec.py); it is also what the hardware conversions of the
// fast kernels and of the quantising appends are compared against.
//
// The 1-byte KV pool (pli.h): value = code * scale[kv head].  The append
// stores code = fp8_e4m3_encode(x * (1.0f / scale)), product in fp32.
#pragma once

#include <cstdint>

#include "paged_plan.h"

namespace pli {

PLI_HD inline uint32_t fp8_f32_bits(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return u;
}
PLI_HD inline float fp8_bits_f32(uint32_t u) {
    float x;
    __builtin_memcpy(&x, &u, sizeof x);
    return x;
}

// Exact: every e4m3fn value is an fp32 (and a bf16, and an fp16) value.
PLI_HD inline float fp8_e4m3_decode(uint8_t code) {
    const uint32_t sign = (uint32_t)(code & 0x80) << 24;
    const uint32_t e = (code >> 3) & 15, m = code & 7;
    if (e == 15 && m == 7) return fp8_bits_f32(sign | 0x7fc00000u);
    if (e == 0) {
        // subnormal m * 2^-9: normalise m (1..7) by hand
        if (m == 0) return fp8_bits_f32(sign);
        const int top = m >= 4 ? 2 : (m >= 2 ? 1 : 0);  // position of m's leading one
        return fp8_bits_f32(sign | (uint32_t)(127 - 9 + top) << 23 | ((m << (23 - top)) & 0x7fffffu));
    }
    return fp8_bits_f32(sign | (e + 120) << 23 | m << 20);
}

// code = rne(clamp(x, -448, 448)): the clamp comes first, so everything past
// +-448 (infinities too) saturates to 0x7E / 0xFE; NaN keeps its sign and
// becomes 0x7F / 0xFF; ties go to the even code; -0 and everything that
// rounds to it is 0x80.
PLI_HD inline uint8_t fp8_e4m3_encode(float x) {
    const uint32_t u = fp8_f32_bits(x);
    const uint8_t sign = (uint8_t)((u >> 24) & 0x80);
    uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return sign | 0x7f;
    if (a > 0x43e00000u) a = 0x43e00000u;  // 448.0f
    const int E = (int)(a >> 23);          // biased by 127
    if (E >= 121) {
        // normal (>= 2^-6): keep 3 mantissa bits, a carry runs into the exponent
        const uint32_t r = (a + 0x7ffffu + ((a >> 20) & 1)) >> 20;
        return sign | (uint8_t)(r - (120u << 3));
    }
    // below 2^-6: the code is rne(|x| * 2^9) in 0 .. 8 (8 is the smallest normal)
    if (E == 0) return sign;  // zero and fp32 subnormals
    const int shift = 141 - E;  // |x| * 2^9 = mant * 2^-shift, shift >= 21
    if (shift > 25) return sign;
    const uint32_t mant = (a & 0x7fffffu) | 0x800000u;
    uint32_t q = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    return sign | (uint8_t)q;
}

}  // namespace pli
