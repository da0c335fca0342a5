// OCP MXFP4 as pure C++17 (no HIP headers): the e2m1 element (1 sign, 2
// exponent bits with bias 1, 1 mantissa bit; magnitudes 0, 0.5, 1, 1.5, 2, 3,
// 4, 6; no infinity, no NaN, -0 is 0) and the E8M0 block scale (byte s is
// 2^(s - 127), 0xFF is NaN).  The functions carry PLI_HD (paged_plan.h), so
// the same text runs in mxfp4w_generic / mxfp4w_widen of linear_mxfp4w.hip
// and in tests/host/fp4_codec_check.cpp (tests/test_fp4_codec.py); it is also
// what the hardware conversions of the fast kernels are compared against.
//
// Packing (pli.h): element i of a row lives in byte i / 2, even i in bits
// 3:0, odd i in bits 7:4.
#pragma once

#include <cstdint>

#include "fp8_codec.h"

namespace pli {

// Exact: every e2m1 value is an fp32 (and a bf16, and an fp16) value.
PLI_HD inline float fp4_e2m1_decode(uint8_t code) {
    const uint32_t sign = (uint32_t)(code & 8) << 28;
    const uint32_t e = (code >> 1) & 3, m = code & 1;
    if (e == 0) return fp8_bits_f32(sign | (m ? 0x3f000000u : 0u));  // 0 or the subnormal 0.5
    return fp8_bits_f32(sign | (e + 126) << 23 | m << 22);
}
// element i (0: bits 3:0, 1: bits 7:4) of a packed byte
PLI_HD inline uint8_t fp4_nibble(uint8_t byte, int i) { return (uint8_t)((byte >> (4 * (i & 1))) & 15); }

// 2^(s - 127); s = 0 is the fp32 subnormal 2^-127, s = 0xFF is NaN
PLI_HD inline float e8m0_decode(uint8_t s) {
    if (s == 0xFF) return fp8_bits_f32(0x7fc00000u);
    return fp8_bits_f32(s ? (uint32_t)s << 23 : 0x00400000u);
}

// code = rne(clamp(x, -6, 6)): ties go to the even code (as values: 0.25 -> 0,
// 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), everything past +-6
// (infinities and NaN too) saturates to 6, the sign bit is kept (-0 -> 0x8).
PLI_HD inline uint8_t fp4_e2m1_encode(float x) {
    const uint8_t sign = (uint8_t)((fp8_f32_bits(x) >> 28) & 8);
    const float a = x < 0.f ? -x : x;
    if (a != a) return sign | 7;
    return sign | (uint8_t)((a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) +
                            (a > 5.f));
}

}  // namespace pli
