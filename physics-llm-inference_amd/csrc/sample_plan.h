// Next-token sampling (pli_sample, csrc/sample.hip) as pure C++17 (no HIP
// headers): everything of the rule a test has to replay on the host.  The
// functions carry PLI_HD (paged_plan.h): the same text runs in the kernel, in
// its launcher and in tests/host/sample_plan_check.cpp
// (tests/test_sample_plan.py).
//
//   - Philox4x32-10 and the map from its first output word to the uniform u;
//   - the order-preserving integer key of a logit with the rule's
//     canonicalisation (NaN counts as -inf, -0 as +0), its inverse, and the
//     8-bit digits the radix select walks from the top;
//   - the weight exp((x - m) / temperature) as a 45-bit fixed-point integer:
//     every sum that feeds a decision (S1, the top-p prefix weights, S2, the
//     draw's running sum) is a sum of these integers, so it is exact, has no
//     order and is the same on every call and every replay;
//   - the launch configuration: one workgroup of kSampleWaves waves per row,
//     wave w owns the contiguous segment [w * seg, (w + 1) * seg) of the row
//     and walks it 64 elements a step, so that "lower index first" is "lower
//     wave, lower step, lower lane first".
#pragma once

#include <cmath>
#include <cstdint>

#include "paged_plan.h"

namespace pli {

constexpr int kSampleWaves = 16;                       // waves of 64 lanes per workgroup (one row)
constexpr int kSampleThreads = kSampleWaves * 64;      // 1024: the elements all waves take in one step
constexpr int kSampleMaxVocab = 262144;                // 2^18 weights of at most 2^45 sum below 2^64
constexpr int kSampleFracBits = 45;                    // weight 1.0 = 2^45
constexpr uint64_t kSampleOne = (uint64_t)1 << kSampleFracBits;
constexpr int kSampleDigitBits = 8;

// ---------------------------------------------------------------- Philox --
struct Philox4 {
    uint32_t v[4];
};

PLI_HD inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                    uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// 24 random bits -> u in [0, 1): every value is an fp32
PLI_HD inline float sample_bits_to_u(uint32_t r0) { return (float)(r0 >> 8) * 5.9604644775390625e-08f; }

// u of one row: counter {(uint32)offset, row, 0, 0}, key {seed lo, seed hi}
PLI_HD inline float sample_philox_u(uint64_t seed, int64_t offset, uint32_t row) {
    return sample_bits_to_u(
        philox4x32_10((uint32_t)(uint64_t)offset, row, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32)).v[0]);
}

// ------------------------------------------------------------------- keys --
// fp32 bits -> key: a > b as numbers <=> key(a) > key(b); NaN -> key(-inf), -0 -> key(+0)
PLI_HD inline uint32_t sample_key_f32(uint32_t bits) {
    if ((bits & 0x7fffffffu) > 0x7f800000u) bits = 0xff800000u;
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
// the same on the 16 bits of an fp16 (exponent mask 0x7c00) or a bf16 (0x7f80) value
PLI_HD inline uint32_t sample_key_16(uint32_t bits, uint32_t inf_bits) {
    if ((bits & 0x7fffu) > inf_bits) bits = 0x8000u | inf_bits;
    if (bits == 0x8000u) bits = 0u;
    return (bits & 0x8000u) ? (~bits & 0xffffu) : (bits | 0x8000u);
}
// key -> the canonical bits (the inverse on canonical values)
PLI_HD inline uint32_t sample_unkey_f32(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }
PLI_HD inline uint32_t sample_unkey_16(uint32_t key) { return (key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu); }

// dtype codes of pli.h: 0 fp32, 1 fp16, 2 bf16
PLI_HD inline uint32_t sample_key(uint32_t bits, int dtype) {
    return dtype == 0 ? sample_key_f32(bits) : sample_key_16(bits, dtype == 1 ? 0x7c00u : 0x7f80u);
}
PLI_HD inline uint32_t sample_key_neg_inf(int dtype) { return sample_key(dtype == 0 ? 0xff800000u : dtype == 1 ? 0xfc00u : 0xff80u, dtype); }
PLI_HD inline uint32_t sample_key_pos_inf(int dtype) { return sample_key(dtype == 0 ? 0x7f800000u : dtype == 1 ? 0x7c00u : 0x7f80u, dtype); }
// 8-bit digit passes, most significant first: 4 for fp32 keys, 2 for 16-bit keys
PLI_HD inline int sample_digit_passes(int dtype) { return dtype == 0 ? 4 : 2; }
// digit `pass` (0 = most significant) of a key, and the key's bits above that digit
PLI_HD inline int sample_digit_shift(int pass, int dtype) { return (sample_digit_passes(dtype) - 1 - pass) * kSampleDigitBits; }
PLI_HD inline uint32_t sample_digit(uint32_t key, int pass, int dtype) { return (key >> sample_digit_shift(pass, dtype)) & 0xffu; }
PLI_HD inline uint32_t sample_prefix(uint32_t key, int pass, int dtype) {
    return pass == 0 ? 0u : key >> (sample_digit_shift(pass, dtype) + kSampleDigitBits);
}

// ---------------------------------------------------------------- weights --
// exp((x - m) / temperature) in fp32, then floor(w * 2^45) (the product is exact).  x == m gives exactly 2^45;
// x == -inf gives 0.  m == +inf is the caller's case (weight 1 for +inf, 0 for the rest).
PLI_HD inline uint64_t sample_weight_fx(float x, float m, float temperature) {
    if (!(x > -INFINITY)) return 0;  // (-inf / an infinite temperature would be NaN)
    const float w = expf((x - m) / temperature);
    return (uint64_t)(w * 35184372088832.0f);
}
// floor(f * s) for f in [0, 1]: top_p * S1 and u * S2 (one fp64 product of two exactly converted values)
PLI_HD inline uint64_t sample_scale_fx(float f, uint64_t s) { return (uint64_t)((double)f * (double)s); }

// ----------------------------------------------------------------- launch --
// elements of a row per wave: whole 64-element steps, kSampleWaves segments cover the row
PLI_HD inline int sample_seg_len(int vocab) { return 64 * ((vocab + kSampleThreads - 1) / kSampleThreads); }
PLI_HD inline int sample_seg_steps(int vocab) { return sample_seg_len(vocab) / 64; }
// element that lane `lane` of wave `wave` takes in step `step` (>= vocab: none)
PLI_HD inline int sample_index(int wave, int step, int lane, int seg) { return wave * seg + step * 64 + lane; }

}  // namespace pli
