// MXFP4 activations x MXFP4 weights (W4A4) as pure C++17 (no HIP headers): the
// scale contract of x_exp, the route rule of pli_gemm_mxfp4_a4, the index
// arithmetic of gemm_mxfp4_a4_mx (what every lane stages, which 16-byte chunk
// each e2m1 operand of the scaled MFMA reads, which E8M0 byte accompanies it on
// either side) and the arithmetic of quant_rows_mxfp4 (exponents, the element
// map).  The tile order, the operand image with its pieces and swizzle and the
// accumulator map are gemm_fp8_mx's (fp8a_plan.h), the scale-byte shift is
// gemm_mxfp4_mx's (mxfp4a_plan.h), all unchanged.  The functions carry PLI_HD
// (paged_plan.h), so the same text runs in the kernels and in the launchers of
// gemm_mxfp4_a4.hip and quant_mxfp4.hip.
//
// Layout: x4 [m, k / 2] and w4 [n, k / 2] bytes of two e2m1 codes (element i in
// byte i / 2, even i in bits 3:0; ldx4 / ldw in bytes), x_exp [m, k / 32] and
// w_exp [n, k / 32] E8M0 bytes (leading dimensions ldxs / lds), x_scale fp32
// [m]; C [m, n] 16-bit, ldc in elements.
#pragma once

#include <cstddef>
#include <cstdint>

#include "fp4_codec.h"
#include "mxfp4a_plan.h"

namespace pli {

// ---------------------------------------------------------- scale contract --
// x_exp - 127 in [kMxfp4xExpLo, kMxfp4xExpHi] = [-R, R], the largest R for
// which, against a weight byte at either end of its own contract (e_w = -+96),
// every non-zero term code x code x 2^(e_w + e_x) is a normal fp32 number:
//   smallest term 0.5 * 0.5 * 2^(-96 - R) >= 2^-126        <=>  R <= 28
//   largest term  6 * 6 * 2^(96 + R) = 1.125 * 2^(101 + R) < 2^128  <=>  R <= 26
// so R = 26: the terms lie in [2^-124, 36 * 2^122].  (At R = 28 the small end
// would still hold, but 36 * 2^124 is past the largest fp32 number.)
constexpr int kMxfp4xExpLo = -26;
constexpr int kMxfp4xExpHi = 26;

// ------------------------------------------------------------------ routes --
enum Mxfp4xRoute {
    MXFP4X_EMPTY = 0,    // m == 0 or n == 0: nothing; k == 0: bias or 0 (generic kernel)
    MXFP4X_MX = 1,       // gemm_mxfp4_a4_mx (v_mfma_scale_f32_32x32x64_f8f6f4, e2m1 x e2m1)
    MXFP4X_GENERIC = 2,  // gemm_mxfp4_a4_generic
};

constexpr int kMxfp4xKStep = 256;  // codes of k per stage: 128 bytes per row on both sides, eight blocks
constexpr int kMxfp4xStages = 2;   // LDS stages: step s + 1 lands while step s is multiplied
constexpr int kMxfp4xMinM = 17;    // below: the W4A16 decode kernels' ground
constexpr int kMxfp4xQuarters = kMxfp4xKStep / 64;                    // MFMA depths per step: 4
constexpr int kMxfp4xStepScales = kMxfp4xKStep / kMxfp4aBlock;        // scale bytes per row and step: 8, two dwords
constexpr int kMxfp4xStageBytes = 2 * kFp8aImgBytes;                  // W image, then X image: 32 KiB
constexpr int kMxfp4xLdsBytes = kMxfp4xStages * kMxfp4xStageBytes;    // 64 KiB

static_assert(kMxfp4xKStep / 2 == kFp8aRowBytes, "both operand images have the shape of gemm_fp8_mx's X image");

struct Mxfp4xCall {
    int m, n, k;
    int64_t ldx4, ldxs, ldw, lds, ldc;
    uintptr_t x4, x_exp, w4, w_exp, c;
};

PLI_HD inline bool mxfp4x_mx_ok(const Mxfp4xCall& a) {
    return a.m >= kMxfp4xMinM && a.k % kMxfp4xKStep == 0 && ((a.x4 | a.w4) & 15) == 0 && a.ldx4 % 16 == 0 &&
           a.ldw % 16 == 0 && ((a.x_exp | a.w_exp) & 3) == 0 && a.ldxs % 4 == 0 && a.lds % 4 == 0 &&
           a.n % kFp8aStoreN == 0 && a.ldc % kFp8aStoreN == 0 && (a.c & 7) == 0;
}

// The route of a call (k % 32 == 0 was checked), from host arguments only (a
// captured call replays).
PLI_HD inline int mxfp4x_route(const Mxfp4xCall& a) {
    if (a.m <= 0 || a.n <= 0 || a.k <= 0) return MXFP4X_EMPTY;
    if (mxfp4x_mx_ok(a)) return MXFP4X_MX;
    return MXFP4X_GENERIC;
}

// -------------------------------------------------------- gemm_mxfp4_a4_mx --
// Staging: both images are [128 rows][8 chunks of 16 bytes], the pieces, the
// lane -> (row, chunk) map, the swizzle and the source offset are
// fp8a_stage_* / fp8a_src_off with a step of 128 bytes = 256 codes.
//
// Fragments.  Of the 64 k of one instruction a 4-register e2m1 operand holds
// k = 32 (lane >> 5) + j in element j (nibble j & 1 of byte j >> 1), on the A
// side (cbsz = 4, settled by gemm_mxfp4_mx) and on the B side (blgp = 4): the
// operand of tile t, k-quarter q (64 codes) of a lane is the one 16-byte chunk
// 2 q + (lane >> 5) of row fp8a_frag_row(wq, t, lane), read at
// fp8a_frag_lds(row, chunk).  A phase of that read (16 consecutive rows of one
// chunk) takes slots 8 (row & 1) + (chunk ^ ((row >> 1) & 7)) modulo 16: all
// different, no bank conflict.
PLI_HD inline int mxfp4x_frag_chunk(int q, int lane) { return 2 * q + (lane >> 5); }
// k (inside the K-step) of element j of that operand
PLI_HD inline int mxfp4x_frag_k(int q, int lane, int j) { return 64 * q + 32 * (lane >> 5) + j; }

// Scale bytes.  Per K-step and tile a lane loads the two dwords of the eight
// scale bytes of its row (clamped like the codes), blocks 8 step .. 8 step + 7.
// The instruction takes byte 0 of lane l's scale register as the scale of row
// (A) / column (B) l & 31 over the 32 k of lane half l >> 5, so the operand of
// quarter q is dword q >> 1 shifted right by mxfp4a_scale_shift(q & 1, lane):
// its byte 0 is block 2 q + (lane >> 5).
PLI_HD inline int64_t mxfp4x_scale_off(int row0, int row, int rows, int64_t ld, int step) {
    const int r = row0 + row < rows ? row0 + row : rows - 1;
    return (int64_t)r * ld + (int64_t)step * kMxfp4xStepScales;
}
PLI_HD inline int mxfp4x_scale_dword(int q) { return q >> 1; }
PLI_HD inline int mxfp4x_scale_shift(int q, int lane) { return mxfp4a_scale_shift(q & 1, lane); }
PLI_HD inline int mxfp4x_scale_block(int q, int lane) { return 2 * q + (lane >> 5); }

// -------------------------------------------------------- quant_rows_mxfp4 --
// One workgroup of 256 threads per row.  Vector class: thread t takes the
// 8-element chunks t, t + 256, ...; a block of 32 is the chunks of four
// adjacent lanes; the first kMxfp4xQuantHeld chunks stay in registers between
// the row amax and the encode, so a row of up to kMxfp4xQuantRegK elements is
// read once and the rest of a longer one twice.  Scalar class: thread t takes
// whole blocks t, t + 256, ... and reads them once per pass.
constexpr int kMxfp4xQuantThreads = 256;
constexpr int kMxfp4xQuantHeld = 4;
constexpr int kMxfp4xQuantRegK = 8 * kMxfp4xQuantThreads * kMxfp4xQuantHeld;  // 8192
PLI_HD inline bool mxfp4x_quant_vec(int64_t ldx, int64_t ldx4, int64_t ldxs, uintptr_t x, uintptr_t x4,
                                    uintptr_t x_exp) {
    return ldx % 8 == 0 && ldx4 % 4 == 0 && ldxs % 4 == 0 && (x & 15) == 0 && (x4 & 3) == 0 && (x_exp & 3) == 0;
}
PLI_HD inline int mxfp4x_quant_item(int t, int u) { return t + kMxfp4xQuantThreads * u; }
PLI_HD inline int mxfp4x_quant_trips(int items) { return (items + kMxfp4xQuantThreads - 1) / kMxfp4xQuantThreads; }

// floor(log2(a)) of a finite a > 0 given as fp32 bits (sign clear), subnormals included
PLI_HD inline int mxfp4x_floor_log2(uint32_t bits) {
    const int e = (int)(bits >> 23);
    if (e) return e - 127;
    return 31 - __builtin_clz(bits) - 149;  // bits != 0: the top mantissa bit
}
// fp32 bits of 2^e, -149 <= e <= 127
PLI_HD inline uint32_t mxfp4x_pow2_bits(int e) { return e >= -126 ? (uint32_t)(e + 127) << 23 : 1u << (e + 149); }
// E_r of a row (amax over its finite elements, as fp32 bits); 0 for amax == 0
PLI_HD inline int mxfp4x_row_exp(uint32_t amax_bits) { return amax_bits ? mxfp4x_floor_log2(amax_bits) - 2 : 0; }
// e_b of a block against its row's E_r: never positive (the block's amax is at most the row's)
PLI_HD inline int mxfp4x_block_exp(uint32_t amax_bits, int row_exp) {
    if (!amax_bits) return 0;
    const int e = mxfp4x_floor_log2(amax_bits) - 2 - row_exp;
    return e < kMxfp4xExpLo ? kMxfp4xExpLo : e;
}
// the scale byte of a block; a NaN element anywhere in it: 0xFF
PLI_HD inline uint8_t mxfp4x_block_byte(int block_exp, bool has_nan) { return has_nan ? 0xFF : (uint8_t)(127 + block_exp); }

}  // namespace pli
