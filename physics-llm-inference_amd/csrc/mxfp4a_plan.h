// MXFP4 weights x fp8 activations (W4A8) as pure C++17 (no HIP headers): the
// route rule of pli_gemm_mxfp4 and the W side of gemm_mxfp4_mx -- what every
// lane stages, where it lands in LDS, which nibble each e2m1 operand slot of
// the scaled MFMA reads, which E8M0 byte of w_exp accompanies it, and which k
// each byte of the e4m3 operand must hold against it.  The tile order, the X
// image and the accumulator map are gemm_fp8_mx's (fp8a_plan.h), unchanged.
// The functions carry PLI_HD (paged_plan.h), so the same text runs
// in the kernels and launchers of gemm_mxfp4.hip and in
// tests/host/mxfp4a_plan_check.cpp (tests/test_mxfp4a_plan.py).
//
// Layout: x8 [m, k] one e4m3fn code per byte (ldx8 in bytes), x_scale fp32 [m];
// w4 [n, k / 2] bytes of two e2m1 codes (element i in byte i / 2, even i in
// bits 3:0; ldw in bytes), w_exp [n, k / 32] E8M0 bytes (leading dimension
// lds); C [m, n] 16-bit, ldc in elements.
#pragma once

#include <cstddef>
#include <cstdint>

#include "fp8a_plan.h"

namespace pli {

// ------------------------------------------------------------------ routes --
enum Mxfp4aRoute {
    MXFP4A_EMPTY = 0,    // m == 0 or n == 0: nothing; k == 0: bias or 0 (generic kernel)
    MXFP4A_MX = 1,       // gemm_mxfp4_mx (v_mfma_scale_f32_32x32x64_f8f6f4, e2m1 x e4m3)
    MXFP4A_GENERIC = 2,  // gemm_mxfp4_generic
};

constexpr int kMxfp4aBlock = 32;    // elements per E8M0 scale: the instruction's block is the format's
constexpr int kMxfp4aKStep = 128;   // codes of k per stage = kFp8aKStep: four blocks, one dword of scale bytes
constexpr int kMxfp4aStages = 2;    // LDS stages: step s + 1 lands while step s is multiplied
constexpr int kMxfp4aMinM = 17;     // below: the W4A16 decode kernels' ground
constexpr int kMxfp4aWRowBytes = kMxfp4aKStep / 2;                        // one staged W row: 64 bytes = 4 chunks
constexpr int kMxfp4aWChunks = kMxfp4aWRowBytes / kFp8aChunk;             // 4
constexpr int kMxfp4aWImgBytes = kFp8aTN * kMxfp4aWRowBytes;              // 8 KiB
constexpr int kMxfp4aStageBytes = kMxfp4aWImgBytes + kFp8aImgBytes;       // W image, then X image: 24 KiB
constexpr int kMxfp4aLdsBytes = kMxfp4aStages * kMxfp4aStageBytes;        // 48 KiB
constexpr int kMxfp4aWPieces = kMxfp4aWImgBytes / 1024;                   // 1 KiB wave-instructions: 8
constexpr int kMxfp4aWPiecesPerWave = kMxfp4aWPieces / 4;                 // 2
constexpr int kMxfp4aWPieceRows = 1024 / kMxfp4aWRowBytes;                // 16 rows per piece

static_assert(kMxfp4aKStep == kFp8aKStep, "the X image is gemm_fp8_mx's");

struct Mxfp4aCall {
    int m, n, k;
    int64_t ldx8, ldw, lds, ldc;
    uintptr_t x8, w4, w_exp, c;
};

PLI_HD inline bool mxfp4a_shape_ok(int k) { return k % kMxfp4aBlock == 0; }

PLI_HD inline bool mxfp4a_mx_ok(const Mxfp4aCall& a) {
    return a.m >= kMxfp4aMinM && a.k % kMxfp4aKStep == 0 && ((a.x8 | a.w4) & 15) == 0 && a.ldx8 % 16 == 0 &&
           a.ldw % 16 == 0 && (a.w_exp & 3) == 0 && a.lds % 4 == 0 && a.n % kFp8aStoreN == 0 &&
           a.ldc % kFp8aStoreN == 0 && (a.c & 7) == 0;
}

// The route of a call (k % 32 == 0 was checked), from host arguments only (a
// captured call replays).
PLI_HD inline int mxfp4a_route(const Mxfp4aCall& a) {
    if (a.m <= 0 || a.n <= 0 || a.k <= 0) return MXFP4A_EMPTY;
    if (mxfp4a_mx_ok(a)) return MXFP4A_MX;
    return MXFP4A_GENERIC;
}

// ----------------------------------------------------------- gemm_mxfp4_mx --
// W staging.  The image is [128 rows][4 chunks of 16 bytes]; piece p (one
// LDS-DMA wave-instruction, 1 KiB, lane-linear: lane l lands at 1024 p + 16 l)
// is rows 16 p .. 16 p + 15, wave w issues pieces 2 w, 2 w + 1.  Lane l lands
// in row 16 p + (l >> 2), slot l & 3, and fetches the chunk that belongs in
// that slot: the XOR swizzle sits on the source address.
//
// The swizzle.  A ds_read_b128 is served 16 lanes at a time, and those 16
// lanes are conflict-free when their 16-byte slots differ modulo the 256-byte
// LDS line (64 banks x 4 bytes).  The 16 lanes of a phase of a fragment read
// hold 16 consecutive rows r0 .. r0 + 15 (r0 % 16 == 0) of one chunk c.  Slot
// of (row, c) modulo 16 = 4 (row & 3) + (c ^ swz(row)): the term 4 (row & 3)
// separates four classes of rows, and inside a class (row >> 2) & 3 takes each
// of its four values once, so swz(row) = (row >> 2) & 3 makes c ^ swz(row) a
// different one of the four slots for each: 16 distinct slots.  Unswizzled the
// four rows of a class share a slot (4 bank groups, 4 deep).
PLI_HD inline int mxfp4a_swz(int row) { return (row >> 2) & 3; }
PLI_HD inline int mxfp4a_stage_piece(int wave, int i) { return kMxfp4aWPiecesPerWave * wave + i; }
PLI_HD inline int mxfp4a_stage_row(int piece, int lane) { return kMxfp4aWPieceRows * piece + (lane >> 2); }
PLI_HD inline int mxfp4a_stage_chunk(int piece, int lane) {
    return (lane & 3) ^ mxfp4a_swz(mxfp4a_stage_row(piece, lane));
}
PLI_HD inline int mxfp4a_stage_lds(int piece, int lane) { return 1024 * piece + kFp8aChunk * lane; }
// rows past the operand re-read its last row (their outputs are never stored)
PLI_HD inline int mxfp4a_w_row(int n0, int row, int n) { return n0 + row < n ? n0 + row : n - 1; }
// byte offset in w4 of the chunk a lane fetches at K-step `step`
PLI_HD inline int64_t mxfp4a_w_off(int n0, int row, int n, int64_t ldw, int step, int chunk) {
    return (int64_t)mxfp4a_w_row(n0, row, n) * ldw + (int64_t)step * kMxfp4aWRowBytes + chunk * kFp8aChunk;
}

// W fragments.  The e2m1 operand of tile t, k-half h (64 codes) of a lane is
// one 16-byte chunk: row fp8a_frag_row(wn, t, lane), k = 64 h + 32 (lane >> 5)
// + j, j = 0 .. 31, element j in nibble j & 1 of byte j >> 1.
PLI_HD inline int mxfp4a_frag_chunk(int h, int lane) { return 2 * h + (lane >> 5); }
PLI_HD inline int mxfp4a_frag_lds(int row, int chunk) {
    return row * kMxfp4aWRowBytes + ((chunk ^ mxfp4a_swz(row)) * kFp8aChunk);
}
// k (inside the K-step) of element j of that operand
PLI_HD inline int mxfp4a_frag_k(int h, int lane, int j) { return 64 * h + 32 * (lane >> 5) + j; }

// Scale bytes.  Per K-step and tile t a lane loads the dword of the four scale
// bytes of its row (row fp8a_frag_row(wn, t, lane), clamped like the codes),
// blocks 4 step .. 4 step + 3.  The instruction takes byte 0 of the scale
// register of lane l (op_sel 0) as the scale of row l & 31, the 32 k of lane
// half l >> 5, so the operand of k-half h is the dword shifted right by
// mxfp4a_scale_shift(h, lane): its byte 0 is block 2 h + (lane >> 5).
PLI_HD inline int64_t mxfp4a_scale_off(int n0, int row, int n, int64_t lds, int step) {
    return (int64_t)mxfp4a_w_row(n0, row, n) * lds + (int64_t)step * (kMxfp4aKStep / kMxfp4aBlock);
}
PLI_HD inline int mxfp4a_scale_shift(int h, int lane) { return 8 * (2 * h + (lane >> 5)); }

// X fragments.  The image, its pieces and its swizzle are gemm_fp8_mx's; the
// order of the fragment halves is not.  Settled on the device: of the 64 k of
// one instruction a 4-register (e2m1) operand holds k = 32 (lane >> 5) + j in
// element j, but an 8-register (e4m3) operand holds k = 32 (b >> 4) +
// 16 (lane >> 5) + (b & 15) in byte b.  Between two 8-register operands, as in
// gemm_fp8_mx, the order cancels; here it does not, so 16-byte half h of the X
// operand of k-half s is chunk 4 s + 2 h + (lane >> 5) of the row.
PLI_HD inline int mxfp4a_xfrag_chunk(int s, int lane, int h) { return 4 * s + 2 * h + (lane >> 5); }
// k (inside the K-step) of byte b of that operand
PLI_HD inline int mxfp4a_xfrag_k(int s, int lane, int b) { return 64 * s + 32 * (b >> 4) + 16 * (lane >> 5) + (b & 15); }

}  // namespace pli
