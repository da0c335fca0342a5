// fp8 activations (W8A8) as pure C++17 (no HIP headers): the route rule of
// pli_gemm_fp8, the tile map of gemm_fp8_mx (what every lane stages, where it
// lands in LDS, which bytes each scaled-MFMA operand slot reads, where every
// accumulator register is stored) and the element map of quant_rows_fp8.  The
// functions carry PLI_HD (paged_plan.h), so the same text runs in the kernels
// and launchers of gemm_fp8.hip and in tests/host/fp8a_plan_check.cpp
// (tests/test_fp8a_plan.py).
//
// Layout: X8 [m, k] and W8 [n, k] one e4m3fn code per byte, row-major, leading
// dimensions ldx8 / ldw in bytes; x_scale fp32 [m], w_scale fp32 [n];
// C [m, n] 16-bit, ldc in elements.
#pragma once

#include <cstddef>
#include <cstdint>

#include "paged_plan.h"

namespace pli {

// ------------------------------------------------------------------ routes --
enum Fp8aRoute {
    FP8A_EMPTY = 0,    // m == 0 or n == 0: nothing; k == 0: bias or 0 (generic kernel)
    FP8A_MX = 1,       // gemm_fp8_mx (v_mfma_scale_f32_32x32x64_f8f6f4)
    FP8A_GENERIC = 2,  // gemm_fp8_generic
};

constexpr int kFp8aTM = 128;     // X rows of a tile
constexpr int kFp8aTN = 128;     // W rows (C columns) of a tile
constexpr int kFp8aKStep = 128;  // codes of k per stage: two 32x32x64 MFMAs deep
constexpr int kFp8aStages = 2;   // LDS stages: step s + 1 lands while step s is multiplied
constexpr int kFp8aMinM = 17;    // below: the W8A16 decode kernels' ground (unmeasured threshold)
constexpr int kFp8aStoreN = 4;   // C columns per packed 8-byte store
constexpr int kFp8aChunk = 16;   // bytes per lane of one LDS-DMA
constexpr int kFp8aRowBytes = kFp8aKStep;                   // one staged row: 128 bytes = 8 chunks
constexpr int kFp8aImgBytes = kFp8aTM * kFp8aRowBytes;      // one operand image: 16 KiB
constexpr int kFp8aStageBytes = 2 * kFp8aImgBytes;          // W image, then X image
constexpr int kFp8aLdsBytes = kFp8aStages * kFp8aStageBytes;  // 64 KiB
constexpr int kFp8aPieces = kFp8aImgBytes / 1024;           // 1 KiB wave-instructions per image: 16
constexpr int kFp8aPiecesPerWave = kFp8aPieces / 4;         // 4 waves: 4 pieces of each operand

struct Fp8aCall {
    int m, n, k;
    int64_t ldx8, ldw, ldc;
    uintptr_t x8, w8, c;
};

PLI_HD inline bool fp8a_mx_ok(const Fp8aCall& a) {
    return a.m >= kFp8aMinM && a.k % kFp8aKStep == 0 && ((a.x8 | a.w8) & 15) == 0 && a.ldx8 % 16 == 0 &&
           a.ldw % 16 == 0 && a.n % kFp8aStoreN == 0 && a.ldc % kFp8aStoreN == 0 && (a.c & 7) == 0;
}

// The route of a call, from host arguments only (a captured call replays).
PLI_HD inline int fp8a_route(const Fp8aCall& a) {
    if (a.m <= 0 || a.n <= 0 || a.k <= 0) return FP8A_EMPTY;
    if (fp8a_mx_ok(a)) return FP8A_MX;
    return FP8A_GENERIC;
}

// ------------------------------------------------------------- gemm_fp8_mx --
// One workgroup of 4 waves per 128 x 128 tile of C.  Tile order: bands of
// kFp8aGroupM m-tiles, inside a band m fastest, then n -- neighbouring
// workgroups share a W tile, and the workgroups in flight together (a run of
// consecutive tiles per XCD) cover a block of about 8 x 8 tiles rather than
// one column of all m, so they re-read 8 X tiles and 8 W tiles, not every X
// tile, per 64.  Up to kFp8aGroupM m-tiles this is plain m-fastest order.
// The kernel computes C^T: W rows are the MFMA's A operand, X rows its B
// operand, so a lane's accumulator registers hold consecutive n of one m.
constexpr int kFp8aGroupM = 8;
PLI_HD inline int fp8a_tiles(int dim, int tile) { return dim / tile + (dim % tile != 0); }
PLI_HD inline int fp8a_tile_band_rows(int t, int tiles_m, int tiles_n) {
    const int first = t / (kFp8aGroupM * tiles_n) * kFp8aGroupM;
    return tiles_m - first < kFp8aGroupM ? tiles_m - first : kFp8aGroupM;
}
PLI_HD inline int fp8a_tile_m(int t, int tiles_m, int tiles_n) {
    const int band = t / (kFp8aGroupM * tiles_n);
    return band * kFp8aGroupM + (t - band * kFp8aGroupM * tiles_n) % fp8a_tile_band_rows(t, tiles_m, tiles_n);
}
PLI_HD inline int fp8a_tile_n(int t, int tiles_m, int tiles_n) {
    const int band = t / (kFp8aGroupM * tiles_n);
    return (t - band * kFp8aGroupM * tiles_n) / fp8a_tile_band_rows(t, tiles_m, tiles_n);
}

// Staging.  An image is [128 rows][8 chunks of 16 bytes]; piece p (one LDS-DMA
// wave-instruction, 1 KiB, lane-linear: lane l lands at 1024 p + 16 l) is rows
// 8 p .. 8 p + 7, wave w issues pieces 4 w .. 4 w + 3 of both images.  Lane l
// lands in row 8 p + (l >> 3), slot l & 7, and fetches the chunk that belongs
// in that slot: the XOR swizzle sits on the source address.
PLI_HD inline int fp8a_swz(int row) { return (row >> 1) & 7; }
PLI_HD inline int fp8a_stage_piece(int wave, int i) { return kFp8aPiecesPerWave * wave + i; }
PLI_HD inline int fp8a_stage_row(int piece, int lane) { return 8 * piece + (lane >> 3); }
PLI_HD inline int fp8a_stage_chunk(int piece, int lane) { return (lane & 7) ^ fp8a_swz(fp8a_stage_row(piece, lane)); }
PLI_HD inline int fp8a_stage_lds(int piece, int lane) { return 1024 * piece + kFp8aChunk * lane; }
// byte offset in the operand of the chunk a lane fetches at K-step s: rows past
// the operand re-read its last row (their outputs are never stored)
PLI_HD inline int64_t fp8a_src_off(int row0, int row, int rows, int64_t ld, int step, int chunk) {
    const int r = row0 + row < rows ? row0 + row : rows - 1;
    return (int64_t)r * ld + (int64_t)step * kFp8aKStep + chunk * kFp8aChunk;
}

// Fragments.  Wave w owns the 64 x 64 block (wn = w & 1, wm = w >> 1) as 2 x 2
// MFMA tiles of 32 x 32.  The operand of tile t, k-half s (64 codes) of a lane
// is 32 bytes: row 64 wq + 32 t + (lane & 31), k = 64 s + 32 (lane >> 5) + j,
// j = 0 .. 31, read as two 16-byte halves h = 0, 1.
PLI_HD inline int fp8a_frag_row(int wq, int t, int lane) { return 64 * wq + 32 * t + (lane & 31); }
PLI_HD inline int fp8a_frag_chunk(int s, int lane, int h) { return 4 * s + 2 * (lane >> 5) + h; }
PLI_HD inline int fp8a_frag_lds(int row, int chunk) {
    return row * kFp8aRowBytes + ((chunk ^ fp8a_swz(row)) * kFp8aChunk);
}
// k (inside the K-step) of byte j of that operand
PLI_HD inline int fp8a_frag_k(int s, int lane, int j) { return 64 * s + 32 * (lane >> 5) + j; }

// Accumulator register r (0 .. 15) of MFMA tile (nt, mt): C^T row = n, column = m
PLI_HD inline int fp8a_acc_n(int wn, int nt, int lane, int r) {
    return 64 * wn + 32 * nt + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
}
PLI_HD inline int fp8a_acc_m(int wm, int mt, int lane) { return 64 * wm + 32 * mt + (lane & 31); }

// ---------------------------------------------------------- quant_rows_fp8 --
// One workgroup of 256 threads per row.  Vector class (k, ldx multiples of 8,
// ldx8 a multiple of 8, x 16-byte and x8 8-byte aligned): thread t takes the
// 8-element chunks t, t + 256, ...; the first kFp8aQuantHeld of them stay in
// registers between the absmax and the encode, so a row of up to
// kFp8aQuantRegK elements is read once; longer rows re-read the rest.
// Everything else: one element per thread and trip, read twice.
constexpr int kFp8aQuantThreads = 256;
constexpr int kFp8aQuantHeld = 4;
constexpr int kFp8aQuantRegK = 8 * kFp8aQuantThreads * kFp8aQuantHeld;  // 8192
PLI_HD inline bool fp8a_quant_vec(int k, int64_t ldx, int64_t ldx8, uintptr_t x, uintptr_t x8) {
    return k % 8 == 0 && ldx % 8 == 0 && ldx8 % 8 == 0 && (x & 15) == 0 && (x8 & 7) == 0;
}
// chunk (vector class) or element (scalar) index of thread t at trip u
PLI_HD inline int fp8a_quant_item(int t, int u) { return t + kFp8aQuantThreads * u; }
PLI_HD inline int fp8a_quant_trips(int items) { return (items + kFp8aQuantThreads - 1) / kFp8aQuantThreads; }

}  // namespace pli
