// Split-K block-scaled GEMM for few rows (pli_gemm_fp8_ws / pli_gemm_mxfp4_ws)
// as pure C++17 (no HIP headers): the route and split rule, the K chunks, and
// the index arithmetic of gemm_mx_splitk -- which X chunk every lane stages and
// where it lands, which bytes of W and w_exp every lane loads straight into its
// operand registers, which k each of them holds, and where every accumulator
// register is stored in the workspace.  The X image, its swizzle and the k maps
// of the two operand widths are fp8a_plan.h's and mxfp4a_plan.h's, unchanged.
// The functions carry PLI_HD (paged_plan.h), so the same text runs in the
// kernels and launchers of gemm_mx_splitk.hip and in
// tests/host/mx_splitk_plan_check.cpp (tests/test_mx_splitk_plan.py).
//
// Layout: the operands of pli_gemm_fp8 / pli_gemm_mxfp4; workspace fp32
// [S][m][n], row-major, leading dimension n.
#pragma once

#include <cstddef>
#include <cstdint>

#include "mxfp4a_plan.h"

namespace pli {

// -------------------------------------------------------------- split rule --
// The rule constants.  kMxskTargetWgs: the workgroups a call should reach
// (one per CU of the part it was tuned on; a constant, not a device query, so
// the plan replays on the host).  kMxskMaxTiles: with more tiles than this the
// plain call already covers most of the device and two chunks only add the
// reduce (measured: 224 tiles, S = 2 ran at 0.88x / 0.98x of the plain call).
// kMxskMaxSplits: the most partials the reduce kernel sums.  kMxskMinSteps: the fewest K-steps of 128 codes a chunk of the
// rule keeps, so the prologue (two stages in flight before the first MFMA) is
// paid over at least that many steps.
constexpr int kMxskTargetWgs = 256;
constexpr int kMxskMaxTiles = 128;
constexpr int kMxskMaxSplits = 16;
constexpr int kMxskMinSteps = 4;
constexpr int kMxskMinM = 17;    // = kFp8aMinM: below, the *_mx routes do not apply at all
constexpr int kMxskMaxM = 256;   // above: the 128 x 128 tile kernels fill the device by themselves
constexpr int kMxskStages = 3;   // X stages in LDS: steps s + 1 and s + 2 land while step s is multiplied
constexpr int kMxskBlockM = 32;  // X rows of one m block (one MFMA tile)
constexpr int kMxskMaxMC = 4;    // m blocks of a workgroup: 128 X rows
constexpr int kMxskBlockBytes = kMxskBlockM * kFp8aRowBytes;  // 4 KiB of the X image per m block and stage
constexpr int kMxskWaveN = 32;   // W rows of a wave: four waves own the 128 of the tile

static_assert(kMxskMinM == kFp8aMinM && kMxskMinM == kMxfp4aMinM, "the few-row range starts where the mx routes do");
static_assert(kMxskMaxMC * kMxskBlockM == kFp8aTM && 4 * kMxskWaveN == kFp8aTN, "the tile is gemm_fp8_mx's");

enum MxskFormat { MXSK_E4M3 = 0, MXSK_E2M1 = 1 };

struct MxskPlan {
    int splits;   // S: >= 2 on the split route, otherwise the call is the plain entry point
    int per;      // K-steps per chunk: ceil(ks / S)
    int mc;       // m blocks of a workgroup
    int tiles_m, tiles_n;
};

PLI_HD inline int mxsk_mc(int m) { return ((m < kFp8aTM ? m : kFp8aTM) + kMxskBlockM - 1) / kMxskBlockM; }

// S of a shape (0 where the shape itself rules the split route out).  splits ==
// 0: the smallest S with tiles * S >= kMxskTargetWgs (1 above kMxskMaxTiles
// tiles), at most kMxskMaxSplits and ks / kMxskMinSteps; splits >= 1: forced,
// at most ks and kMxskMaxSplits.  Either way S is then lowered to ceil(ks / ceil(ks / S)): no chunk is empty.
PLI_HD inline int mxsk_splits(int m, int n, int k, int splits) {
    if (m < kMxskMinM || m > kMxskMaxM || n <= 0 || n % kFp8aStoreN != 0 || k <= 0 || k % kFp8aKStep != 0 ||
        splits < 0)
        return 0;
    const int ks = k / kFp8aKStep;
    int s;
    if (splits == 0) {
        const int64_t tiles = (int64_t)fp8a_tiles(n, kFp8aTN) * fp8a_tiles(m, kFp8aTM);
        s = tiles > kMxskMaxTiles ? 1 : (int)((kMxskTargetWgs + tiles - 1) / tiles);
        if (s > ks / kMxskMinSteps) s = ks / kMxskMinSteps;
    } else {
        s = splits < ks ? splits : ks;
    }
    if (s > kMxskMaxSplits) s = kMxskMaxSplits;
    if (s < 1) s = 1;
    const int per = (ks + s - 1) / s;
    return (ks + per - 1) / per;
}

PLI_HD inline size_t mxsk_ws_bytes(int m, int n, int s) { return (size_t)s * (size_t)m * (size_t)n * sizeof(float); }

// What pli_gemm_*_workspace_size reports: the bytes the split route uses, 0
// where it does not apply.
PLI_HD inline size_t mxsk_workspace_size(int m, int n, int k, int splits) {
    const int s = mxsk_splits(m, n, k, splits);
    return s >= 2 ? mxsk_ws_bytes(m, n, s) : 0;
}

// The plan of a call, from host arguments only (a captured call replays).
// base_mx: fp8a_mx_ok / mxfp4a_route == MXFP4A_MX of the same call.
PLI_HD inline MxskPlan mxsk_plan(bool base_mx, int m, int n, int k, int splits, uintptr_t ws, size_t ws_bytes) {
    MxskPlan p{1, 0, 0, 0, 0};
    if (!base_mx || ws == 0 || (ws & 15) != 0) return p;
    const int s = mxsk_splits(m, n, k, splits);
    if (s < 2 || ws_bytes < mxsk_ws_bytes(m, n, s)) return p;
    const int ks = k / kFp8aKStep;
    return MxskPlan{s, (ks + s - 1) / s, mxsk_mc(m), fp8a_tiles(m, kFp8aTM), fp8a_tiles(n, kFp8aTN)};
}

// K-steps [begin, end) of chunk c
PLI_HD inline int mxsk_chunk_begin(int c, int per) { return c * per; }
PLI_HD inline int mxsk_chunk_end(int c, int per, int ks) { return (c + 1) * per < ks ? (c + 1) * per : ks; }

// ---------------------------------------------------------- gemm_mx_splitk --
// Grid: x = n tile of 128 W rows, y = chunk, z = m tile of 128 X rows; one
// workgroup of 4 waves, MC = mxsk_mc(m) m blocks of 32 X rows.
//
// X staging.  The image of a stage is the first 32 MC rows of gemm_fp8_mx's:
// [rows][8 chunks of 16 bytes], piece p (one LDS-DMA wave-instruction, 1 KiB)
// is rows 8 p .. 8 p + 7 with fp8a_plan.h's lane map and swizzle; the 4 MC
// pieces go round the waves, wave w issues pieces w, w + 4, ..: MC each.
PLI_HD inline int mxsk_x_piece(int wave, int i) { return 4 * i + wave; }

// X fragments.  m block b, k-half kh, 16-byte half h of a lane's 32-byte e4m3
// operand: row 32 b + (lane & 31); against an 8-register e4m3 W operand the
// chunk order of gemm_fp8_mx (W is loaded in the same order, below), against a
// 4-register e2m1 operand the halves crosswise (mxfp4a_plan.h).
PLI_HD inline int mxsk_x_row(int b, int lane) { return kMxskBlockM * b + (lane & 31); }
PLI_HD inline int mxsk_x_chunk(int fmt, int kh, int lane, int h) {
    return fmt == MXSK_E2M1 ? mxfp4a_xfrag_chunk(kh, lane, h) : fp8a_frag_chunk(kh, lane, h);
}

// W, straight from global memory into the operand registers.  Wave w owns W
// rows 32 w .. 32 w + 31 of the tile, lane l row 32 w + (l & 31), clamped to
// the last row of the operand.  Per K-step and k-half kh the lane loads
//   e4m3: the 32 bytes at k = 64 kh + 32 (l >> 5), as two 16-byte halves h --
//         byte b of the operand is the k fp8a_frag_k gives the X byte it meets;
//   e2m1: the 16-byte chunk 2 kh + (l >> 5) of the 64-byte row, which is the
//         operand as stored; and once per K-step the dword of its four scale
//         bytes (mxfp4a_scale_off / mxfp4a_scale_shift).
PLI_HD inline int mxsk_w_row(int wave, int lane) { return kMxskWaveN * wave + (lane & 31); }
PLI_HD inline int64_t mxsk_w_off(int fmt, int n0, int row, int n, int64_t ldw, int step, int kh, int lane, int h) {
    if (fmt == MXSK_E2M1) return mxfp4a_w_off(n0, row, n, ldw, step, mxfp4a_frag_chunk(kh, lane));
    return fp8a_src_off(n0, row, n, ldw, step, fp8a_frag_chunk(kh, lane, h));
}

// Accumulator register r (0 .. 15) of m block b: C^T row = n, column = m
PLI_HD inline int mxsk_acc_n(int wave, int lane, int r) {
    return kMxskWaveN * wave + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
}
PLI_HD inline int mxsk_acc_m(int b, int lane) { return kMxskBlockM * b + (lane & 31); }
// element index of (chunk, row, column) in the workspace
PLI_HD inline int64_t mxsk_ws_index(int c, int row, int col, int m, int n) {
    return ((int64_t)c * m + row) * n + col;
}

// --------------------------------------------------- gemm_mx_splitk_reduce --
// One thread per 4 consecutive n of one m, 256 threads per workgroup.
constexpr int kMxskReduceThreads = 256;
PLI_HD inline int64_t mxsk_reduce_items(int m, int n) { return (int64_t)m * (n / kFp8aStoreN); }
PLI_HD inline int64_t mxsk_reduce_blocks(int m, int n) {
    return (mxsk_reduce_items(m, n) + kMxskReduceThreads - 1) / kMxskReduceThreads;
}

}  // namespace pli
