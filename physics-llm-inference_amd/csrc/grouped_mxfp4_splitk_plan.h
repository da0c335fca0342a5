// Split-K grouped W4A8 GEMM for decode (pli_gemm_grouped_mxfp4_ws, at most 32
// sorted rows) as pure C++17 (no HIP headers): the route and split rule, the K
// chunks and their passes over the LDS stage, which X piece every lane stages
// and where it lands, where every accumulator register is stored in the
// workspace, and the reduce kernel's item map.  The e2m1 operand chunk, the
// scale dword and its shift, the X image and its swizzle and the accumulator
// map are mxfp4a_plan.h's, fp8a_plan.h's and mx_splitk_plan.h's, unchanged: a
// wave loads its weight rows exactly as gemm_mx_splitk<MXSK_E2M1> and
// gemm_grouped_mxfp4 do.  The functions carry PLI_HD (paged_plan.h), so the
// same text runs in the kernels and launcher of gemm_grouped_mxfp4_splitk.hip
// and in tests/host/grouped_mxfp4_splitk_plan_check.cpp
// (tests/test_grouped_mxfp4_splitk_plan.py).
//
// Layout: the operands of pli_gemm_grouped_mxfp4 (grouped_mxfp4_plan.h);
// workspace fp32 [S][rows_bound][n], or [S][rows_bound][2][n] for SwiGLU (gate,
// then up), row-major.
#pragma once

#include <cstddef>
#include <cstdint>

#include "grouped_mxfp4_plan.h"

namespace pli {

// -------------------------------------------------------------- split rule --
// The host knows rows_bound and the number of experts, not how many experts
// have rows: at one token two of them do, and only their workgroups work.  So
// the rule aims at kGsk4TargetWgs workgroups PER EXPERT (x = tiles of 128
// weight rows, y = chunks): two active experts then put four workgroups on
// every CU of the part it was tuned on, each with all its W loads in flight.
// kGsk4MaxSplits: the most partials the reduce sums.  kGsk4MinSteps: the
// fewest K-steps of 128 codes a chunk of the rule keeps, so the fill, the
// barrier and the partial's store are paid over at least that many steps.
// Values 512 / 16 / 4, kept by the sweep of forced S in DESIGN.md §3.7c
// (MoEConfig defaults; W2: k 14336, 32 tiles, S = 16, 7 steps per chunk; W1/W3:
// k 4096, 112 tiles, S = 5, 7 steps).  The legs that decided: W2 at one token
// needs S >= 12 (25 us against 38 us at S = 2), and W1/W3 at one token must not
// get S = 16 (56 us, slower than the plain call's 50; 46 - 48 us at S = 2 .. 8).
// Not settled: at 16 tokens, all experts active, S = 2 ran 6 % faster than the
// rule on both GEMMs; the rule does not count the experts that can have rows.
constexpr int kGsk4TargetWgs = 512;
constexpr int kGsk4MaxSplits = 16;
constexpr int kGsk4MinSteps = 4;
constexpr int kGsk4MaxRows = kMxskBlockM;  // one m block: every expert's rows fit it, so there is no slot scan
constexpr int kGsk4MaxExperts = 65535;     // experts sit in blockIdx.z
// The LDS stage: one fp8a_plan.h image of 32 rows (4 KiB, pieces 0 .. 3) per
// K-step, kGsk4StageSteps of them.  A chunk of more steps runs in passes of at
// most that many (fill -> barrier -> multiply, a barrier between two passes).
// Under the rule a chunk has ceil(ks / S) steps with S <= 16, so passes repeat
// for k > 16384, for k > 1024 * S where few splits reach the target (n of more
// than 4096 weight rows: S <= 4), and for a forced `splits` below ks / 8.
constexpr int kGsk4StageSteps = 8;
constexpr int kGsk4ImgBytes = kMxskBlockBytes;                     // 4 KiB
constexpr int kGsk4LdsBytes = kGsk4StageSteps * kGsk4ImgBytes;     // 32 KiB
// vector-memory operations of one wave per K-step and weight matrix: two operand chunks and the scale dword.
// The wait for X in gsk4_pass counts on it: between a pass's LDS-DMA pieces and its barrier a wave issues exactly
// kGsk4WLoads * NW * LEN vector-memory operations.  A load or store added there (a hoisted partial store, a
// prefetch) without raising the count makes that wait too weak, and nothing reports it: X would be read early.
constexpr int kGsk4WLoads = 3;

struct Gsk4Plan {
    int splits;  // S: >= 2 on the split route, otherwise the call is the plain entry point
    int per;     // K-steps per chunk: ceil(ks / S)
};

// S of a shape (0 where the shape itself rules the split route out).  splits ==
// 0: the smallest S with tiles * S >= kGsk4TargetWgs, at most kGsk4MaxSplits
// and ks / kGsk4MinSteps; splits >= 1: forced, at most ks and kGsk4MaxSplits.
// Either way S is then lowered to ceil(ks / ceil(ks / S)): no chunk is empty.
PLI_HD inline int gsk4_splits(int experts, int rows_bound, int n, int k, int splits) {
    if (experts < 1 || experts > kGsk4MaxExperts || rows_bound < 1 || rows_bound > kGsk4MaxRows || n <= 0 ||
        n % 16 != 0 || k <= 0 || k % kMxfp4aKStep != 0 || splits < 0)
        return 0;
    const int ks = k / kMxfp4aKStep, tiles = fp8a_tiles(n, kGmx4TN);
    int s;
    if (splits == 0) {
        s = (kGsk4TargetWgs + tiles - 1) / tiles;
        if (s > ks / kGsk4MinSteps) s = ks / kGsk4MinSteps;
    } else {
        s = splits < ks ? splits : ks;
    }
    if (s > kGsk4MaxSplits) s = kGsk4MaxSplits;
    if (s < 1) s = 1;
    const int per = (ks + s - 1) / s;
    return (ks + per - 1) / per;
}

PLI_HD inline size_t gsk4_ws_bytes(int rows_bound, int n, int swiglu, int s) {
    return (size_t)s * (size_t)rows_bound * (size_t)n * (size_t)(swiglu ? 2 : 1) * sizeof(float);
}

// What pli_gemm_grouped_mxfp4_workspace_size reports: the bytes the split route
// uses, 0 where it does not apply.
PLI_HD inline size_t gsk4_workspace_size(int experts, int rows_bound, int n, int k, int swiglu, int splits) {
    const int s = gsk4_splits(experts, rows_bound, n, k, splits);
    return s >= 2 ? gsk4_ws_bytes(rows_bound, n, swiglu, s) : 0;
}

// The plan of a call, from host arguments only (a captured call replays).
// base_mx: gmx4_route == GMX4_MX of the same call.
PLI_HD inline Gsk4Plan gsk4_plan(bool base_mx, int experts, int rows_bound, int n, int k, int swiglu, int splits,
                                 uintptr_t ws, size_t ws_bytes) {
    const Gsk4Plan plain{1, 0};
    if (!base_mx || ws == 0 || (ws & 15) != 0) return plain;
    const int s = gsk4_splits(experts, rows_bound, n, k, splits);
    if (s < 2 || ws_bytes < gsk4_ws_bytes(rows_bound, n, swiglu, s)) return plain;
    const int ks = k / kMxfp4aKStep;
    return Gsk4Plan{s, (ks + s - 1) / s};
}

// K-steps [begin, end) of chunk c: mxsk_chunk_begin / mxsk_chunk_end.  Pass p
// of a chunk of `len` steps covers its local steps [8 p, 8 p + gsk4_pass_len).
PLI_HD inline int gsk4_passes(int len) { return (len + kGsk4StageSteps - 1) / kGsk4StageSteps; }
PLI_HD inline int gsk4_pass_len(int len, int p) {
    return len - p * kGsk4StageSteps < kGsk4StageSteps ? len - p * kGsk4StageSteps : kGsk4StageSteps;
}

// ----------------------------------------------- gemm_grouped_mxfp4_splitk --
// Grid: x = tile of 128 weight rows, y = chunk, z = expert; one workgroup of 4
// waves.  The expert's sorted rows [offsets[e], offsets[e + 1]) are image rows
// 0 .. count - 1 of every stage; an expert without rows leaves first.
//
// X staging.  Image i of the stage holds local step i of the pass; wave w
// issues piece w (image rows 8 w .. 8 w + 7) of every image, one 16-byte
// LDS-DMA wave-instruction each, with fp8a_plan.h's lane map and swizzle.  An
// image row stands for sorted row gmx4_sorted_row(rbeg, row, rend) (clamped to
// the expert's last row; the clamped rows are multiplied and never stored) and
// its bytes are gmx4_x_off(gather[sorted row], ldx8, step, chunk).
PLI_HD inline int gsk4_stage_lds(int image, int wave, int lane) {
    return image * kGsk4ImgBytes + fp8a_stage_lds(wave, lane);
}
// where a fragment read of image `image` finds (row, chunk)
PLI_HD inline int gsk4_frag_lds(int image, int row, int chunk) {
    return image * kGsk4ImgBytes + fp8a_frag_lds(row, chunk);
}

// Partials.  Accumulator register r of matrix m (0: gate or the only one, 1:
// up) is sorted row rbeg + mxsk_acc_m(0, lane), column n0 + mxsk_acc_n(wave,
// lane, r); element index in the workspace, nw = 1 + swiglu matrices:
PLI_HD inline int64_t gsk4_ws_index(int c, int row, int m, int col, int rows_bound, int n, int nw) {
    return (((int64_t)c * rows_bound + row) * nw + m) * n + col;
}

// ---------------------------------------- gemm_grouped_mxfp4_splitk_reduce --
// One thread per 4 consecutive n of one sorted row, 256 threads per workgroup:
// mxsk_reduce_items / mxsk_reduce_blocks over [rows_bound, n].  Rows at and
// past offsets[experts] belong to no expert and are left alone.
PLI_HD inline int gsk4_reduce_row(int64_t item, int n) { return (int)(item / (n / kFp8aStoreN)); }
PLI_HD inline int gsk4_reduce_col(int64_t item, int n) { return (int)(item % (n / kFp8aStoreN)) * kFp8aStoreN; }

}  // namespace pli
