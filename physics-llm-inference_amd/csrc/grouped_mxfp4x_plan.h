// Grouped W4A4 GEMM over MoE experts (pli_gemm_grouped_mxfp4_a4) as pure C++17
// (no HIP headers): the route rule, where the gathered MXFP4 activation rows'
// codes and scale dwords come from, and the stage layout of the plain (two
// images) and the SwiGLU (three images) instance.  The slot -> (expert, slab)
// scan and the sorted-row clamp are grouped_mxfp4_plan.h's, the operand image
// with its pieces, swizzle and accumulator map fp8a_plan.h's, the e2m1 operand
// chunk and the scale-dword maps mxfp4x_plan.h's, all unchanged.  The
// functions carry PLI_HD (paged_plan.h), so the same text runs in the kernels
// and launcher of gemm_grouped_mxfp4_a4.hip and in
// tests/host/grouped_mxfp4x_plan_check.cpp (tests/test_grouped_mxfp4x_plan.py).
//
// Layout: x4 [tokens, k / 2] e2m1 code pairs (ldx4 bytes), x_exp [tokens,
// k / 32] E8M0 bytes (ldxs), x_scale fp32 [tokens], as pli_quantize_rows_mxfp4
// writes them; the expert weights, offsets, gather and C as in
// grouped_mxfp4_plan.h.
#pragma once

#include <cstddef>
#include <cstdint>

#include "grouped_mxfp4_plan.h"
#include "mxfp4x_plan.h"

namespace pli {

// ------------------------------------------------------------------ routes --
enum Gmx4xRoute {
    GMX4X_EMPTY = 0,    // rows_bound == 0 or n == 0: nothing
    GMX4X_MX = 1,       // gemm_grouped_mxfp4_a4<T, SW>
    GMX4X_GENERIC = 2,  // gemm_grouped_mxfp4_a4_generic
};

struct Gmx4xCall {
    int experts, rows_bound, n, k;
    int64_t ldx4, ldxs, ldw, lds, ldc;
    uintptr_t x4, x_exp, c;
};

// The MX route, from host arguments only (a captured call replays).  As in
// gmx4_mx_ok the table entries are device values: 16-byte (codes) and 4-byte
// (scale bytes) aligned by the call's contract.
PLI_HD inline bool gmx4x_mx_ok(const Gmx4xCall& a) {
    return a.k > 0 && a.k % kMxfp4xKStep == 0 && a.n % 16 == 0 && (a.x4 & 15) == 0 && a.ldx4 % 16 == 0 &&
           a.ldw % 16 == 0 && (a.x_exp & 3) == 0 && a.ldxs % 4 == 0 && a.lds % 4 == 0 && a.ldc % kFp8aStoreN == 0 &&
           (a.c & 7) == 0 && gmx4_slots(a.rows_bound, a.experts) <= kGmx4MaxSlots;
}
PLI_HD inline int gmx4x_route(const Gmx4xCall& a) {
    if (a.rows_bound <= 0 || a.n <= 0) return GMX4X_EMPTY;
    return gmx4x_mx_ok(a) ? GMX4X_MX : GMX4X_GENERIC;
}

// -------------------------------------------------- gemm_grouped_mxfp4_a4 --
// Grid: x = tile of 128 weight rows, y = slot (gmx4_slab).  Image row `row` of
// the X side stands for sorted row gmx4_sorted_row(rbeg, row, rend); its codes
// and its scale bytes are row `token` = gather[that row] of x4 / x_exp (gather
// NULL: the sorted row itself).  Per K-step of 256 codes a row is 128 bytes of
// codes (8 chunks of 16) and 8 scale bytes (two dwords).
PLI_HD inline int64_t gmx4x_x_off(int token, int64_t ldx4, int step, int chunk) {
    return (int64_t)token * ldx4 + (int64_t)step * kFp8aRowBytes + chunk * kFp8aChunk;
}
PLI_HD inline int64_t gmx4x_xscale_off(int token, int64_t ldxs, int step, int dword) {
    return (int64_t)token * ldxs + (int64_t)step * kMxfp4xStepScales + 4 * dword;
}

// Stage layout: the W images first (plain: W; SwiGLU: gate W, then up W), then
// the X image, 16 KiB each; two stages.
constexpr int kGmx4xLdsLimit = 160 * 1024;  // LDS of a gfx950 workgroup
PLI_HD constexpr int gmx4x_w_images(bool swiglu) { return swiglu ? 2 : 1; }
PLI_HD constexpr int gmx4x_w_img_off(int matrix) { return matrix * kFp8aImgBytes; }
PLI_HD constexpr int gmx4x_x_img_off(bool swiglu) { return gmx4x_w_images(swiglu) * kFp8aImgBytes; }
PLI_HD constexpr int gmx4x_stage_bytes(bool swiglu) { return (gmx4x_w_images(swiglu) + 1) * kFp8aImgBytes; }
PLI_HD constexpr int gmx4x_stage_off(bool swiglu, int step) { return step % kMxfp4xStages * gmx4x_stage_bytes(swiglu); }
PLI_HD constexpr int gmx4x_lds_bytes(bool swiglu) { return kMxfp4xStages * gmx4x_stage_bytes(swiglu); }
static_assert(gmx4x_lds_bytes(true) == 96 * 1024 && gmx4x_lds_bytes(true) <= kGmx4xLdsLimit, "three images, two stages");

}  // namespace pli
