// Grouped W4A8 GEMM over MoE experts (pli_gemm_grouped_mxfp4) as pure C++17
// (no HIP headers): the route rule, the slot -> (expert, slab) scan, which
// sorted row every lane of the X staging stands for and where its bytes come
// from, and where every accumulator register is stored.  The X image, its
// swizzle, the e2m1 operand and scale-byte maps and the accumulator map are
// fp8a_plan.h's, mxfp4a_plan.h's and mx_splitk_plan.h's, unchanged: a wave
// loads its weight rows exactly as gemm_mx_splitk<MXSK_E2M1> does.  The
// functions carry PLI_HD (paged_plan.h), so the same text runs in the kernels
// and launcher of gemm_grouped_mxfp4.hip and in
// tests/host/grouped_mxfp4_plan_check.cpp (tests/test_grouped_mxfp4_plan.py).
//
// Layout: x8 [tokens, k] e4m3fn codes (ldx8 bytes), x_scale fp32 [tokens];
// per expert w4 [n, k / 2] e2m1 code pairs (ldw bytes) and w_exp [n, k / 32]
// E8M0 bytes (lds), reached through device pointer tables; offsets [E + 1]
// and gather [rows] int32 on the device; C [rows_bound, n] 16-bit, ldc in
// elements, rows in expert-sorted order.
#pragma once

#include <cstddef>
#include <cstdint>

#include "mx_splitk_plan.h"

namespace pli {

// ------------------------------------------------------------------ routes --
enum Gmx4Route {
    GMX4_EMPTY = 0,    // rows_bound == 0 or n == 0: nothing
    GMX4_MX = 1,       // gemm_grouped_mxfp4<MC, SW>
    GMX4_GENERIC = 2,  // gemm_grouped_mxfp4_generic
};

constexpr int kGmx4SlabM = kFp8aTM;   // sorted rows of a slot: one workgroup's X rows
constexpr int kGmx4TN = kFp8aTN;      // weight rows (C columns) of a workgroup, every instance
constexpr int kGmx4MaxSlots = 65535;  // slots sit in blockIdx.y

struct Gmx4Call {
    int experts, rows_bound, n, k;
    int64_t ldx8, ldw, lds, ldc;
    uintptr_t x8, c;
};

// m blocks of 32 rows a workgroup multiplies: rows_bound bounds every expert's
// rows, so no slab holds more than min(rows_bound, 128) of them
PLI_HD inline int gmx4_mc(int rows_bound) { return mxsk_mc(rows_bound); }
// an upper bound of sum_e ceil(count_e / 128) for counts summing to at most rows_bound
PLI_HD inline int64_t gmx4_slots(int rows_bound, int experts) {
    return (int64_t)rows_bound / kGmx4SlabM + (rows_bound % kGmx4SlabM != 0) + experts;
}

// The MX route, from host arguments only (a captured call replays): the table
// entries are device values, so of the weights only their leading dimensions
// are seen here; the entries themselves are 16-byte (codes) and 4-byte (scale
// bytes) aligned by the call's contract.
PLI_HD inline bool gmx4_mx_ok(const Gmx4Call& a) {
    return a.k > 0 && a.k % kMxfp4aKStep == 0 && a.n % 16 == 0 && (a.x8 & 15) == 0 && a.ldx8 % 16 == 0 &&
           a.ldw % 16 == 0 && a.lds % 4 == 0 && a.ldc % kFp8aStoreN == 0 && (a.c & 7) == 0 &&
           gmx4_slots(a.rows_bound, a.experts) <= kGmx4MaxSlots;
}
PLI_HD inline int gmx4_route(const Gmx4Call& a) {
    if (a.rows_bound <= 0 || a.n <= 0) return GMX4_EMPTY;
    return gmx4_mx_ok(a) ? GMX4_MX : GMX4_GENERIC;
}
// workgroups of the generic kernel: one thread per element of [rows_bound, n]
PLI_HD inline int64_t gmx4_generic_blocks(int rows_bound, int n) { return ((int64_t)rows_bound * n + 255) / 256; }

// ------------------------------------------------------ gemm_grouped_mxfp4 --
// Grid: x = tile of 128 weight rows, y = slot.  Expert e's sorted rows
// [offsets[e], offsets[e + 1]) are cut into slabs of 128; the slots count the
// slabs of all experts in expert order.  A slot past the last slab has no
// expert (-1): its workgroup leaves before any barrier.
struct Gmx4Slab {
    int expert, rbeg, rend;  // sorted rows [rbeg, min(rbeg + 128, rend)), rend the expert's end
};
PLI_HD inline Gmx4Slab gmx4_slab(const int32_t* offsets, int experts, int slot) {
    int acc = 0;
    for (int e = 0; e < experts; ++e) {
        const int b0 = offsets[e], b1 = offsets[e + 1];
        const int nt = (b1 - b0 + kGmx4SlabM - 1) / kGmx4SlabM;
        if (slot < acc + nt) return Gmx4Slab{e, b0 + (slot - acc) * kGmx4SlabM, b1};
        acc += nt;
    }
    return Gmx4Slab{-1, 0, 0};
}

// X staging: mx_splitk_plan.h's pieces (wave w issues pieces w, w + 4, ..: MC
// each, piece p = image rows 8 p .. 8 p + 7) over the slab's rows.  Image row
// `row` stands for sorted row rbeg + row, clamped to the expert's last row
// (rows past the end are multiplied and never stored); its bytes are row
// gather[sorted row] of x8 (gather NULL: the sorted row itself).
PLI_HD inline int gmx4_sorted_row(int rbeg, int row, int rend) { return rbeg + row < rend ? rbeg + row : rend - 1; }
PLI_HD inline int64_t gmx4_x_off(int token, int64_t ldx8, int step, int chunk) {
    return (int64_t)token * ldx8 + (int64_t)step * kFp8aKStep + chunk * kFp8aChunk;
}

// C: accumulator register r of m block b is sorted row rbeg + mxsk_acc_m(b,
// lane), column n0 + mxsk_acc_n(wave, lane, r); in the SwiGLU instances the
// gate and the up accumulator of an element are register r of the same lane.
PLI_HD inline int64_t gmx4_c_index(int row, int col, int64_t ldc) { return (int64_t)row * ldc + col; }

// -------------------------------------------- gemm_grouped_mxfp4_generic --
// the expert of a sorted row, -1 past offsets[experts]
PLI_HD inline int gmx4_expert_of(const int32_t* offsets, int experts, int row) {
    for (int e = 0; e < experts; ++e)
        if (row < offsets[e + 1]) return row >= offsets[e] ? e : -1;
    return -1;
}

}  // namespace pli
