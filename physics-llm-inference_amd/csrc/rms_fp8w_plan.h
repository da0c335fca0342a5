// RMSNorm fused into the fp8-weight decode projections (pli_rms_gemm_nt_fp8w,
// csrc/decode_fused_fp8w.hip) as pure C++17 (no HIP headers): the grid, the
// map global output row -> (group, row in group), the load clamps and the
// offset of an X chunk in the LDS image of the normalised rows.  The dot phase
// is linear_fp8w_vec's, so the (ROWS, CPL) choice, the wave -> first row map
// and the lane -> chunk map are fp8w_plan.h's fp8w_vec_* functions, called
// here and not restated.  The functions carry PLI_HD (paged_plan.h): the same
// text runs in the kernel, in its launcher and in
// tests/host/rms_fp8w_plan_check.cpp (tests/test_rms_fp8w_plan.py).
//
// Layout: up to 3 groups (q / k / v) of n_g output rows each, group g with its
// own codes w8_g [n_g, k] (leading dimension ldw_g bytes), scales and output.
// The groups' rows are numbered one after the other, 0 .. sum n_g - 1, and a
// wave owns ROWS consecutive numbers whatever group each falls in.  The m
// normalised rows y [m, k] of T sit in LDS back to back (row stride k).
#pragma once

#include <cstddef>
#include <cstdint>

#include "fp8w_plan.h"

namespace pli {

constexpr int kRmsFp8wMaxGroups = 3;
constexpr int kRmsFp8wMaxM = 4;      // rows of a (<= NB of the kernel)
constexpr int kRmsFp8wMaxK = 8192;   // m * k * 2 <= 65536 bytes of LDS
constexpr int kRmsFp8wNormChunk = 8; // elements per 16-byte chunk of a 16-bit row (rmsnorm_vec's unit)

// (group, row in group) of a global output row; group == ngroups past the last row
struct RmsFp8wRow {
    int group, row;
};

PLI_HD inline int rms_fp8w_total(const int* n, int ngroups) {
    int t = 0;
    for (int g = 0; g < ngroups; ++g) t += n[g];
    return t;
}
// workgroups of kFp8wVecWaves waves x `rows` output rows
PLI_HD inline int rms_fp8w_grid(int ntot, int rows) { return fp8w_vec_grid(ntot, rows); }
PLI_HD inline RmsFp8wRow rms_fp8w_resolve(int64_t grow, const int* n, int ngroups) {
    int g = 0;
    while (g < ngroups && grow >= n[g]) grow -= n[g++];
    return RmsFp8wRow{g, (int)grow};
}
// the row a wave loads for global row `grow`: rows past the end are loaded from the last row of the last group
// (and never stored)
PLI_HD inline RmsFp8wRow rms_fp8w_load_row(int64_t grow, const int* n, int ngroups) {
    const RmsFp8wRow r = rms_fp8w_resolve(grow, n, ngroups);
    return r.group < ngroups ? r : RmsFp8wRow{ngroups - 1, n[ngroups - 1] - 1};
}
// 16-byte chunks per thread of the norm phase: 256 threads x rpt x 8 elements cover a row (rmsnorm_vec's RPT)
PLI_HD inline int rms_fp8w_norm_rpt(int k) {
    const int per = (k / kRmsFp8wNormChunk + 255) / 256;
    return per <= 1 ? 1 : per <= 2 ? 2 : 4;
}
// bytes of the LDS image y [m][k] of T, and the element offset in it of the 16 values of chunk cc of row bb
PLI_HD inline size_t rms_fp8w_lds_bytes(int m, int k) { return (size_t)m * (size_t)k * 2; }
PLI_HD inline int rms_fp8w_x_off(int bb, int cc, int k) { return (int)fp8w_vec_x_off(bb, cc, k); }

}  // namespace pli
