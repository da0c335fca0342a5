// Weight-only fp8 (W8A16) linear as pure C++17 (no HIP headers): the route
// rule of pli_linear_fp8w / pli_linear_swiglu_fp8w, the (ROWS, CPL) choice of
// linear_fp8w_vec, the k-step and the lane -> code-index map of
// linear_fp8w_smallm, every address clamp and the workspace size.  The
// functions carry PLI_HD (paged_plan.h), so the same text runs in the kernels
// and launchers of linear_fp8w.hip and in tests/host/fp8w_plan_check.cpp
// (tests/test_fp8w_plan.py).
//
// Layout: W8 [n, k] one e4m3fn code per byte, row-major, leading dimension
// ldw in bytes; w_scale fp32 [n]; value (j, i) = decode(code) * w_scale[j].
// X [m, k] and C [m, n] are 16-bit, leading dimensions in elements.
#pragma once

#include <cstddef>
#include <cstdint>

#include "paged_plan.h"

namespace pli {

// ------------------------------------------------------------------ routes --
enum Fp8wRoute {
    FP8W_EMPTY = 0,    // m == 0 or n == 0: nothing; k == 0: bias or 0 (generic kernel)
    FP8W_SMALLM = 1,   // linear_fp8w_smallm (MFMA)
    FP8W_VEC = 2,      // linear_fp8w_vec (VALU)
    FP8W_WIDEN = 3,    // fp8w_widen into the workspace, then pli_gemm / pli_gemm_swiglu
    FP8W_GENERIC = 4,  // linear_fp8w_generic
    FP8W_BAD_WORKSPACE = -1,  // FP8W_WIDEN would be taken, but the workspace is short or misaligned
};

constexpr int kFp8wChunk = 16;         // codes per 16-byte load
constexpr int kFp8wVecMaxM = 16;       // X rows linear_fp8w_vec takes
constexpr int kFp8wSmallmMaxM = 128;   // X rows linear_fp8w_smallm takes
// k-step of the small-M body: each of the 4 waves advances 64 codes per
// 16-byte load (4 lane groups x 16 codes), and K is split evenly over the
// waves, so K is a multiple of 4 x 64.
constexpr int kFp8wSmallmWaveStep = 64;
constexpr int kFp8wSmallmKStep = 4 * kFp8wSmallmWaveStep;  // 256

// What the route rule looks at.  Addresses are passed as integers so the rule
// is checked on the CPU with made-up values.
struct Fp8wCall {
    int m, n, k;
    int64_t ldx, ldw, ldc;      // SwiGLU: ldw = ldwg | ldwu (only its alignment is looked at)
    uintptr_t w, x, c, bias;    // SwiGLU: w = wg | wu
    uintptr_t ws;
    size_t ws_bytes;
    bool swiglu;
};

PLI_HD inline size_t fp8w_align16(size_t b) { return (b + 15) & ~(size_t)15; }
// bytes of one widened [n][k] 16-bit weight in the workspace
PLI_HD inline size_t fp8w_widened_bytes(int n, int k) { return fp8w_align16((size_t)n * (size_t)k * 2); }

PLI_HD inline bool fp8w_smallm_ok(const Fp8wCall& a) {
    return a.m > 1 && a.m <= kFp8wSmallmMaxM && a.k % kFp8wSmallmKStep == 0 && a.n % 16 == 0 &&
           ((a.w | a.x | a.c) & 15) == 0 && a.ldw % 16 == 0 && a.ldx % 8 == 0 && a.ldc % 8 == 0;
}
PLI_HD inline bool fp8w_vec_ok(const Fp8wCall& a) {
    return a.m <= kFp8wVecMaxM && a.k % kFp8wChunk == 0 && a.ldw % 16 == 0 && a.ldx % 8 == 0 &&
           ((a.w | a.x) & 15) == 0;
}
// pli_gemm's / pli_gemm_swiglu's vector alignment class over the widened
// weight (contiguous, leading dimension k, 16-byte aligned in the workspace)
PLI_HD inline bool fp8w_gemm_class(const Fp8wCall& a) {
    return a.k % 8 == 0 && a.n % 8 == 0 && a.ldx % 8 == 0 && a.ldc % 8 == 0 && ((a.x | a.c) & 15) == 0 &&
           (a.bias & 7) == 0;
}
// bytes the FP8W_WIDEN route needs
PLI_HD inline size_t fp8w_workspace_need(int n, int k, bool swiglu) {
    return (swiglu ? 2 : 1) * fp8w_widened_bytes(n, k);
}

// The route of a call, from host arguments only (a captured call replays).
PLI_HD inline int fp8w_route(const Fp8wCall& a) {
    if (a.m <= 0 || a.n <= 0 || a.k <= 0) return FP8W_EMPTY;
    if (fp8w_smallm_ok(a)) return FP8W_SMALLM;
    if (fp8w_vec_ok(a)) return FP8W_VEC;
    if (a.m > kFp8wVecMaxM && a.ws != 0 && fp8w_gemm_class(a)) {
        if ((a.ws & 15) != 0 || a.ws_bytes < fp8w_workspace_need(a.n, a.k, a.swiglu)) return FP8W_BAD_WORKSPACE;
        return FP8W_WIDEN;
    }
    return FP8W_GENERIC;
}

// pli_linear_fp8w_workspace_size: 0 where a fast route takes the shape
// (operands assumed aligned), the widened weight(s) otherwise.
PLI_HD inline size_t fp8w_workspace_size(int m, int n, int k, bool swiglu) {
    if (m <= kFp8wVecMaxM || n <= 0 || k <= 0) return 0;
    if (m <= kFp8wSmallmMaxM && k % kFp8wSmallmKStep == 0 && n % 16 == 0) return 0;
    return fp8w_workspace_need(n, k, swiglu);
}

// --------------------------------------------------------- linear_fp8w_vec --
// A wave owns `rows` consecutive W rows; lane l streams the 16-byte chunks
// l, l + 64, ... of each; `cpl` chunks per lane and row are issued per trip,
// all rows x cpl (x 2 for SwiGLU: gate and up) loads before the first use.
// Sized by bytes: rows x cpl (x 2) x 1 KiB = 8 KiB per wave, the bf16 GEMV's
// default.  A row of K codes has K / 16 chunks, so short rows (K <= 2048:
// at most 128 chunks, 2 per lane) get more rows per wave.
struct Fp8wVecCfg {
    int rows, cpl;
};
constexpr int kFp8wVecWaves = 4;  // waves per workgroup
PLI_HD inline Fp8wVecCfg fp8w_vec_cfg(int k, bool swiglu) {
    const bool short_row = k <= 2048;
    if (swiglu) return short_row ? Fp8wVecCfg{2, 2} : Fp8wVecCfg{1, 4};
    return short_row ? Fp8wVecCfg{4, 2} : Fp8wVecCfg{2, 4};
}
PLI_HD inline int fp8w_vec_grid(int n, int rows) { return (n + kFp8wVecWaves * rows - 1) / (kFp8wVecWaves * rows); }
// first row of a wave
PLI_HD inline int64_t fp8w_vec_row0(int block, int wave, int rows) {
    return ((int64_t)block * kFp8wVecWaves + wave) * rows;
}
// row r of the wave, clamped for the loads (rows >= n are loaded from row n - 1 and never stored)
PLI_HD inline int fp8w_vec_row(int64_t row0, int r, int n) {
    return (int)(row0 + r < n ? row0 + r : n - 1);
}
// chunk u of lane `lane` in the trip that starts at chunk c0; consumed when < nchunks
PLI_HD inline int fp8w_vec_chunk(int c0, int lane, int u) { return c0 + lane + 64 * u; }
PLI_HD inline int fp8w_vec_chunk_clamped(int cc, int nchunks) { return cc < nchunks ? cc : nchunks - 1; }
// byte offset of chunk cc of row `row` in W; element offset of its 16 X values in X row bb
PLI_HD inline int64_t fp8w_vec_w_off(int row, int cc, int64_t ldw) { return (int64_t)row * ldw + (int64_t)cc * 16; }
PLI_HD inline int64_t fp8w_vec_x_off(int bb, int cc, int64_t ldx) { return (int64_t)bb * ldx + (int64_t)cc * 16; }

// ------------------------------------------------------ linear_fp8w_smallm --
// One workgroup per 16 W rows, 4 waves, wave w owns k in [w K/4, (w+1) K/4).
// Per step s a lane (r16 = lane & 15, q = lane >> 4) loads the 16 codes
//   W[n0 + r16][w K/4 + 64 s + 16 q + 0..15],
// which fp8_widen16 turns into two v_mfma_f32_16x16x32 A operands: half h
// (0: lo, 1: hi) carries codes 8 h + 0..7.  The MFMA's k-slot 8 q + j of half
// h is therefore global k = base + 16 q + 8 h + j (a permutation of the 64
// k of the step), and the X fragment of half h is X[row][base + 16 q + 8 h +
// 0..7]: the lane reads 32 contiguous bytes of X per W load.
constexpr int kFp8wSmallmUnroll = 8;        // W loads issued ahead per wave: 8 x 1 KiB
constexpr int kFp8wSmallmUnrollSwiglu = 4;  // gate + up: 2 x 4 x 1 KiB
PLI_HD inline int fp8w_smallm_nbg(int m) { return m <= 16 ? 1 : m <= 32 ? 2 : m <= 64 ? 4 : 8; }
PLI_HD inline int fp8w_smallm_kw(int k) { return k / 4; }
// first k of lane's 16 codes at step s
PLI_HD inline int fp8w_smallm_k(int wave, int kw, int step, int lane) {
    return wave * kw + kFp8wSmallmWaveStep * step + 16 * (lane >> 4);
}
// global k of MFMA half h, element j of the lane's operand
PLI_HD inline int fp8w_smallm_k_of(int kbase, int h, int j) { return kbase + 8 * h + j; }
PLI_HD inline int fp8w_smallm_w_row(int n0, int lane, int n) {
    const int r = n0 + (lane & 15);
    return r < n ? r : n - 1;
}
PLI_HD inline int fp8w_smallm_x_row(int gi, int lane, int m) {
    const int r = gi * 16 + (lane & 15);
    return r < m ? r : m - 1;
}
PLI_HD inline int64_t fp8w_smallm_w_off(int row, int kbase, int64_t ldw) { return (int64_t)row * ldw + kbase; }
PLI_HD inline int64_t fp8w_smallm_x_off(int row, int kbase, int h, int64_t ldx) {
    return (int64_t)row * ldx + kbase + 8 * h;
}

}  // namespace pli
