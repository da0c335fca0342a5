// Weight-only MXFP4 (W4A16) linear as pure C++17 (no HIP headers): the route
// rule of pli_linear_mxfp4w / pli_linear_swiglu_mxfp4w, the (ROWS, CPL) choice
// of mxfp4w_vec, the k granule and the lane -> (row, block, k) map of
// mxfp4w_smallm, every address clamp and the workspace size.  The functions
// carry PLI_HD (paged_plan.h), so the same text runs in the kernels and
// launchers of linear_mxfp4w.hip and in tests/host/mxfp4w_plan_check.cpp
// (tests/test_mxfp4w_plan.py).
//
// Layout: w4 [n, k / 2] bytes of two e2m1 codes (element i in byte i / 2, even
// i in bits 3:0), row-major, leading dimension ldw in bytes; w_exp [n, k / 32]
// E8M0 bytes, leading dimension lds; block b of row j covers k in
// [32 b, 32 b + 32); value (j, i) = decode(code) * 2^(w_exp[j, i / 32] - 127).
// X [m, k] and C [m, n] are 16-bit, leading dimensions in elements.  A
// 16-byte load of w4 is 32 codes: exactly one block, one scale byte.
#pragma once

#include <cstddef>
#include <cstdint>

#include "paged_plan.h"

namespace pli {

// ------------------------------------------------------------------ routes --
enum Mxfp4wRoute {
    MXFP4W_EMPTY = 0,    // m == 0 or n == 0: nothing; k == 0: bias or 0 (generic kernel)
    MXFP4W_SMALLM = 1,   // mxfp4w_smallm (MFMA)
    MXFP4W_VEC = 2,      // mxfp4w_vec (VALU)
    MXFP4W_WIDEN = 3,    // mxfp4w_widen into the workspace, then pli_gemm / pli_gemm_swiglu
    MXFP4W_GENERIC = 4,  // mxfp4w_generic
    MXFP4W_BAD_WORKSPACE = -1,  // MXFP4W_WIDEN would be taken, but the workspace is short or misaligned
};

constexpr int kMxfp4Block = 32;           // elements per E8M0 scale = codes per 16-byte load
constexpr int kMxfp4wVecMaxM = 16;        // X rows mxfp4w_vec takes
constexpr int kMxfp4wSmallmMaxM = 128;    // X rows mxfp4w_smallm takes
// The vec / smallm crossover, measured (tools/mxfp4w_linear_bench.py --sections routes, profiles/mxfp4w/): on
// 8192^2 and 28672 x 8192 mxfp4w_smallm / mxfp4w_vec is 0.96-0.97 at M = 2, 0.67-0.70 at 4, 0.46-0.49 at 8 and
// 0.29-0.33 at 16, so the MFMA kernel takes every M >= 2 on its granule, as in fp8w's rule.
constexpr int kMxfp4wSmallmMinM = 2;
// k granule of the small-M body: each of the 4 waves advances 128 k per
// 16-byte load (4 lane groups x one block of 32), and K is split evenly over
// the waves, so K is a multiple of 4 x 4 x 32.
constexpr int kMxfp4wSmallmWaveStep = 4 * kMxfp4Block;           // 128 k
constexpr int kMxfp4wSmallmKStep = 4 * kMxfp4wSmallmWaveStep;    // 512

// What the route rule looks at.  Addresses are passed as integers so the rule
// is checked on the CPU with made-up values.  The scale bytes are read one at
// a time, so neither their address nor lds enters the rule.
struct Mxfp4wCall {
    int m, n, k;
    int64_t ldx, ldw, ldc;      // ldw in bytes; SwiGLU: ldw = ldwg | ldwu (only its alignment is looked at)
    uintptr_t w, x, c, bias;    // SwiGLU: w = wg4 | wu4
    uintptr_t ws;
    size_t ws_bytes;
    bool swiglu;
};

PLI_HD inline bool mxfp4w_shape_ok(int k) { return k % kMxfp4Block == 0; }
PLI_HD inline size_t mxfp4w_align16(size_t b) { return (b + 15) & ~(size_t)15; }
// bytes of one widened [n][k] 16-bit weight in the workspace
PLI_HD inline size_t mxfp4w_widened_bytes(int n, int k) { return mxfp4w_align16((size_t)n * (size_t)k * 2); }

PLI_HD inline bool mxfp4w_smallm_ok(const Mxfp4wCall& a) {
    return a.m >= kMxfp4wSmallmMinM && a.m <= kMxfp4wSmallmMaxM && a.k % kMxfp4wSmallmKStep == 0 && a.n % 16 == 0 &&
           ((a.w | a.x | a.c) & 15) == 0 && a.ldw % 16 == 0 && a.ldx % 8 == 0 && a.ldc % 8 == 0;
}
PLI_HD inline bool mxfp4w_vec_ok(const Mxfp4wCall& a) {
    return a.m <= kMxfp4wVecMaxM && a.k % kMxfp4Block == 0 && a.ldw % 16 == 0 && a.ldx % 8 == 0 &&
           ((a.w | a.x) & 15) == 0;
}
// pli_gemm's / pli_gemm_swiglu's vector alignment class over the widened
// weight (contiguous, leading dimension k, 16-byte aligned in the workspace)
PLI_HD inline bool mxfp4w_gemm_class(const Mxfp4wCall& a) {
    return a.k % 8 == 0 && a.n % 8 == 0 && a.ldx % 8 == 0 && a.ldc % 8 == 0 && ((a.x | a.c) & 15) == 0 &&
           (a.bias & 7) == 0;
}
PLI_HD inline size_t mxfp4w_workspace_need(int n, int k, bool swiglu) {
    return (swiglu ? 2 : 1) * mxfp4w_widened_bytes(n, k);
}

// The route of a call (k % 32 == 0 was checked), from host arguments only (a
// captured call replays).
PLI_HD inline int mxfp4w_route(const Mxfp4wCall& a) {
    if (a.m <= 0 || a.n <= 0 || a.k <= 0) return MXFP4W_EMPTY;
    if (mxfp4w_smallm_ok(a)) return MXFP4W_SMALLM;
    if (mxfp4w_vec_ok(a)) return MXFP4W_VEC;
    if (a.m > kMxfp4wVecMaxM && a.ws != 0 && mxfp4w_gemm_class(a)) {
        if ((a.ws & 15) != 0 || a.ws_bytes < mxfp4w_workspace_need(a.n, a.k, a.swiglu)) return MXFP4W_BAD_WORKSPACE;
        return MXFP4W_WIDEN;
    }
    return MXFP4W_GENERIC;
}

// pli_linear_mxfp4w_workspace_size: 0 where a fast route takes the shape
// (operands assumed aligned), the widened weight(s) otherwise.
PLI_HD inline size_t mxfp4w_workspace_size(int m, int n, int k, bool swiglu) {
    if (m <= kMxfp4wVecMaxM || n <= 0 || k <= 0 || !mxfp4w_shape_ok(k)) return 0;
    if (m <= kMxfp4wSmallmMaxM && k % kMxfp4wSmallmKStep == 0 && n % 16 == 0) return 0;
    return mxfp4w_workspace_need(n, k, swiglu);
}

// -------------------------------------------------------------- mxfp4w_vec --
// A wave owns `rows` consecutive weight rows; lane l streams the 16-byte
// chunks (= blocks) l, l + 64, ... of each; `cpl` chunks per lane and row are
// issued per trip, all rows x cpl (x 2 for SwiGLU: gate and up) code loads and
// their scale-byte loads before the first use.  Sized by bytes, as
// fp8w_vec_cfg: rows x cpl (x 2) x 1 KiB = 8 KiB per wave.  A row of K codes
// is K / 2 bytes = K / 32 chunks, half an fp8 row's, so short rows get more
// rows per wave: K <= 2048 is at most one chunk per lane (8 rows), K <= 4096
// at most two (4 rows), longer rows four (2 rows).
struct Mxfp4wVecCfg {
    int rows, cpl;
};
constexpr int kMxfp4wVecWaves = 4;  // waves per workgroup
PLI_HD inline Mxfp4wVecCfg mxfp4w_vec_cfg(int k, bool swiglu) {
    const int cpl = k <= 2048 ? 1 : k <= 4096 ? 2 : 4;
    return Mxfp4wVecCfg{(swiglu ? 4 : 8) / cpl, cpl};
}
PLI_HD inline int mxfp4w_vec_grid(int n, int rows) {
    return (n + kMxfp4wVecWaves * rows - 1) / (kMxfp4wVecWaves * rows);
}
// first row of a wave
PLI_HD inline int64_t mxfp4w_vec_row0(int block, int wave, int rows) {
    return ((int64_t)block * kMxfp4wVecWaves + wave) * rows;
}
// row r of the wave, clamped for the loads (rows >= n are loaded from row n - 1 and never stored)
PLI_HD inline int mxfp4w_vec_row(int64_t row0, int r, int n) {
    return (int)(row0 + r < n ? row0 + r : n - 1);
}
// chunk u of lane `lane` in the trip that starts at chunk c0; consumed when < nchunks
PLI_HD inline int mxfp4w_vec_chunk(int c0, int lane, int u) { return c0 + lane + 64 * u; }
PLI_HD inline int mxfp4w_vec_chunk_clamped(int cc, int nchunks) { return cc < nchunks ? cc : nchunks - 1; }
// byte offset of chunk cc of row `row` in w4, of its scale byte in w_exp, and
// the element offset of its 32 X values in X row bb
PLI_HD inline int64_t mxfp4w_vec_w_off(int row, int cc, int64_t ldw) { return (int64_t)row * ldw + (int64_t)cc * 16; }
PLI_HD inline int64_t mxfp4w_vec_s_off(int row, int cc, int64_t lds) { return (int64_t)row * lds + cc; }
PLI_HD inline int64_t mxfp4w_vec_x_off(int bb, int cc, int64_t ldx) {
    return (int64_t)bb * ldx + (int64_t)cc * kMxfp4Block;
}

// ----------------------------------------------------------- mxfp4w_smallm --
// One workgroup per 16 weight rows, 4 waves, wave w owns k in [w K/4, (w+1) K/4).
// Per step s a lane (r16 = lane & 15, q = lane >> 4) loads the block
//   w4[n0 + r16][k = w K/4 + 128 s + 32 q + 0..31]   (16 bytes, one scale byte),
// which widens, the scale folded in, to four v_mfma_f32_16x16x32 A operands:
// operand h (0..3) carries elements 8 h + 0..7.  The MFMA's k-slot 8 q + j of
// operand h is therefore global k = base + 32 q + 8 h + j (a permutation of
// the 128 k of the step), and the X fragment of operand h is
// X[row][base + 32 q + 8 h + 0..7]: the lane reads 64 contiguous bytes of X
// per W load.
constexpr int kMxfp4wSmallmUnroll = 8;        // W loads issued ahead per wave: 8 x 1 KiB
constexpr int kMxfp4wSmallmUnrollSwiglu = 4;  // gate + up: 2 x 4 x 1 KiB
PLI_HD inline int mxfp4w_smallm_nbg(int m) { return m <= 16 ? 1 : m <= 32 ? 2 : m <= 64 ? 4 : 8; }
PLI_HD inline int mxfp4w_smallm_kw(int k) { return k / 4; }
// first k of the lane's block at step s
PLI_HD inline int mxfp4w_smallm_k(int wave, int kw, int step, int lane) {
    return wave * kw + kMxfp4wSmallmWaveStep * step + kMxfp4Block * (lane >> 4);
}
// global k of element j of the lane's operand h
PLI_HD inline int mxfp4w_smallm_k_of(int kbase, int h, int j) { return kbase + 8 * h + j; }
PLI_HD inline int mxfp4w_smallm_w_row(int n0, int lane, int n) {
    const int r = n0 + (lane & 15);
    return r < n ? r : n - 1;
}
PLI_HD inline int mxfp4w_smallm_x_row(int gi, int lane, int m) {
    const int r = gi * 16 + (lane & 15);
    return r < m ? r : m - 1;
}
PLI_HD inline int64_t mxfp4w_smallm_w_off(int row, int kbase, int64_t ldw) { return (int64_t)row * ldw + kbase / 2; }
PLI_HD inline int64_t mxfp4w_smallm_s_off(int row, int kbase, int64_t lds) {
    return (int64_t)row * lds + kbase / kMxfp4Block;
}
PLI_HD inline int64_t mxfp4w_smallm_x_off(int row, int kbase, int h, int64_t ldx) {
    return (int64_t)row * ldx + kbase + 8 * h;
}

}  // namespace pli
