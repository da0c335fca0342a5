// MXFP4 weights x MXFP4 activations (W4A4) on gfx950 (MI355X): the all-FP4 GEMM
//   C[r, j] = round_T( x_scale[r] * sum_i decode_e2m1(X4[r, i]) * 2^(x_exp[r, i/32] - 127)
//                                       * decode_e2m1(W4[j, i]) * 2^(w_exp[j, i/32] - 127)  (+ bias[j]) )
// X4 [m, k / 2] e2m1 code pairs, x_exp [m, k / 32] E8M0 block scales and one
// fp32 scale per row (what pli_quantize_rows_mxfp4 writes); W4 [n, k / 2] and
// w_exp [n, k / 32] in pli_linear_mxfp4w's format, nothing re-packed; C, bias
// 16-bit (T = bf16 / fp16).  Inside the two scale contracts (w: s - 127 in
// [-96, 96]; x: [-26, 26], mxfp4x_plan.h) a code x code x 2^(e_w + e_x) term is
// a normal fp32 number of at most 4 significant bits; the sum is fp32; x_scale
// and the bias come after the sum and the result is rounded once.
//
// Kernels (index arithmetic and routes: mxfp4x_plan.h over mxfp4a_plan.h and
// fp8a_plan.h):
//   gemm_mxfp4_a4_mx       gemm_fp8_mx's skeleton (128 x 128 tile, banded tile
//                          order, C^T, two LDS stages fed by 16-byte LDS-DMA) at
//                          a K-step of 256 codes: both operands are 128-byte
//                          rows in an image of gemm_fp8_mx's X shape, both are
//                          4-register e2m1 operands (cbsz = blgp = 4, one
//                          ds_read_b128 each), and both sides' E8M0 bytes go
//                          into the instruction's scale operands as stored
//   gemm_mxfp4_a4_generic  one thread per output through the header codecs, anything
#include "fp4_codec.h"
#include "fp8_kv.h"
#include "mx_finish.h"
#include "mxfp4x_plan.h"
#include "pli_common.h"

namespace pli {
namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// ---------------------------------------------------------------------------
// gemm_mxfp4_a4_mx: C^T tile [128 n][128 m] = W4 tile x X4 tile^T.  Per K-step
// of 256 codes every wave LDS-DMAs 4 KiB of each operand image (4 pieces of 8
// rows x 128 bytes, the swizzle on the source address) into stage (s + 1) % 2
// and loads, for each of its two W tiles and two X tiles, the two dwords of its
// row's eight scale bytes into registers, all in flight while the MFMAs run on
// stage s % 2: one vmcnt(0) and one barrier per step.  A wave multiplies its
// 64 x 64 block as 2 x 2 tiles of 32 x 32, four k-quarters of 64 codes each: 16
// scaled MFMAs per step at the e2m1 x e2m1 pass count, each operand one
// ds_read_b128, each scale one shift of a loaded dword.
//
// Operand maps: a lane's e2m1 operand is k = 32 (l >> 5) + j, j = 0 .. 31, on
// both sides; byte 0 of lane l's scale register is the scale of row (A) or
// column (B) l & 31 over the k of lane half l >> 5.  A 0xFF scale byte on the A
// side makes the instruction's output row NaN, on the B side its output column
// (the row of C).
template <typename T, bool BIAS>
__global__ __launch_bounds__(256) void gemm_mxfp4_a4_mx(const uint8_t* __restrict__ X4,
                                                        const uint8_t* __restrict__ x_exp,
                                                        const float* __restrict__ x_scale,
                                                        const uint8_t* __restrict__ W4,
                                                        const uint8_t* __restrict__ w_exp,
                                                        const uint16_t* __restrict__ bias, uint16_t* __restrict__ C,
                                                        int M, int N, int K, int64_t ldx4, int64_t ldxs, int64_t ldw,
                                                        int64_t lds, int64_t ldc, int tiles_m, int tiles_n) {
    __shared__ __attribute__((aligned(1024))) char smem[kMxfp4xLdsBytes];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave & 1, wm = wave >> 1;
    const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    const int m0 = fp8a_tile_m(t, tiles_m, tiles_n) * kFp8aTM, n0 = fp8a_tile_n(t, tiles_m, tiles_n) * kFp8aTN;
    const int ks = K / kMxfp4xKStep;

    // per-lane source offsets of the wave's pieces and scale dwords at K-step 0
    int64_t woff[kFp8aPiecesPerWave], xoff[kFp8aPiecesPerWave], wsoff[2], xsoff[2];
#pragma unroll
    for (int i = 0; i < kFp8aPiecesPerWave; ++i) {
        const int p = fp8a_stage_piece(wave, i);
        const int row = fp8a_stage_row(p, lane), c = fp8a_stage_chunk(p, lane);
        woff[i] = fp8a_src_off(n0, row, N, ldw, 0, c);
        xoff[i] = fp8a_src_off(m0, row, M, ldx4, 0, c);
    }
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        wsoff[tt] = mxfp4x_scale_off(n0, fp8a_frag_row(wn, tt, lane), N, lds, 0);
        xsoff[tt] = mxfp4x_scale_off(m0, fp8a_frag_row(wm, tt, lane), M, ldxs, 0);
    }

    uint32_t wsc_next[2][2], xsc_next[2][2];  // [tile][dword]: the scale bytes of the step in flight
    auto stage = [&](int s) __attribute__((always_inline)) {
        char* img = smem + (s % kMxfp4xStages) * kMxfp4xStageBytes;
#pragma unroll
        for (int i = 0; i < kFp8aPiecesPerWave; ++i) {
            // the LDS address is the wave's piece base: the hardware adds 16 x lane
            const int lds_off = fp8a_stage_lds(fp8a_stage_piece(wave, i), 0);
            __builtin_amdgcn_global_load_lds(W4 + woff[i] + (int64_t)s * kFp8aRowBytes, (lds_void*)(img + lds_off), 16,
                                             0, 0);
            __builtin_amdgcn_global_load_lds(X4 + xoff[i] + (int64_t)s * kFp8aRowBytes,
                                             (lds_void*)(img + kFp8aImgBytes + lds_off), 16, 0, 0);
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                wsc_next[tt][d] = *reinterpret_cast<const uint32_t*>(w_exp + wsoff[tt] +
                                                                     (int64_t)s * kMxfp4xStepScales + 4 * d);
                xsc_next[tt][d] = *reinterpret_cast<const uint32_t*>(x_exp + xsoff[tt] +
                                                                     (int64_t)s * kMxfp4xStepScales + 4 * d);
            }
    };

    // fragment read offsets inside a stage: [tile][k-quarter]
    int wrd[2][kMxfp4xQuarters], xrd[2][kMxfp4xQuarters];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int q = 0; q < kMxfp4xQuarters; ++q) {
            wrd[tt][q] = fp8a_frag_lds(fp8a_frag_row(wn, tt, lane), mxfp4x_frag_chunk(q, lane));
            xrd[tt][q] = kFp8aImgBytes + fp8a_frag_lds(fp8a_frag_row(wm, tt, lane), mxfp4x_frag_chunk(q, lane));
        }
    const int shift0 = mxfp4x_scale_shift(0, lane), shift1 = mxfp4x_scale_shift(1, lane);

    f32x16 acc[2][2];  // [nt][mt]
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nt][mt][r] = 0.f;

    stage(0);
    for (int s = 0; s < ks; ++s) {
        // step s has landed (this wave's pieces and scale dwords; the barrier covers the others' pieces), and
        // every wave is done reading the stage that step s + 1 overwrites.  The dwords pass through the
        // statement so that nothing derived from them is scheduled in front of the wait.
        asm volatile("s_waitcnt vmcnt(0)"
                     : "+v"(wsc_next[0][0]), "+v"(wsc_next[0][1]), "+v"(wsc_next[1][0]), "+v"(wsc_next[1][1]),
                       "+v"(xsc_next[0][0]), "+v"(xsc_next[0][1]), "+v"(xsc_next[1][0]), "+v"(xsc_next[1][1])::"memory");
        __syncthreads();
        uint32_t wsc[2][2], xsc[2][2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                wsc[tt][d] = wsc_next[tt][d];
                xsc[tt][d] = xsc_next[tt][d];
            }
        if (s + 1 < ks) stage(s + 1);
        const char* img = smem + (s % kMxfp4xStages) * kMxfp4xStageBytes;
#pragma unroll
        for (int q = 0; q < kMxfp4xQuarters; ++q) {
            const int shift = q & 1 ? shift1 : shift0, d = mxfp4x_scale_dword(q);
            i32x8 wf[2], xf[2];
            int ws[2], xs[2];  // byte 0 is the block's scale
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const i32x4 w = lds_read_b128(img, wrd[tt][q]), x = lds_read_b128(img, xrd[tt][q]);
                wf[tt] = i32x8{w.x, w.y, w.z, w.w, 0, 0, 0, 0};  // cbsz = blgp = 4 read the first four registers
                xf[tt] = i32x8{x.x, x.y, x.z, x.w, 0, 0, 0, 0};
                ws[tt] = (int)(wsc[tt][d] >> shift);
                xs[tt] = (int)(xsc[tt][d] >> shift);
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    // cbsz = 4: e2m1 A; blgp = 4: e2m1 B; both scales: byte 0 of the lane's register
                    acc[nt][mt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[nt], xf[mt], acc[nt][mt], 4, 4, 0,
                                                                                   ws[nt], 0, xs[mt]);
        }
    }

    // epilogue: a lane holds, per tile and register group g, 4 consecutive n of one m
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int mrow = m0 + fp8a_acc_m(wm, mt, lane);
        if (mrow >= M) continue;
        const float xs = fp8_scale_of(x_scale, mrow);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ncol = n0 + fp8a_acc_n(wn, nt, lane, 4 * g);
                if (ncol >= N) continue;  // N % 4 == 0: the group is inside or outside as a whole
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v[r] = mxfp4a_finish(acc[nt][mt][4 * g + r], xs);
                    if constexpr (BIAS) v[r] += elem<T>::to_f32(T{bias[ncol + r]});
                }
                *reinterpret_cast<i32x2*>(C + (int64_t)mrow * ldc + ncol) =
                    i32x2{(int)pack2<T>(v[0], v[1]), (int)pack2<T>(v[2], v[3])};
            }
    }
}

// ---------------------------------------------------------------------------
// gemm_mxfp4_a4_generic: one thread per output, any M / N / K / ld / alignment,
// K = 0 (bias or 0).  Decodes with the header codecs; fp32 fma in k order; the
// two block scales multiply exactly inside the contracts.  A 0xFF scale byte on
// either side decodes to NaN and poisons the sum.
template <typename T>
__global__ __launch_bounds__(256) void gemm_mxfp4_a4_generic(const uint8_t* __restrict__ X4,
                                                             const uint8_t* __restrict__ x_exp,
                                                             const float* __restrict__ x_scale,
                                                             const uint8_t* __restrict__ W4,
                                                             const uint8_t* __restrict__ w_exp,
                                                             const T* __restrict__ bias, T* __restrict__ C, int M,
                                                             int N, int K, int64_t ldx4, int64_t ldxs, int64_t ldw,
                                                             int64_t lds, int64_t ldc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)M * N) return;
    const int r = (int)(i / N), j = (int)(i % N);
    const uint8_t* x = X4 + (int64_t)r * ldx4;
    const uint8_t* xe = x_exp + (int64_t)r * ldxs;
    const uint8_t* w = W4 + (int64_t)j * ldw;
    const uint8_t* we = w_exp + (int64_t)j * lds;
    float sum = 0.f;
    for (int b = 0; b < K / kMxfp4aBlock; ++b) {
        const float scale = e8m0_decode(we[b]) * e8m0_decode(xe[b]);
        for (int kk = b * kMxfp4aBlock; kk < (b + 1) * kMxfp4aBlock; ++kk)
            sum = fmaf(fp4_e2m1_decode(fp4_nibble(x[kk >> 1], kk)), fp4_e2m1_decode(fp4_nibble(w[kk >> 1], kk)) * scale,
                       sum);
    }
    float v = mxfp4a_finish(sum, fp8_scale_of(x_scale, r));
    if (bias) v += elem<T>::to_f32(bias[j]);
    C[(int64_t)r * ldc + j] = elem<T>::from_f32(v);
}

// ------------------------------------------------------------------ launch --
struct Mxfp4xArgs {
    const void *x4, *x_exp, *w4, *w_exp, *bias;
    const float* x_scale;
    void* c;
    int m, n, k;
    int64_t ldx4, ldxs, ldw, lds, ldc;
};

template <typename T>
int launch_mx(const Mxfp4xArgs& a, hipStream_t s) {
    const int tiles_m = fp8a_tiles(a.m, kFp8aTM), tiles_n = fp8a_tiles(a.n, kFp8aTN);
    const int nblocks = tiles_m * tiles_n;
#define PLI_MXFP4X_MX(BIAS)                                                                                          \
    hipLaunchKernelGGL((gemm_mxfp4_a4_mx<T, BIAS>), dim3(nblocks), dim3(256), 0, s, (const uint8_t*)a.x4,            \
                       (const uint8_t*)a.x_exp, a.x_scale, (const uint8_t*)a.w4, (const uint8_t*)a.w_exp,            \
                       (const uint16_t*)a.bias, (uint16_t*)a.c, a.m, a.n, a.k, a.ldx4, a.ldxs, a.ldw, a.lds, a.ldc, \
                       tiles_m, tiles_n)
    if (a.bias) PLI_MXFP4X_MX(true);
    else PLI_MXFP4X_MX(false);
#undef PLI_MXFP4X_MX
    return launch_status("gemm_mxfp4_a4_mx");
}

template <typename T>
int launch_generic(const Mxfp4xArgs& a, hipStream_t s) {
    const int64_t blocks = ((int64_t)a.m * a.n + 255) / 256;
    hipLaunchKernelGGL((gemm_mxfp4_a4_generic<T>), dim3((unsigned)blocks), dim3(256), 0, s, (const uint8_t*)a.x4,
                       (const uint8_t*)a.x_exp, a.x_scale, (const uint8_t*)a.w4, (const uint8_t*)a.w_exp,
                       (const T*)a.bias, (T*)a.c, a.m, a.n, a.k, a.ldx4, a.ldxs, a.ldw, a.lds, a.ldc);
    return launch_status("gemm_mxfp4_a4_generic");
}

}  // namespace
}  // namespace pli

extern "C" int pli_gemm_mxfp4_a4(const void* x4, const void* x_exp, const float* x_scale, const void* w4,
                                 const void* w_exp, const void* bias, void* c, int m, int n, int k, int64_t ldx4,
                                 int64_t ldxs, int64_t ldw, int64_t lds, int64_t ldc, int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(dtype == PLI_F16 || dtype == PLI_BF16, "pli_gemm_mxfp4_a4: bad dtype %d (fp16 / bf16 output only)",
                dtype);
    PLI_REQUIRE(m >= 0 && n >= 0 && k >= 0, "pli_gemm_mxfp4_a4: bad shape m=%d n=%d k=%d", m, n, k);
    PLI_REQUIRE(mxfp4a_shape_ok(k), "pli_gemm_mxfp4_a4: k=%d is not a multiple of the MX block of 32", k);
    PLI_REQUIRE(ldx4 >= k / 2 && ldxs >= k / kMxfp4aBlock && ldw >= k / 2 && lds >= k / kMxfp4aBlock && ldc >= n,
                "pli_gemm_mxfp4_a4: leading dimension too small (ldx4=%lld ldxs=%lld ldw=%lld lds=%lld ldc=%lld)",
                (long long)ldx4, (long long)ldxs, (long long)ldw, (long long)lds, (long long)ldc);
    if (m == 0 || n == 0) return PLI_OK;  // empty operands may be NULL
    PLI_REQUIRE(c && (k == 0 || (x4 && x_exp && w4 && w_exp)),
                "pli_gemm_mxfp4_a4: null pointer (the scale bytes have no default)");
    PLI_REQUIRE(((int64_t)m * n + 255) / 256 <= 0x7fffffffLL, "pli_gemm_mxfp4_a4: grid too large");
    const Mxfp4xCall call{m, n, k, ldx4, ldxs, ldw, lds, ldc, (uintptr_t)x4, (uintptr_t)x_exp, (uintptr_t)w4,
                          (uintptr_t)w_exp, (uintptr_t)c};
    const Mxfp4xArgs a{x4, x_exp, w4, w_exp, bias, x_scale, c, m, n, k, ldx4, ldxs, ldw, lds, ldc};
    hipStream_t s = (hipStream_t)stream;
    if (mxfp4x_route(call) == MXFP4X_MX)
        return dtype == PLI_BF16 ? launch_mx<bf16_t>(a, s) : launch_mx<f16_t>(a, s);
    return dtype == PLI_BF16 ? launch_generic<bf16_t>(a, s) : launch_generic<f16_t>(a, s);
}
