// MXFP4 weights x fp8 e4m3 activations (W4A8) on gfx950 (MI355X): the prefill GEMM
//   C[r, j] = round_T( x_scale[r] * sum_i decode_e4m3(X8[r, i]) * decode_e2m1(W4[j, i]) * 2^(w_exp[j, i/32] - 127)
//                      (+ bias[j]) )
// X8 [m, k] OCP e4m3fn codes and one fp32 scale per row (what pli_quantize_rows_fp8
// writes); W4 [n, k / 2] e2m1 code pairs and w_exp [n, k / 32] E8M0 block scales
// (pli_linear_mxfp4w's format, nothing re-packed); C, bias 16-bit (T = bf16 /
// fp16).  Inside the scale contract (s - 127 in [-96, 96]) a code x code x 2^e
// term is a normal fp32 number of at most 6 significant bits; the sum is fp32;
// x_scale and the bias come after the sum and the result is rounded once.
//
// Kernels (index arithmetic and routes: mxfp4a_plan.h over fp8a_plan.h, checked
// on the CPU by tests/host/mxfp4a_plan_check.cpp):
//   gemm_mxfp4_mx       gemm_fp8_mx's skeleton (128 x 128 tile, banded tile
//                       order, C^T, two LDS stages fed by 16-byte LDS-DMA) with a
//                       W side of its own: a 64-byte row per K-step in an 8 KiB
//                       image with its own swizzle, one ds_read_b128 per e2m1
//                       operand (cbsz = 4), and the weight's E8M0 bytes loaded
//                       straight into the instruction's scale register
//   gemm_mxfp4_generic  one thread per output through the header codecs, anything
#include "fp4_codec.h"
#include "fp8_kv.h"
#include "mx_finish.h"
#include "mxfp4a_plan.h"
#include "pli_common.h"

namespace pli {
namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// The shared epilogue expression, mxfp4a_finish (mx_finish.h): the two kernels
// agree bit for bit wherever their sums do.

// ---------------------------------------------------------------------------
// gemm_mxfp4_mx: C^T tile [128 n][128 m] = W4 tile x X8 tile^T.  Per K-step of
// 128 codes every wave LDS-DMAs 2 KiB of the W image (2 pieces of 16 rows x 64
// bytes) and 4 KiB of the X image (4 pieces of 8 rows x 128 bytes) into stage
// (s + 1) % 2 and loads two dwords of scale bytes (one per W tile) into
// registers, all in flight while the MFMAs run on stage s % 2: one vmcnt(0) and
// one barrier per step.  A wave multiplies its 64 x 64 block as 2 x 2 tiles of
// 32 x 32, two k-halves of 64 codes each: 8 scaled MFMAs per step, the W
// operand one ds_read_b128, the X operand two.
//
// Operand k maps (settled on the device): a lane's e2m1 operand is k = 32 (l >> 5)
// + j, j = 0 .. 31, but its e4m3 operand is k = 32 (j >> 4) + 16 (l >> 5) + (j & 15)
// in byte j, so the X fragment halves are read crosswise (mxfp4a_xfrag_chunk).
// A 0xFF scale byte makes the instruction's whole output row NaN by itself.
template <typename T, bool BIAS>
__global__ __launch_bounds__(256) void gemm_mxfp4_mx(const uint8_t* __restrict__ X8, const float* __restrict__ x_scale,
                                                     const uint8_t* __restrict__ W4,
                                                     const uint8_t* __restrict__ w_exp,
                                                     const uint16_t* __restrict__ bias, uint16_t* __restrict__ C,
                                                     int M, int N, int K, int64_t ldx8, int64_t ldw, int64_t lds,
                                                     int64_t ldc, int tiles_m, int tiles_n) {
    __shared__ __attribute__((aligned(1024))) char smem[kMxfp4aLdsBytes];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave & 1, wm = wave >> 1;
    const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    const int m0 = fp8a_tile_m(t, tiles_m, tiles_n) * kFp8aTM, n0 = fp8a_tile_n(t, tiles_m, tiles_n) * kFp8aTN;
    const int ks = K / kMxfp4aKStep;

    // per-lane source offsets of the wave's pieces and scale dwords at K-step 0
    int64_t woff[kMxfp4aWPiecesPerWave], xoff[kFp8aPiecesPerWave], soff[2];
#pragma unroll
    for (int i = 0; i < kMxfp4aWPiecesPerWave; ++i) {
        const int p = mxfp4a_stage_piece(wave, i);
        woff[i] = mxfp4a_w_off(n0, mxfp4a_stage_row(p, lane), N, ldw, 0, mxfp4a_stage_chunk(p, lane));
    }
#pragma unroll
    for (int i = 0; i < kFp8aPiecesPerWave; ++i) {
        const int p = fp8a_stage_piece(wave, i);
        xoff[i] = fp8a_src_off(m0, fp8a_stage_row(p, lane), M, ldx8, 0, fp8a_stage_chunk(p, lane));
    }
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) soff[tt] = mxfp4a_scale_off(n0, fp8a_frag_row(wn, tt, lane), N, lds, 0);

    uint32_t sc_next[2];  // the scale dwords of the step in flight
    auto stage = [&](int s) __attribute__((always_inline)) {
        char* img = smem + (s % kMxfp4aStages) * kMxfp4aStageBytes;
        // the LDS address is the wave's piece base: the hardware adds 16 x lane
#pragma unroll
        for (int i = 0; i < kMxfp4aWPiecesPerWave; ++i)
            __builtin_amdgcn_global_load_lds(W4 + woff[i] + (int64_t)s * kMxfp4aWRowBytes,
                                             (lds_void*)(img + mxfp4a_stage_lds(mxfp4a_stage_piece(wave, i), 0)), 16,
                                             0, 0);
#pragma unroll
        for (int i = 0; i < kFp8aPiecesPerWave; ++i)
            __builtin_amdgcn_global_load_lds(
                X8 + xoff[i] + (int64_t)s * kFp8aKStep,
                (lds_void*)(img + kMxfp4aWImgBytes + fp8a_stage_lds(fp8a_stage_piece(wave, i), 0)), 16, 0, 0);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
            sc_next[tt] = *reinterpret_cast<const uint32_t*>(w_exp + soff[tt] + (int64_t)s * (kMxfp4aKStep / kMxfp4aBlock));
    };

    // fragment read offsets inside a stage: W [tile][k-half], X [tile][k-half][16-byte half]
    int wrd[2][2], xrd[2][2][2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            wrd[tt][kh] = mxfp4a_frag_lds(fp8a_frag_row(wn, tt, lane), mxfp4a_frag_chunk(kh, lane));
#pragma unroll
            for (int h = 0; h < 2; ++h)
                xrd[tt][kh][h] =
                    kMxfp4aWImgBytes + fp8a_frag_lds(fp8a_frag_row(wm, tt, lane), mxfp4a_xfrag_chunk(kh, lane, h));
        }
    const int shift0 = mxfp4a_scale_shift(0, lane), shift1 = mxfp4a_scale_shift(1, lane);

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
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(sc_next[0]), "+v"(sc_next[1])::"memory");
        __syncthreads();
        int sc[2][2];  // [tile][k-half]: byte 0 is the block's scale
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            sc[tt][0] = (int)(sc_next[tt] >> shift0);
            sc[tt][1] = (int)(sc_next[tt] >> shift1);
        }
        if (s + 1 < ks) stage(s + 1);
        const char* img = smem + (s % kMxfp4aStages) * kMxfp4aStageBytes;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            i32x8 wf[2], xf[2];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const i32x4 w = lds_read_b128(img, wrd[tt][kh]);
                const i32x4 xl = lds_read_b128(img, xrd[tt][kh][0]), xh = lds_read_b128(img, xrd[tt][kh][1]);
                wf[tt] = i32x8{w.x, w.y, w.z, w.w, 0, 0, 0, 0};  // cbsz = 4 reads the first four registers
                xf[tt] = i32x8{xl.x, xl.y, xl.z, xl.w, xh.x, xh.y, xh.z, xh.w};
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    // cbsz = 4: e2m1 A; blgp = 0: e4m3 B; A scale: byte 0 of the lane's register; B scale 2^0
                    acc[nt][mt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[nt], xf[mt], acc[nt][mt], 4, 0, 0,
                                                                                   sc[nt][kh], 0, 127);
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
// gemm_mxfp4_generic: one thread per output, any M / N / K / ld / alignment,
// K = 0 (bias or 0).  Decodes with the header codecs; fp32 fma in k order.  A
// 0xFF scale byte decodes to NaN and poisons the sum.
template <typename T>
__global__ __launch_bounds__(256) void gemm_mxfp4_generic(const uint8_t* __restrict__ X8,
                                                          const float* __restrict__ x_scale,
                                                          const uint8_t* __restrict__ W4,
                                                          const uint8_t* __restrict__ w_exp,
                                                          const T* __restrict__ bias, T* __restrict__ C, int M, int N,
                                                          int K, int64_t ldx8, int64_t ldw, int64_t lds, int64_t ldc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)M * N) return;
    const int r = (int)(i / N), j = (int)(i % N);
    const uint8_t* x = X8 + (int64_t)r * ldx8;
    const uint8_t* w = W4 + (int64_t)j * ldw;
    const uint8_t* e = w_exp + (int64_t)j * lds;
    float sum = 0.f;
    for (int b = 0; b < K / kMxfp4aBlock; ++b) {
        const float scale = e8m0_decode(e[b]);
        for (int kk = b * kMxfp4aBlock; kk < (b + 1) * kMxfp4aBlock; ++kk)
            sum = fmaf(fp8_e4m3_decode(x[kk]), fp4_e2m1_decode(fp4_nibble(w[kk >> 1], kk)) * scale, sum);
    }
    float v = mxfp4a_finish(sum, fp8_scale_of(x_scale, r));
    if (bias) v += elem<T>::to_f32(bias[j]);
    C[(int64_t)r * ldc + j] = elem<T>::from_f32(v);
}

// ------------------------------------------------------------------ launch --
struct Mxfp4aArgs {
    const void *x8, *w4, *w_exp, *bias;
    const float* x_scale;
    void* c;
    int m, n, k;
    int64_t ldx8, ldw, lds, ldc;
};

template <typename T>
int launch_mx(const Mxfp4aArgs& a, hipStream_t s) {
    const int tiles_m = fp8a_tiles(a.m, kFp8aTM), tiles_n = fp8a_tiles(a.n, kFp8aTN);
    const int nblocks = tiles_m * tiles_n;
#define PLI_MXFP4A_MX(BIAS)                                                                                         \
    hipLaunchKernelGGL((gemm_mxfp4_mx<T, BIAS>), dim3(nblocks), dim3(256), 0, s, (const uint8_t*)a.x8, a.x_scale,   \
                       (const uint8_t*)a.w4, (const uint8_t*)a.w_exp, (const uint16_t*)a.bias, (uint16_t*)a.c, a.m, \
                       a.n, a.k, a.ldx8, a.ldw, a.lds, a.ldc, tiles_m, tiles_n)
    if (a.bias) PLI_MXFP4A_MX(true);
    else PLI_MXFP4A_MX(false);
#undef PLI_MXFP4A_MX
    return launch_status("gemm_mxfp4_mx");
}

template <typename T>
int launch_generic(const Mxfp4aArgs& a, hipStream_t s) {
    const int64_t blocks = ((int64_t)a.m * a.n + 255) / 256;
    hipLaunchKernelGGL((gemm_mxfp4_generic<T>), dim3((unsigned)blocks), dim3(256), 0, s, (const uint8_t*)a.x8,
                       a.x_scale, (const uint8_t*)a.w4, (const uint8_t*)a.w_exp, (const T*)a.bias, (T*)a.c, a.m, a.n,
                       a.k, a.ldx8, a.ldw, a.lds, a.ldc);
    return launch_status("gemm_mxfp4_generic");
}

}  // namespace
}  // namespace pli

extern "C" int pli_gemm_mxfp4(const void* x8, const float* x_scale, const void* w4, const void* w_exp,
                              const void* bias, void* c, int m, int n, int k, int64_t ldx8, int64_t ldw, int64_t lds,
                              int64_t ldc, int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(dtype == PLI_F16 || dtype == PLI_BF16, "pli_gemm_mxfp4: bad dtype %d (fp16 / bf16 output only)", dtype);
    PLI_REQUIRE(m >= 0 && n >= 0 && k >= 0, "pli_gemm_mxfp4: bad shape m=%d n=%d k=%d", m, n, k);
    PLI_REQUIRE(mxfp4a_shape_ok(k), "pli_gemm_mxfp4: k=%d is not a multiple of the MX block of 32", k);
    PLI_REQUIRE(ldx8 >= k && ldw >= k / 2 && lds >= k / kMxfp4aBlock && ldc >= n,
                "pli_gemm_mxfp4: leading dimension too small (ldx8=%lld ldw=%lld lds=%lld ldc=%lld)", (long long)ldx8,
                (long long)ldw, (long long)lds, (long long)ldc);
    if (m == 0 || n == 0) return PLI_OK;  // empty operands may be NULL
    PLI_REQUIRE(c && (k == 0 || (x8 && w4 && w_exp)), "pli_gemm_mxfp4: null pointer (the scale bytes have no default)");
    PLI_REQUIRE(((int64_t)m * n + 255) / 256 <= 0x7fffffffLL, "pli_gemm_mxfp4: grid too large");
    const Mxfp4aCall call{m, n, k, ldx8, ldw, lds, ldc, (uintptr_t)x8, (uintptr_t)w4, (uintptr_t)w_exp, (uintptr_t)c};
    const Mxfp4aArgs a{x8, w4, w_exp, bias, x_scale, c, m, n, k, ldx8, ldw, lds, ldc};
    hipStream_t s = (hipStream_t)stream;
    if (mxfp4a_route(call) == MXFP4A_MX)
        return dtype == PLI_BF16 ? launch_mx<bf16_t>(a, s) : launch_mx<f16_t>(a, s);
    return dtype == PLI_BF16 ? launch_generic<bf16_t>(a, s) : launch_generic<f16_t>(a, s);
}
