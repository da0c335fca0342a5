// fp8 e4m3 activations on gfx950 (MI355X): the row quantiser and the W8A8 GEMM
//   C[r, j] = round_T( x_scale[r] * w_scale[j] * sum_i decode(X8[r, i]) * decode(W8[j, i])  (+ bias[j]) )
// X8 [m, k], W8 [n, k] OCP e4m3fn codes, one byte each; one fp32 scale per X
// row and per W row, both read on the device; C, bias 16-bit (T = bf16 /
// fp16).  A code x code product has at most 8 significant bits, so it is exact
// in fp32; the sum is fp32; both scales and the bias are folded in after the
// sum and the result is rounded once.
//
// Kernels (index arithmetic and routes: fp8a_plan.h, checked on the CPU by
// tests/host/fp8a_plan_check.cpp):
//   quant_rows_fp8    x [m, k] 16-bit -> codes + one scale per row, the rule
//                     of pli_hip.quantize_weight_fp8 per row
//   gemm_fp8_mx       128 x 128 tile, codes staged HBM -> LDS by 16-byte
//                     LDS-DMA into a swizzled image (two stages), multiplied
//                     by v_mfma_scale_f32_32x32x64_f8f6f4 with both E8M0
//                     scales at 2^0: twice the bf16 MFMA rate per clock
//   gemm_fp8_generic  one thread per output through the header codec, anything
#include "fp8_kv.h"
#include "fp8a_plan.h"
#include "pli_common.h"

namespace pli {
namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// ---------------------------------------------------------------------------
// quant_rows_fp8.  scale = absmax / 448 over the row's finite elements (1.0
// when there is none that is non-zero), inv = 1.0f / scale, code =
// e4m3fn(clamp(x * inv, +-448)).  A NaN gets 0x7F, an infinity the code of
// +-448 (the clamp), and neither enters the absmax.
__device__ __forceinline__ float quant_abs_finite(float x) {
    const float a = fabsf(x);
    return a < __builtin_inff() ? a : 0.f;  // false for NaN and inf
}
// a NaN of either sign -> the positive quiet NaN, which fp8_encode4 turns into 0x7F
__device__ __forceinline__ float quant_pos_nan(float x) { return x != x ? __uint_as_float(0x7fc00000u) : x; }

template <typename T> __device__ __forceinline__ void quant_unpack8(i32x4 v, float (&x)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[2 * i] = elem<T>::to_f32(T{(uint16_t)((uint32_t)v[i] & 0xffffu)});
        x[2 * i + 1] = elem<T>::to_f32(T{(uint16_t)((uint32_t)v[i] >> 16)});
    }
}
template <typename T> __device__ __forceinline__ float quant_absmax8(i32x4 v, float amax) {
    float x[8];
    quant_unpack8<T>(v, x);
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, quant_abs_finite(x[i]));
    return amax;
}
template <typename T> __device__ __forceinline__ i32x2 quant_encode8(i32x4 v, float inv) {
    float x[8];
    quant_unpack8<T>(v, x);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = quant_pos_nan(x[i]);
    return i32x2{(int)fp8_encode4(x[0], x[1], x[2], x[3], inv), (int)fp8_encode4(x[4], x[5], x[6], x[7], inv)};
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kFp8aQuantThreads) void quant_rows_fp8(const uint16_t* __restrict__ X, int64_t ldx,
                                                                   uint8_t* __restrict__ X8, int64_t ldx8,
                                                                   float* __restrict__ x_scale, int K) {
    __shared__ float part[kFp8aQuantThreads / 64];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const uint16_t* x = X + row * ldx;
    uint8_t* x8 = X8 + row * ldx8;
    const int items = VEC ? K / 8 : K;
    const int trips = fp8a_quant_trips(items);
    float amax = 0.f;
    i32x4 held[kFp8aQuantHeld];
    if constexpr (VEC) {
#pragma unroll
        for (int u = 0; u < kFp8aQuantHeld; ++u) {
            const int c = fp8a_quant_item(tid, u);
            held[u] = i32x4{0, 0, 0, 0};
            if (c < items) {
                held[u] = *reinterpret_cast<const i32x4*>(x + (int64_t)c * 8);
                amax = quant_absmax8<T>(held[u], amax);
            }
        }
        for (int u = kFp8aQuantHeld; u < trips; ++u) {
            const int c = fp8a_quant_item(tid, u);
            if (c < items) amax = quant_absmax8<T>(*reinterpret_cast<const i32x4*>(x + (int64_t)c * 8), amax);
        }
    } else {
        for (int u = 0; u < trips; ++u) {
            const int e = fp8a_quant_item(tid, u);
            if (e < items) amax = fmaxf(amax, quant_abs_finite(elem<T>::to_f32(T{x[e]})));
        }
    }
    amax = wave_max(amax);
    if ((tid & 63) == 0) part[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
    const float scale = amax > 0.f ? amax / 448.f : 1.f;
    const float inv = 1.0f / scale;
    if (tid == 0) x_scale[row] = scale;
    if constexpr (VEC) {
#pragma unroll
        for (int u = 0; u < kFp8aQuantHeld; ++u) {
            const int c = fp8a_quant_item(tid, u);
            if (c < items) *reinterpret_cast<i32x2*>(x8 + (int64_t)c * 8) = quant_encode8<T>(held[u], inv);
        }
        for (int u = kFp8aQuantHeld; u < trips; ++u) {
            const int c = fp8a_quant_item(tid, u);
            if (c < items)
                *reinterpret_cast<i32x2*>(x8 + (int64_t)c * 8) =
                    quant_encode8<T>(*reinterpret_cast<const i32x4*>(x + (int64_t)c * 8), inv);
        }
    } else {
        for (int u = 0; u < trips; ++u) {
            const int e = fp8a_quant_item(tid, u);
            if (e < items) {
                const float v = quant_pos_nan(elem<T>::to_f32(T{x[e]}));
                x8[e] = (uint8_t)(fp8_encode4(v, 0.f, 0.f, 0.f, inv) & 0xffu);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// The shared epilogue expression: the two kernels agree bit for bit wherever
// their sums do.
__device__ __forceinline__ float fp8a_finish(float sum, float xs, float ws) { return sum * (xs * ws); }

// ---------------------------------------------------------------------------
// gemm_fp8_mx: C^T tile [128 n][128 m] = W8 tile x X8 tile^T.  Per K-step of
// 128 codes every wave LDS-DMAs 4 KiB of each operand image (4 pieces of 8
// rows x 128 bytes, the XOR swizzle of fp8a_plan.h on the source address) into
// stage (s + 1) % 2 while the MFMAs run on stage s % 2: one barrier per step.
// A wave multiplies its 64 x 64 block as 2 x 2 tiles of 32 x 32, two k-halves
// of 64 codes each: 8 scaled MFMAs per step, operands by ds_read_b128.
template <typename T, bool BIAS>
__global__ __launch_bounds__(256) void gemm_fp8_mx(const uint8_t* __restrict__ X8, const float* __restrict__ x_scale,
                                                   const uint8_t* __restrict__ W8, const float* __restrict__ w_scale,
                                                   const uint16_t* __restrict__ bias, uint16_t* __restrict__ C, int M,
                                                   int N, int K, int64_t ldx8, int64_t ldw, int64_t ldc, int tiles_m,
                                                   int tiles_n) {
    __shared__ __attribute__((aligned(1024))) char smem[kFp8aLdsBytes];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave & 1, wm = wave >> 1;
    const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    const int m0 = fp8a_tile_m(t, tiles_m, tiles_n) * kFp8aTM, n0 = fp8a_tile_n(t, tiles_m, tiles_n) * kFp8aTN;
    const int ks = K / kFp8aKStep;

    // per-lane source offsets of the wave's pieces at K-step 0 (step s: + 128 s)
    int64_t woff[kFp8aPiecesPerWave], xoff[kFp8aPiecesPerWave];
#pragma unroll
    for (int i = 0; i < kFp8aPiecesPerWave; ++i) {
        const int p = fp8a_stage_piece(wave, i);
        const int row = fp8a_stage_row(p, lane), c = fp8a_stage_chunk(p, lane);
        woff[i] = fp8a_src_off(n0, row, N, ldw, 0, c);
        xoff[i] = fp8a_src_off(m0, row, M, ldx8, 0, c);
    }
    auto stage = [&](int s) __attribute__((always_inline)) {
        char* img = smem + (s % kFp8aStages) * kFp8aStageBytes;
#pragma unroll
        for (int i = 0; i < kFp8aPiecesPerWave; ++i) {
            // the LDS address is the wave's piece base: the hardware adds 16 x lane
            const int lds = fp8a_stage_lds(fp8a_stage_piece(wave, i), 0);
            __builtin_amdgcn_global_load_lds(W8 + woff[i] + (int64_t)s * kFp8aKStep, (lds_void*)(img + lds), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(X8 + xoff[i] + (int64_t)s * kFp8aKStep,
                                             (lds_void*)(img + kFp8aImgBytes + lds), 16, 0, 0);
        }
    };

    // fragment read offsets inside a stage: [operand tile][k-half][16-byte half]
    int wrd[2][2][2], xrd[2][2][2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                wrd[tt][s][h] = fp8a_frag_lds(fp8a_frag_row(wn, tt, lane), fp8a_frag_chunk(s, lane, h));
                xrd[tt][s][h] = kFp8aImgBytes + fp8a_frag_lds(fp8a_frag_row(wm, tt, lane), fp8a_frag_chunk(s, lane, h));
            }

    f32x16 acc[2][2];  // [nt][mt]
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nt][mt][r] = 0.f;

    stage(0);
    for (int s = 0; s < ks; ++s) {
        // step s has landed (this wave's pieces; the barrier covers the others'), and every wave is done
        // reading the stage that step s + 1 overwrites
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (s + 1 < ks) stage(s + 1);
        const char* img = smem + (s % kFp8aStages) * kFp8aStageBytes;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            i32x8 wf[2], xf[2];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const i32x4 wl = lds_read_b128(img, wrd[tt][kh][0]), wh = lds_read_b128(img, wrd[tt][kh][1]);
                const i32x4 xl = lds_read_b128(img, xrd[tt][kh][0]), xh = lds_read_b128(img, xrd[tt][kh][1]);
                wf[tt] = i32x8{wl.x, wl.y, wl.z, wl.w, wh.x, wh.y, wh.z, wh.w};
                xf[tt] = i32x8{xl.x, xl.y, xl.z, xl.w, xh.x, xh.y, xh.z, xh.w};
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    // cbsz = blgp = 0: e4m3 x e4m3; E8M0 scale byte 127 = 2^0 for both operands
                    acc[nt][mt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[nt], xf[mt], acc[nt][mt], 0, 0, 0,
                                                                                   127, 0, 127);
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
                    v[r] = fp8a_finish(acc[nt][mt][4 * g + r], xs, fp8_scale_of(w_scale, ncol + r));
                    if constexpr (BIAS) v[r] += elem<T>::to_f32(T{bias[ncol + r]});
                }
                *reinterpret_cast<i32x2*>(C + (int64_t)mrow * ldc + ncol) =
                    i32x2{(int)pack2<T>(v[0], v[1]), (int)pack2<T>(v[2], v[3])};
            }
    }
}

// ---------------------------------------------------------------------------
// gemm_fp8_generic: one thread per output, any M / N / K / ld / alignment,
// K = 0 (bias or 0).  Decodes with the header codec; fp32 fma in k order.
template <typename T>
__global__ __launch_bounds__(256) void gemm_fp8_generic(const uint8_t* __restrict__ X8,
                                                        const float* __restrict__ x_scale,
                                                        const uint8_t* __restrict__ W8,
                                                        const float* __restrict__ w_scale, const T* __restrict__ bias,
                                                        T* __restrict__ C, int M, int N, int K, int64_t ldx8,
                                                        int64_t ldw, int64_t ldc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)M * N) return;
    const int r = (int)(i / N), j = (int)(i % N);
    const uint8_t* x = X8 + (int64_t)r * ldx8;
    const uint8_t* w = W8 + (int64_t)j * ldw;
    float sum = 0.f;
    for (int kk = 0; kk < K; ++kk) sum = fmaf(fp8_e4m3_decode(x[kk]), fp8_e4m3_decode(w[kk]), sum);
    float v = fp8a_finish(sum, fp8_scale_of(x_scale, r), fp8_scale_of(w_scale, j));
    if (bias) v += elem<T>::to_f32(bias[j]);
    C[(int64_t)r * ldc + j] = elem<T>::from_f32(v);
}

// ------------------------------------------------------------------ launch --
struct Fp8aArgs {
    const void *x8, *w8, *bias;
    const float *x_scale, *w_scale;
    void* c;
    int m, n, k;
    int64_t ldx8, ldw, ldc;
};

template <typename T>
int launch_mx(const Fp8aArgs& a, hipStream_t s) {
    const int tiles_m = fp8a_tiles(a.m, kFp8aTM), tiles_n = fp8a_tiles(a.n, kFp8aTN);
    const int nblocks = tiles_m * tiles_n;
#define PLI_FP8A_MX(BIAS)                                                                                        \
    hipLaunchKernelGGL((gemm_fp8_mx<T, BIAS>), dim3(nblocks), dim3(256), 0, s, (const uint8_t*)a.x8, a.x_scale,  \
                       (const uint8_t*)a.w8, a.w_scale, (const uint16_t*)a.bias, (uint16_t*)a.c, a.m, a.n, a.k,  \
                       a.ldx8, a.ldw, a.ldc, tiles_m, tiles_n)
    if (a.bias) PLI_FP8A_MX(true);
    else PLI_FP8A_MX(false);
#undef PLI_FP8A_MX
    return launch_status("gemm_fp8_mx");
}

template <typename T>
int launch_generic(const Fp8aArgs& a, hipStream_t s) {
    const int64_t blocks = ((int64_t)a.m * a.n + 255) / 256;
    hipLaunchKernelGGL((gemm_fp8_generic<T>), dim3((unsigned)blocks), dim3(256), 0, s, (const uint8_t*)a.x8,
                       a.x_scale, (const uint8_t*)a.w8, a.w_scale, (const T*)a.bias, (T*)a.c, a.m, a.n, a.k, a.ldx8,
                       a.ldw, a.ldc);
    return launch_status("gemm_fp8_generic");
}

template <typename T>
int launch_quant(const void* x, int64_t ldx, void* x8, int64_t ldx8, float* x_scale, int m, int k, hipStream_t s) {
    const bool vec = fp8a_quant_vec(k, ldx, ldx8, (uintptr_t)x, (uintptr_t)x8);
    if (vec)
        hipLaunchKernelGGL((quant_rows_fp8<T, true>), dim3(m), dim3(kFp8aQuantThreads), 0, s, (const uint16_t*)x, ldx,
                           (uint8_t*)x8, ldx8, x_scale, k);
    else
        hipLaunchKernelGGL((quant_rows_fp8<T, false>), dim3(m), dim3(kFp8aQuantThreads), 0, s, (const uint16_t*)x, ldx,
                           (uint8_t*)x8, ldx8, x_scale, k);
    return launch_status("quant_rows_fp8");
}

}  // namespace
}  // namespace pli

extern "C" int pli_quantize_rows_fp8(const void* x, int64_t ldx, void* x8, int64_t ldx8, float* x_scale, int m, int k,
                                     int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(dtype == PLI_F16 || dtype == PLI_BF16, "pli_quantize_rows_fp8: bad dtype %d (fp16 / bf16 rows only)",
                dtype);
    PLI_REQUIRE(m >= 0 && k >= 0, "pli_quantize_rows_fp8: bad shape m=%d k=%d", m, k);
    PLI_REQUIRE(ldx >= k && ldx8 >= k, "pli_quantize_rows_fp8: leading dimension too small (ldx=%lld ldx8=%lld)",
                (long long)ldx, (long long)ldx8);
    if (m == 0) return PLI_OK;  // empty operands may be NULL
    PLI_REQUIRE(x_scale && (k == 0 || (x && x8)), "pli_quantize_rows_fp8: null pointer");
    // k == 0: the kernel reads and writes no element and stores scale 1.0
    return dtype == PLI_BF16 ? launch_quant<bf16_t>(x, ldx, x8, ldx8, x_scale, m, k, (hipStream_t)stream)
                             : launch_quant<f16_t>(x, ldx, x8, ldx8, x_scale, m, k, (hipStream_t)stream);
}

extern "C" int pli_gemm_fp8(const void* x8, const float* x_scale, const void* w8, const float* w_scale,
                            const void* bias, void* c, int m, int n, int k, int64_t ldx8, int64_t ldw, int64_t ldc,
                            int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(dtype == PLI_F16 || dtype == PLI_BF16, "pli_gemm_fp8: bad dtype %d (fp16 / bf16 output only)", dtype);
    PLI_REQUIRE(m >= 0 && n >= 0 && k >= 0, "pli_gemm_fp8: bad shape m=%d n=%d k=%d", m, n, k);
    PLI_REQUIRE(ldx8 >= k && ldw >= k && ldc >= n,
                "pli_gemm_fp8: leading dimension too small (ldx8=%lld ldw=%lld ldc=%lld)", (long long)ldx8,
                (long long)ldw, (long long)ldc);
    if (m == 0 || n == 0) return PLI_OK;  // empty operands may be NULL
    PLI_REQUIRE(c && (k == 0 || (x8 && w8)), "pli_gemm_fp8: null pointer");
    PLI_REQUIRE(((int64_t)m * n + 255) / 256 <= 0x7fffffffLL, "pli_gemm_fp8: grid too large");
    const Fp8aCall call{m, n, k, ldx8, ldw, ldc, (uintptr_t)x8, (uintptr_t)w8, (uintptr_t)c};
    const Fp8aArgs a{x8, w8, bias, x_scale, w_scale, c, m, n, k, ldx8, ldw, ldc};
    hipStream_t s = (hipStream_t)stream;
    if (fp8a_route(call) == FP8A_MX)
        return dtype == PLI_BF16 ? launch_mx<bf16_t>(a, s) : launch_mx<f16_t>(a, s);
    return dtype == PLI_BF16 ? launch_generic<bf16_t>(a, s) : launch_generic<f16_t>(a, s);
}
