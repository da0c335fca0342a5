// Weight-only fp8 linear (W8A16) for decode batches on gfx950 (MI355X):
//   C[r, j] = round_T( w_scale[j] * sum_i decode(W8[j, i]) * X[r, i]  (+ bias[j]) )
// W8 [n, k] OCP e4m3fn codes, one byte each, one fp32 scale per output row;
// X, C, bias 16-bit (T = bf16 / fp16); fp32 accumulate, one rounding to T.
// A code widens exactly to T (fp8_kv.h), a code x 16-bit product is exact in
// fp32, and the scale is folded in after the sum, so the 16-bit tolerances
// hold against an oracle over the dequantised weights.  The weight stream,
// the byte stream a decode step is bound by, is half of the 16-bit kernels'.
//
// Kernels (index arithmetic and routes: fp8w_plan.h, checked on the CPU by
// tests/host/fp8w_plan_check.cpp):
//   linear_fp8w_vec     VALU, M <= 16 (M = 1 is the GEMV): gemv_vec /
//                       gemm_skinny_nt over 1-byte rows
//   linear_fp8w_smallm  MFMA 16x16x32, 1 < M <= 128: gemm_smallm_nt over
//                       1-byte rows
//   linear_fp8w_generic one thread per output, anything
//   fp8w_widen          codes -> T(decode * scale) into a workspace for the
//                       existing pli_gemm / pli_gemm_swiglu (M > 16 without a
//                       fast route)
// SWIGLU forms stream row j of Wg and of Wu and write silu(sg g) * (su u);
// neither gate nor up is written to memory.
#include "fp8_kv.h"
#include "fp8w_plan.h"
#include "pli_common.h"

namespace pli {
// capi.cpp: put `first` in front of the calling thread's route string
void route_prepend(const char* first);

namespace {

// gemm.hip's silu_mul (the same expression, so the fused SwiGLU forms agree)
__device__ __forceinline__ float silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

// acc + lo(a) * lo(b) + hi(a) * hi(b) of two packed pairs of T, fp32 accumulate: v_dot2_f32_bf16 / v_dot2_f32_f16
// on the pairs as loaded and widened, so neither W nor X is unpacked to fp32 (which cost 25 of the 60 VALU
// instructions per 16-byte chunk of the fma form)
template <typename T> __device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float acc);
template <> __device__ __forceinline__ float dot2<bf16_t>(uint32_t a, uint32_t b, float acc) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a), __builtin_bit_cast(bf16x2, b), acc, false);
}
template <> __device__ __forceinline__ float dot2<f16_t>(uint32_t a, uint32_t b, float acc) {
    typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b), acc, false);
}

// acc += sum of the 8 products of two dwords-of-pairs vectors, pair by pair in element order
template <typename T> __device__ __forceinline__ float dot8(const i32x4& w, const i32x4& x, float acc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int wi = w[i], xi = x[i];  // copy the lanes out first (gemv.hip)
        acc = dot2<T>((uint32_t)wi, (uint32_t)xi, acc);
    }
    return acc;
}

// ---------------------------------------------------------------------------
// linear_fp8w_vec: a wave owns ROWS consecutive W rows (of Wg and Wu when
// SWIGLU); lane l streams the 16-byte chunks l, l + 64, ... of each row
// (non-temporal: W is read once), all NW x ROWS x CPL loads issued before
// the first use.  A chunk is 16 codes; the matching 2 x 16 bytes of every X
// row (L1 / L2 resident) are read once per chunk and reused for the wave's
// rows.  fp32 accumulators, one wave reduction per output.
template <typename T, int NB, int ROWS, int CPL, bool SWIGLU, bool BIAS>
__global__ __launch_bounds__(kFp8wVecWaves * 64) void linear_fp8w_vec(
    const char* __restrict__ X, const char* __restrict__ W, const float* __restrict__ w_scale,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ C, int M, int N, int nchunks, int64_t ldx,
    int64_t ldw, int64_t ldc, const char* __restrict__ Wu, const float* __restrict__ wu_scale, int64_t ldwu) {
    constexpr int NW = SWIGLU ? 2 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row0 = fp8w_vec_row0(blockIdx.x, wave, ROWS);
    if (row0 >= N) return;
    const char* wrow[NW][ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int row = fp8w_vec_row(row0, r, N);
        wrow[0][r] = W + fp8w_vec_w_off(row, 0, ldw);
        if constexpr (SWIGLU) wrow[NW - 1][r] = Wu + fp8w_vec_w_off(row, 0, ldwu);
    }
    float acc[NW][ROWS][NB];
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int bb = 0; bb < NB; ++bb) acc[w][r][bb] = 0.f;

    for (int c0 = 0; c0 < nchunks; c0 += 64 * CPL) {
        i32x4 wv[NW][ROWS][CPL];
#pragma unroll
        for (int u = 0; u < CPL; ++u) {
            const int cc = fp8w_vec_chunk_clamped(fp8w_vec_chunk(c0, lane, u), nchunks);
#pragma unroll
            for (int w = 0; w < NW; ++w)
#pragma unroll
                for (int r = 0; r < ROWS; ++r)
                    wv[w][r][u] =
                        __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wrow[w][r] + (int64_t)cc * 16));
        }
#pragma unroll
        for (int u = 0; u < CPL; ++u) {
            const int cc = fp8w_vec_chunk(c0, lane, u);
            if (cc < nchunks) {
                i32x4 wl[NW][ROWS], wh[NW][ROWS];
#pragma unroll
                for (int w = 0; w < NW; ++w)
#pragma unroll
                    for (int r = 0; r < ROWS; ++r) fp8_widen16<T>(wv[w][r][u], wl[w][r], wh[w][r]);
#pragma unroll
                for (int bb = 0; bb < NB; ++bb) {
                    if (bb < M) {
                        const char* xp = X + fp8w_vec_x_off(bb, cc, ldx) * 2;
                        const i32x4 xl = *reinterpret_cast<const i32x4*>(xp);
                        const i32x4 xh = *reinterpret_cast<const i32x4*>(xp + 16);
#pragma unroll
                        for (int w = 0; w < NW; ++w)
#pragma unroll
                            for (int r = 0; r < ROWS; ++r)
                                acc[w][r][bb] = dot8<T>(wh[w][r], xh, dot8<T>(wl[w][r], xl, acc[w][r][bb]));
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int64_t row = row0 + r;
        if (row >= N) break;  // wave-uniform
        const float sg = fp8_scale_of(w_scale, (int)row);
        float su = 1.f, bn = 0.f;
        if constexpr (SWIGLU) su = fp8_scale_of(wu_scale, (int)row);
        if constexpr (BIAS) bn = elem<T>::to_f32(T{bias[row]});
#pragma unroll
        for (int bb = 0; bb < NB; ++bb) {
            if (bb < M) {
                float v = sg * wave_sum(acc[0][r][bb]);
                if constexpr (SWIGLU) v = silu_mul(v, su * wave_sum(acc[NW - 1][r][bb]));
                if constexpr (BIAS) v += bn;
                if (lane == 0) C[(int64_t)bb * ldc + row] = __builtin_bit_cast(uint16_t, elem<T>::from_f32(v));
            }
        }
    }
}

// ---------------------------------------------------------------------------
// linear_fp8w_smallm: C^T[16 W rows][M] on v_mfma_f32_16x16x32.  One workgroup
// per 16 W rows, K split over its 4 waves, W streamed exactly once (16 codes
// per lane and load: 1 KiB per wave-instruction, U of them issued ahead),
// X fragments from L2, partial C^T tiles summed through LDS in wave order.
// k-permutation (fp8w_plan.h): the lane's 16 codes are k = kb + 0..15 of row
// r16 with kb = wave K/4 + 64 step + 16 (lane >> 4); the lo / hi halves of
// fp8_widen16 are the A operands of two MFMAs, whose B operands are
// X[row][kb + 0..7] and X[row][kb + 8..15] -- 32 contiguous bytes of X.
template <typename T, int NBG, bool SWIGLU, bool BIAS>
__global__ __launch_bounds__(256) void linear_fp8w_smallm(
    const char* __restrict__ X, const char* __restrict__ W, const float* __restrict__ w_scale,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ C, int M, int N, int K, int64_t ldx, int64_t ldw,
    int64_t ldc, const char* __restrict__ Wu, const float* __restrict__ wu_scale, int64_t ldwu) {
    constexpr int NW = SWIGLU ? 2 : 1;
    constexpr int U = SWIGLU ? kFp8wSmallmUnrollSwiglu : kFp8wSmallmUnroll;
    __shared__ __attribute__((aligned(16))) float part[4][NBG][NW][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * 16;
    const int r16 = lane & 15;
    const int kw = fp8w_smallm_kw(K);
    const int wrow = fp8w_smallm_w_row(n0, lane, N);
    const int kb0 = fp8w_smallm_k(wave, kw, 0, lane);
    const char* wp[NW];
    wp[0] = W + fp8w_smallm_w_off(wrow, kb0, ldw);
    if constexpr (SWIGLU) wp[NW - 1] = Wu + fp8w_smallm_w_off(wrow, kb0, ldwu);
    const char* xp[NBG];
#pragma unroll
    for (int gi = 0; gi < NBG; ++gi) xp[gi] = X + fp8w_smallm_x_off(fp8w_smallm_x_row(gi, lane, M), kb0, 0, ldx) * 2;
    f32x4 acc[NW][NBG];
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int gi = 0; gi < NBG; ++gi) acc[w][gi] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int steps = kw / kFp8wSmallmWaveStep;
    int s = 0;
    for (; s + U <= steps; s += U) {
        i32x4 wf[NW][U];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int w = 0; w < NW; ++w)
                wf[w][u] = __builtin_nontemporal_load(
                    reinterpret_cast<const i32x4*>(wp[w] + (s + u) * kFp8wSmallmWaveStep));
#pragma unroll
        for (int u = 0; u < U; ++u) {
            i32x4 xl[NBG], xh[NBG];
#pragma unroll
            for (int gi = 0; gi < NBG; ++gi) {
                xl[gi] = *reinterpret_cast<const i32x4*>(xp[gi] + (s + u) * kFp8wSmallmWaveStep * 2);
                xh[gi] = *reinterpret_cast<const i32x4*>(xp[gi] + (s + u) * kFp8wSmallmWaveStep * 2 + 16);
            }
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                i32x4 lo, hi;
                fp8_widen16<T>(wf[w][u], lo, hi);
#pragma unroll
                for (int gi = 0; gi < NBG; ++gi) {
                    acc[w][gi] = mfma16x16x32<T>(lo, xl[gi], acc[w][gi]);
                    acc[w][gi] = mfma16x16x32<T>(hi, xh[gi], acc[w][gi]);
                }
            }
        }
    }
    for (; s < steps; ++s) {  // remainder steps
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const i32x4 wf =
                __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp[w] + s * kFp8wSmallmWaveStep));
            i32x4 lo, hi;
            fp8_widen16<T>(wf, lo, hi);
#pragma unroll
            for (int gi = 0; gi < NBG; ++gi) {
                const char* xq = xp[gi] + s * kFp8wSmallmWaveStep * 2;
                acc[w][gi] = mfma16x16x32<T>(lo, *reinterpret_cast<const i32x4*>(xq), acc[w][gi]);
                acc[w][gi] = mfma16x16x32<T>(hi, *reinterpret_cast<const i32x4*>(xq + 16), acc[w][gi]);
            }
        }
    }
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int gi = 0; gi < NBG; ++gi)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[wave][gi][w][r][lane] = acc[w][gi][r];
    __syncthreads();
    // wave w reduces batch groups gi = w, w + 4, ...; lane: column = batch row, rows 4q .. 4q+3 = W rows
    for (int gi = wave; gi < NBG; gi += 4) {
        const int bt = gi * 16 + r16;
        const int nr = n0 + 4 * (lane >> 4);
        if (bt < M && nr < N) {  // N % 16 == 0: nr + 3 < N
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = part[0][gi][0][r][lane] + part[1][gi][0][r][lane] + part[2][gi][0][r][lane] +
                       part[3][gi][0][r][lane];
                v[r] *= fp8_scale_of(w_scale, nr + r);
                if constexpr (SWIGLU)
                    v[r] = silu_mul(v[r], fp8_scale_of(wu_scale, nr + r) *
                                              (part[0][gi][NW - 1][r][lane] + part[1][gi][NW - 1][r][lane] +
                                               part[2][gi][NW - 1][r][lane] + part[3][gi][NW - 1][r][lane]));
                if constexpr (BIAS) v[r] += elem<T>::to_f32(T{bias[nr + r]});
            }
            *reinterpret_cast<i32x2*>(C + (int64_t)bt * ldc + nr) =
                i32x2{(int)pack2<T>(v[0], v[1]), (int)pack2<T>(v[2], v[3])};
        }
    }
}

// ---------------------------------------------------------------------------
// linear_fp8w_generic: one thread per output, any M / N / K / ld / alignment,
// K = 0 (bias or 0).  Decodes with the header codec; fp32 fma in k order.
template <typename T, bool SWIGLU>
__global__ __launch_bounds__(256) void linear_fp8w_generic(
    const T* __restrict__ X, const uint8_t* __restrict__ W, const float* __restrict__ w_scale,
    const T* __restrict__ bias, T* __restrict__ C, int M, int N, int K, int64_t ldx, int64_t ldw, int64_t ldc,
    const uint8_t* __restrict__ Wu, const float* __restrict__ wu_scale, int64_t ldwu) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)M * N) return;
    const int r = (int)(i / N), j = (int)(i % N);
    const T* x = X + (int64_t)r * ldx;
    const uint8_t* w = W + (int64_t)j * ldw;
    float g = 0.f, u = 0.f;
    for (int kk = 0; kk < K; ++kk) {
        const float xv = elem<T>::to_f32(x[kk]);
        g = fmaf(fp8_e4m3_decode(w[kk]), xv, g);
        if constexpr (SWIGLU) u = fmaf(fp8_e4m3_decode(Wu[(int64_t)j * ldwu + kk]), xv, u);
    }
    float v = fp8_scale_of(w_scale, j) * g;
    if constexpr (SWIGLU) v = silu_mul(v, fp8_scale_of(wu_scale, j) * u);
    if (bias) v += elem<T>::to_f32(bias[j]);
    C[(int64_t)r * ldc + j] = elem<T>::from_f32(v);
}

// ---------------------------------------------------------------------------
// fp8w_widen: out[j][i] = T( float(decode(W[j][i])) * w_scale[j] ), out
// contiguous [n][k]: one fp32 multiply, one round-to-nearest-even (bitwise
// torch's (codes.float() * scale[:, None]).to(T)).  VEC: one thread per 16
// codes (k, ldw multiples of 16, W 16-byte aligned), else one per element.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void fp8w_widen(const uint8_t* __restrict__ W, const float* __restrict__ w_scale,
                                                  uint16_t* __restrict__ out, int N, int K, int64_t ldw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if constexpr (VEC) {
        const int cpr = K / 16;  // chunks per row
        if (i >= (int64_t)N * cpr) return;
        const int j = (int)(i / cpr), c = (int)(i % cpr);
        const float sc = fp8_scale_of(w_scale, j);
        i32x4 lo, hi;
        fp8_widen16<T>(*reinterpret_cast<const i32x4*>(W + (int64_t)j * ldw + (int64_t)c * 16), lo, hi);
        i32x4 o[2];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t p = (uint32_t)(h ? hi[e] : lo[e]);
                o[h][e] = (int)pack2<T>(elem<T>::to_f32(T{(uint16_t)(p & 0xffffu)}) * sc,
                                        elem<T>::to_f32(T{(uint16_t)(p >> 16)}) * sc);
            }
        i32x4* dst = reinterpret_cast<i32x4*>(out + (int64_t)j * K + (int64_t)c * 16);
        dst[0] = o[0];
        dst[1] = o[1];
    } else {
        if (i >= (int64_t)N * K) return;
        const int j = (int)(i / K), c = (int)(i % K);
        const float v = fp8_e4m3_decode(W[(int64_t)j * ldw + c]) * fp8_scale_of(w_scale, j);
        out[i] = __builtin_bit_cast(uint16_t, elem<T>::from_f32(v));
    }
}

// ------------------------------------------------------------------ launch --
struct Fp8wArgs {
    const void *x, *w, *bias, *wu;
    const float *w_scale, *wu_scale;
    void* c;
    int m, n, k;
    int64_t ldx, ldw, ldwu, ldc;
    bool swiglu;
};

template <typename T, int NB, int ROWS, int CPL, bool SWIGLU>
int launch_vec_cfg(const Fp8wArgs& a, hipStream_t s) {
    const dim3 grid(fp8w_vec_grid(a.n, ROWS)), block(kFp8wVecWaves * 64);
    const int nch = a.k / kFp8wChunk;
#define PLI_FP8W_VEC(BIAS)                                                                                     \
    hipLaunchKernelGGL((linear_fp8w_vec<T, NB, ROWS, CPL, SWIGLU, BIAS>), grid, block, 0, s, (const char*)a.x, \
                       (const char*)a.w, a.w_scale, (const uint16_t*)a.bias, (uint16_t*)a.c, a.m, a.n, nch,    \
                       a.ldx, a.ldw, a.ldc, (const char*)a.wu, a.wu_scale, a.ldwu)
    if constexpr (SWIGLU) {
        PLI_FP8W_VEC(false);
        return launch_status("linear_fp8w_vec<swiglu>");
    } else {
        if (a.bias) PLI_FP8W_VEC(true);
        else PLI_FP8W_VEC(false);
        return launch_status("linear_fp8w_vec");
    }
#undef PLI_FP8W_VEC
}

template <typename T, int NB, bool SWIGLU>
int launch_vec_nb(const Fp8wArgs& a, hipStream_t s) {
    const Fp8wVecCfg c = fp8w_vec_cfg(a.k, SWIGLU);
    if constexpr (SWIGLU) {
        if (c.rows == 2 && c.cpl == 2) return launch_vec_cfg<T, NB, 2, 2, true>(a, s);
        return launch_vec_cfg<T, NB, 1, 4, true>(a, s);
    } else {
        if (c.rows == 4 && c.cpl == 2) return launch_vec_cfg<T, NB, 4, 2, false>(a, s);
        return launch_vec_cfg<T, NB, 2, 4, false>(a, s);
    }
}

template <typename T, bool SWIGLU>
int launch_vec(const Fp8wArgs& a, hipStream_t s) {
    if (a.m <= 1) return launch_vec_nb<T, 1, SWIGLU>(a, s);
    if (a.m <= 2) return launch_vec_nb<T, 2, SWIGLU>(a, s);
    if (a.m <= 4) return launch_vec_nb<T, 4, SWIGLU>(a, s);
    if (a.m <= 8) return launch_vec_nb<T, 8, SWIGLU>(a, s);
    return launch_vec_nb<T, 16, SWIGLU>(a, s);
}

template <typename T, int NBG, bool SWIGLU>
int launch_smallm_nbg(const Fp8wArgs& a, hipStream_t s) {
    const dim3 grid(a.n / 16), block(256);
#define PLI_FP8W_SMALLM(BIAS)                                                                                   \
    hipLaunchKernelGGL((linear_fp8w_smallm<T, NBG, SWIGLU, BIAS>), grid, block, 0, s, (const char*)a.x,         \
                       (const char*)a.w, a.w_scale, (const uint16_t*)a.bias, (uint16_t*)a.c, a.m, a.n, a.k,     \
                       a.ldx, a.ldw, a.ldc, (const char*)a.wu, a.wu_scale, a.ldwu)
    if constexpr (SWIGLU) {
        PLI_FP8W_SMALLM(false);
        return launch_status("linear_fp8w_smallm<swiglu>");
    } else {
        if (a.bias) PLI_FP8W_SMALLM(true);
        else PLI_FP8W_SMALLM(false);
        return launch_status("linear_fp8w_smallm");
    }
#undef PLI_FP8W_SMALLM
}

template <typename T, bool SWIGLU>
int launch_smallm(const Fp8wArgs& a, hipStream_t s) {
    switch (fp8w_smallm_nbg(a.m)) {
        case 1: return launch_smallm_nbg<T, 1, SWIGLU>(a, s);
        case 2: return launch_smallm_nbg<T, 2, SWIGLU>(a, s);
        case 4: return launch_smallm_nbg<T, 4, SWIGLU>(a, s);
        default: return launch_smallm_nbg<T, 8, SWIGLU>(a, s);
    }
}

template <typename T, bool SWIGLU>
int launch_generic(const Fp8wArgs& a, hipStream_t s) {
    const int64_t blocks = ((int64_t)a.m * a.n + 255) / 256;
    hipLaunchKernelGGL((linear_fp8w_generic<T, SWIGLU>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)a.x,
                       (const uint8_t*)a.w, a.w_scale, (const T*)a.bias, (T*)a.c, a.m, a.n, a.k, a.ldx, a.ldw,
                       a.ldc, (const uint8_t*)a.wu, a.wu_scale, a.ldwu);
    return launch_status(SWIGLU ? "linear_fp8w_generic<swiglu>" : "linear_fp8w_generic");
}

template <typename T>
int launch_widen(const void* w, const float* scale, void* out, int n, int k, int64_t ldw, hipStream_t s) {
    const bool vec = k % 16 == 0 && ldw % 16 == 0 && aligned16(w);
    const int64_t items = vec ? (int64_t)n * (k / 16) : (int64_t)n * k;
    const dim3 grid((unsigned)((items + 255) / 256)), block(256);
    if (vec)
        hipLaunchKernelGGL((fp8w_widen<T, true>), grid, block, 0, s, (const uint8_t*)w, scale, (uint16_t*)out, n, k,
                           ldw);
    else
        hipLaunchKernelGGL((fp8w_widen<T, false>), grid, block, 0, s, (const uint8_t*)w, scale, (uint16_t*)out, n,
                           k, ldw);
    return launch_status("fp8w_widen");
}

template <typename T, bool SWIGLU>
int run_route(int route, const Fp8wArgs& a, hipStream_t s) {
    switch (route) {
        case FP8W_SMALLM: return launch_smallm<T, SWIGLU>(a, s);
        case FP8W_VEC: return launch_vec<T, SWIGLU>(a, s);
        default: return launch_generic<T, SWIGLU>(a, s);
    }
}

// argument checks, route, launch.  `what` names the entry point in messages.
int dispatch(const char* what, const Fp8wArgs& a, int dtype, void* ws, size_t ws_bytes, void* stream) {
    clear_error();
    PLI_REQUIRE(a.m >= 0 && a.n >= 0 && a.k >= 0, "%s: bad shape m=%d n=%d k=%d", what, a.m, a.n, a.k);
    PLI_REQUIRE(dtype == PLI_F16 || dtype == PLI_BF16, "%s: bad dtype %d (fp16 / bf16 activations only)", what, dtype);
    PLI_REQUIRE(a.ldx >= a.k && a.ldw >= a.k && a.ldc >= a.n && (!a.swiglu || a.ldwu >= a.k),
                "%s: leading dimension too small (ldx=%lld ldw=%lld ldwu=%lld ldc=%lld)", what, (long long)a.ldx,
                (long long)a.ldw, (long long)a.ldwu, (long long)a.ldc);
    if (a.m == 0 || a.n == 0) return PLI_OK;  // empty operands may be NULL
    PLI_REQUIRE(a.c && (a.k == 0 || (a.x && a.w && (!a.swiglu || a.wu))), "%s: null pointer", what);
    PLI_REQUIRE(((int64_t)a.m * a.n + 255) / 256 <= 0x7fffffffLL, "%s: grid too large", what);
    const Fp8wCall call{a.m, a.n, a.k, a.ldx, a.ldw | (a.swiglu ? a.ldwu : 0), a.ldc,
                        (uintptr_t)a.w | (a.swiglu ? (uintptr_t)a.wu : 0), (uintptr_t)a.x, (uintptr_t)a.c,
                        (uintptr_t)a.bias, (uintptr_t)ws, ws_bytes, a.swiglu};
    const int route = fp8w_route(call);
    PLI_REQUIRE(route != FP8W_BAD_WORKSPACE,
                "%s: workspace must be 16-byte aligned and hold %zu bytes (got %zu at %p)", what,
                fp8w_workspace_need(a.n, a.k, a.swiglu), ws_bytes, ws);
    hipStream_t s = (hipStream_t)stream;
    if (route == FP8W_WIDEN) {
        // the widened weight(s), contiguous [n][k] of T, then the 16-bit GEMM
        char* wsg = (char*)ws;
        char* wsu = wsg + fp8w_widened_bytes(a.n, a.k);
        int rc = dtype == PLI_BF16 ? launch_widen<bf16_t>(a.w, a.w_scale, wsg, a.n, a.k, a.ldw, s)
                                   : launch_widen<f16_t>(a.w, a.w_scale, wsg, a.n, a.k, a.ldw, s);
        if (rc != PLI_OK) return rc;
        if (a.swiglu) {
            rc = dtype == PLI_BF16 ? launch_widen<bf16_t>(a.wu, a.wu_scale, wsu, a.n, a.k, a.ldwu, s)
                                   : launch_widen<f16_t>(a.wu, a.wu_scale, wsu, a.n, a.k, a.ldwu, s);
            if (rc != PLI_OK) return rc;
            rc = pli_gemm_swiglu(a.x, wsg, wsu, a.c, a.m, a.n, a.k, a.ldx, a.k, a.k, a.ldc, dtype, stream);
            if (rc == PLI_OK) route_prepend("fp8w_widen+fp8w_widen");
            return rc;
        }
        rc = pli_gemm(a.x, wsg, a.c, a.bias, a.m, a.n, a.k, a.ldx, a.k, a.ldc, 1, dtype, stream);
        if (rc == PLI_OK) route_prepend("fp8w_widen");  // pli_gemm started the route string anew
        return rc;
    }
    const int r = (a.k == 0) ? FP8W_GENERIC : route;
    if (a.swiglu)
        return dtype == PLI_BF16 ? run_route<bf16_t, true>(r, a, s) : run_route<f16_t, true>(r, a, s);
    return dtype == PLI_BF16 ? run_route<bf16_t, false>(r, a, s) : run_route<f16_t, false>(r, a, s);
}

}  // namespace
}  // namespace pli

extern "C" size_t pli_linear_fp8w_workspace_size(int m, int n, int k, int dtype) {
    if (dtype != PLI_BF16 && dtype != PLI_F16) return 0;
    return pli::fp8w_workspace_size(m, n, k, false);
}

extern "C" size_t pli_linear_swiglu_fp8w_workspace_size(int m, int n, int k, int dtype) {
    if (dtype != PLI_BF16 && dtype != PLI_F16) return 0;
    return pli::fp8w_workspace_size(m, n, k, true);
}

extern "C" int pli_linear_fp8w(const void* x, const void* w8, const float* w_scale, const void* bias, void* c, int m,
                               int n, int k, int64_t ldx, int64_t ldw, int64_t ldc, int dtype, void* workspace,
                               size_t workspace_bytes, void* stream) {
    const pli::Fp8wArgs a{x, w8, bias, nullptr, w_scale, nullptr, c, m, n, k, ldx, ldw, 0, ldc, false};
    return pli::dispatch("pli_linear_fp8w", a, dtype, workspace, workspace_bytes, stream);
}

// y = W8 x: pli_linear_fp8w with one X row and no bias, on the same kernel
extern "C" int pli_gemv_fp8w(const void* w8, const float* w_scale, const void* x, void* y, int m, int k, int64_t ldw,
                             int dtype, void* stream) {
    const pli::Fp8wArgs a{x, w8, nullptr, nullptr, w_scale, nullptr, y, 1, m, k, k, ldw, 0, m, false};
    return pli::dispatch("pli_gemv_fp8w", a, dtype, nullptr, 0, stream);
}

extern "C" int pli_linear_swiglu_fp8w(const void* x, const void* wg8, const float* wg_scale, const void* wu8,
                                      const float* wu_scale, void* h, int m, int n, int k, int64_t ldx,
                                      int64_t ldwg, int64_t ldwu, int64_t ldh, int dtype, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    const pli::Fp8wArgs a{x, wg8, nullptr, wu8, wg_scale, wu_scale, h, m, n, k, ldx, ldwg, ldwu, ldh, true};
    return pli::dispatch("pli_linear_swiglu_fp8w", a, dtype, workspace, workspace_bytes, stream);
}
