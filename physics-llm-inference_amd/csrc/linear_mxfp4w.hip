// Weight-only MXFP4 linear (W4A16) for decode batches on gfx950 (MI355X):
//   C[r, j] = round_T( sum_i decode(w4[j, i]) * 2^(w_exp[j, i / 32] - 127) * X[r, i]  (+ bias[j]) )
// w4 [n, k / 2] bytes of two OCP e2m1 codes, w_exp [n, k / 32] E8M0 bytes (one
// power-of-two scale per 32 elements along k); X, C, bias 16-bit (T = bf16 /
// fp16); fp32 accumulate, one rounding to T.  Under the scale contract of
// pli.h every element value is a normal number of T, so the widening
// (v_cvt_scalef32_pk_{bf16,f16}_fp4, the block scale as its fp32 operand) is
// exact, a value x 16-bit product is exact in fp32, and the 16-bit tolerances
// hold against an oracle over the dequantised weights.  The weight stream is
// 4.25 bits per element: 0.53 of the fp8 kernels', 0.27 of the 16-bit ones'.
//
// Kernels (index arithmetic and routes: mxfp4w_plan.h, checked on the CPU by
// tests/host/mxfp4w_plan_check.cpp):
//   mxfp4w_vec      VALU, M <= 16 (M = 1 is the GEMV): linear_fp8w_vec over
//                   half-byte rows, one scale byte per 16-byte chunk
//   mxfp4w_smallm   MFMA 16x16x32, 1 < M <= 128: the block scale folded into
//                   the A operand, k granule 512
//   mxfp4w_generic  one thread per output, anything (header codec)
//   mxfp4w_widen    codes -> T(decode * scale) into a workspace for the
//                   existing pli_gemm / pli_gemm_swiglu (M > 16 without a
//                   fast route)
// SWIGLU forms stream row j of Wg and of Wu and write silu(g) * u; neither
// gate nor up is written to memory.
#include <type_traits>

#include "fp4_codec.h"
#include "mxfp4w_plan.h"
#include "pli_common.h"

namespace pli {
// capi.cpp: put `first` in front of the calling thread's route string
void route_prepend(const char* first);

namespace {

// gemm.hip's silu_mul (the same expression, so the fused SwiGLU forms agree)
__device__ __forceinline__ float silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

// acc + lo(a) * lo(b) + hi(a) * hi(b) of two packed pairs of T, fp32 accumulate: v_dot2_f32_bf16 / v_dot2_f32_f16
template <typename T> __device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float acc);
template <> __device__ __forceinline__ float dot2<bf16_t>(uint32_t a, uint32_t b, float acc) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a), __builtin_bit_cast(bf16x2, b), acc, false);
}
template <> __device__ __forceinline__ float dot2<f16_t>(uint32_t a, uint32_t b, float acc) {
    typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b), acc, false);
}
template <typename T> __device__ __forceinline__ float dot8(const i32x4& w, const i32x4& x, float acc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int wi = w[i], xi = x[i];  // copy the lanes out first (gemv.hip)
        acc = dot2<T>((uint32_t)wi, (uint32_t)xi, acc);
    }
    return acc;
}

// The fp32 operand of the scaled conversions for scale byte s: 2^(s - 127) for
// every byte of the scale contract (s << 23 is its fp32 pattern).  0xFF is
// handled by fp4_poison, not here.
__device__ __forceinline__ float mx_scale_f32(uint32_t s) { return __uint_as_float(s << 23); }

// Byte SEL of w (codes 2 SEL in bits 3:0 and 2 SEL + 1 in bits 7:4 of it) -> one dword of two T, each
// decode(code) * sc: v_cvt_scalef32_pk_{bf16,f16}_fp4.  Exact when the product is a normal number of T.
template <typename T, int SEL> __device__ __forceinline__ uint32_t fp4_widen2(uint32_t w, float sc) {
    if constexpr (std::is_same<T, bf16_t>::value)
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, SEL));
    else
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, SEL));
}
template <typename T> __device__ __forceinline__ i32x4 fp4_widen8(uint32_t w, float sc) {
    return i32x4{(int)fp4_widen2<T, 0>(w, sc), (int)fp4_widen2<T, 1>(w, sc), (int)fp4_widen2<T, 2>(w, sc),
                 (int)fp4_widen2<T, 3>(w, sc)};
}
// The pair a 0xFF scale byte puts in place of a block's first widened pair: NaN poisons every dot product and
// every MFMA row the block enters, whatever the conversion does with such an operand.
template <typename T> __device__ __forceinline__ int fp4_poison(uint32_t s, int pair) {
    constexpr int kNaN2 = std::is_same<T, bf16_t>::value ? 0x7fc07fc0 : 0x7e007e00;
    return s == 0xffu ? kNaN2 : pair;
}
// One block (a 16-byte load, scale byte s) -> 32 T in element order: o[h] = elements 8 h .. 8 h + 7, the first
// pair poisoned for a 0xFF scale.
template <typename T> __device__ __forceinline__ void fp4_widen32(const i32x4& x, uint32_t s, i32x4 (&o)[4]) {
    const float sc = mx_scale_f32(s);
    o[0] = fp4_widen8<T>((uint32_t)x.x, sc);
    o[1] = fp4_widen8<T>((uint32_t)x.y, sc);
    o[2] = fp4_widen8<T>((uint32_t)x.z, sc);
    o[3] = fp4_widen8<T>((uint32_t)x.w, sc);
    o[0].x = fp4_poison<T>(s, o[0].x);
}

// ---------------------------------------------------------------------------
// mxfp4w_vec: a wave owns ROWS consecutive weight rows (of Wg and Wu when
// SWIGLU); lane l streams the 16-byte chunks l, l + 64, ... of each row
// (non-temporal: W is read once) and the one scale byte of each chunk, all
// NW x ROWS x CPL code loads and scale loads issued before the first use.  A
// chunk is one block of 32 codes; the matching 64 bytes of every X row (L1 /
// L2 resident) are read once per chunk and reused for the wave's rows.  fp32
// accumulators, one wave reduction per output.
template <typename T, int NB, int ROWS, int CPL, bool SWIGLU, bool BIAS>
__global__ __launch_bounds__(kMxfp4wVecWaves * 64) void mxfp4w_vec(
    const char* __restrict__ X, const char* __restrict__ W, const uint8_t* __restrict__ S,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ C, int M, int N, int nchunks, int64_t ldx,
    int64_t ldw, int64_t lds, int64_t ldc, const char* __restrict__ Wu, const uint8_t* __restrict__ Su, int64_t ldwu,
    int64_t ldsu) {
    constexpr int NW = SWIGLU ? 2 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row0 = mxfp4w_vec_row0(blockIdx.x, wave, ROWS);
    if (row0 >= N) return;
    const char* wrow[NW][ROWS];
    const uint8_t* srow[NW][ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int row = mxfp4w_vec_row(row0, r, N);
        wrow[0][r] = W + mxfp4w_vec_w_off(row, 0, ldw);
        srow[0][r] = S + mxfp4w_vec_s_off(row, 0, lds);
        if constexpr (SWIGLU) {
            wrow[NW - 1][r] = Wu + mxfp4w_vec_w_off(row, 0, ldwu);
            srow[NW - 1][r] = Su + mxfp4w_vec_s_off(row, 0, ldsu);
        }
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
        uint32_t sv[NW][ROWS][CPL];
#pragma unroll
        for (int u = 0; u < CPL; ++u) {
            const int cc = mxfp4w_vec_chunk_clamped(mxfp4w_vec_chunk(c0, lane, u), nchunks);
#pragma unroll
            for (int w = 0; w < NW; ++w)
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    wv[w][r][u] =
                        __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wrow[w][r] + (int64_t)cc * 16));
                    sv[w][r][u] = srow[w][r][cc];
                }
        }
#pragma unroll
        for (int u = 0; u < CPL; ++u) {
            const int cc = mxfp4w_vec_chunk(c0, lane, u);
            if (cc < nchunks) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {  // 16 codes at a time: bounds the widened registers
                    i32x4 wl[NW][ROWS][2];
#pragma unroll
                    for (int w = 0; w < NW; ++w)
#pragma unroll
                        for (int r = 0; r < ROWS; ++r) {
                            const float sc = mx_scale_f32(sv[w][r][u]);
                            const i32x4 v = wv[w][r][u];
                            wl[w][r][0] = fp4_widen8<T>((uint32_t)(half ? v.z : v.x), sc);
                            wl[w][r][1] = fp4_widen8<T>((uint32_t)(half ? v.w : v.y), sc);
                            wl[w][r][0].x = fp4_poison<T>(sv[w][r][u], wl[w][r][0].x);  // either half poisons the sum
                        }
#pragma unroll
                    for (int bb = 0; bb < NB; ++bb) {
                        if (bb < M) {
                            const char* xp = X + mxfp4w_vec_x_off(bb, cc, ldx) * 2 + half * 32;
                            const i32x4 x0 = *reinterpret_cast<const i32x4*>(xp);
                            const i32x4 x1 = *reinterpret_cast<const i32x4*>(xp + 16);
#pragma unroll
                            for (int w = 0; w < NW; ++w)
#pragma unroll
                                for (int r = 0; r < ROWS; ++r)
                                    acc[w][r][bb] =
                                        dot8<T>(wl[w][r][1], x1, dot8<T>(wl[w][r][0], x0, acc[w][r][bb]));
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int64_t row = row0 + r;
        if (row >= N) break;  // wave-uniform
        float bn = 0.f;
        if constexpr (BIAS) bn = elem<T>::to_f32(T{bias[row]});
#pragma unroll
        for (int bb = 0; bb < NB; ++bb) {
            if (bb < M) {
                float v = wave_sum(acc[0][r][bb]);
                if constexpr (SWIGLU) v = silu_mul(v, wave_sum(acc[NW - 1][r][bb]));
                if constexpr (BIAS) v += bn;
                if (lane == 0) C[(int64_t)bb * ldc + row] = __builtin_bit_cast(uint16_t, elem<T>::from_f32(v));
            }
        }
    }
}

// ---------------------------------------------------------------------------
// mxfp4w_smallm: C^T[16 W rows][M] on v_mfma_f32_16x16x32.  One workgroup per
// 16 W rows, K split over its 4 waves, W streamed exactly once (one block of
// 32 codes per lane and load: 1 KiB per wave-instruction, U of them and their
// scale bytes issued ahead), X fragments from L2, partial C^T tiles summed
// through LDS in wave order.  The MFMA sums k-slots of different lanes, which
// are different blocks, so the block scale is folded into the A operand by
// the widening conversion (exact under the scale contract).  k-permutation
// (mxfp4w_plan.h): the lane's block is k = kb + 0..31 of row r16 with
// kb = wave K/4 + 128 step + 32 (lane >> 4); its four widened quarters are
// the A operands of four MFMAs, whose B operands are X[row][kb + 8 h + 0..7]:
// 64 contiguous bytes of X.
template <typename T, int NBG, bool SWIGLU, bool BIAS>
__global__ __launch_bounds__(256) void mxfp4w_smallm(
    const char* __restrict__ X, const char* __restrict__ W, const uint8_t* __restrict__ S,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ C, int M, int N, int K, int64_t ldx, int64_t ldw,
    int64_t lds, int64_t ldc, const char* __restrict__ Wu, const uint8_t* __restrict__ Su, int64_t ldwu,
    int64_t ldsu) {
    constexpr int NW = SWIGLU ? 2 : 1;
    constexpr int U = SWIGLU ? kMxfp4wSmallmUnrollSwiglu : kMxfp4wSmallmUnroll;
    constexpr int WSTEP = kMxfp4wSmallmWaveStep / 2;           // bytes of w4 per step
    constexpr int SSTEP = kMxfp4wSmallmWaveStep / kMxfp4Block;  // scale bytes per step
    __shared__ __attribute__((aligned(16))) float part[4][NBG][NW][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * 16;
    const int r16 = lane & 15;
    const int kw = mxfp4w_smallm_kw(K);
    const int wrow = mxfp4w_smallm_w_row(n0, lane, N);
    const int kb0 = mxfp4w_smallm_k(wave, kw, 0, lane);
    const char* wp[NW];
    const uint8_t* sp[NW];
    wp[0] = W + mxfp4w_smallm_w_off(wrow, kb0, ldw);
    sp[0] = S + mxfp4w_smallm_s_off(wrow, kb0, lds);
    if constexpr (SWIGLU) {
        wp[NW - 1] = Wu + mxfp4w_smallm_w_off(wrow, kb0, ldwu);
        sp[NW - 1] = Su + mxfp4w_smallm_s_off(wrow, kb0, ldsu);
    }
    const char* xp[NBG];
#pragma unroll
    for (int gi = 0; gi < NBG; ++gi)
        xp[gi] = X + mxfp4w_smallm_x_off(mxfp4w_smallm_x_row(gi, lane, M), kb0, 0, ldx) * 2;
    f32x4 acc[NW][NBG];
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int gi = 0; gi < NBG; ++gi) acc[w][gi] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int steps = kw / kMxfp4wSmallmWaveStep;
    int s = 0;
    for (; s + U <= steps; s += U) {
        i32x4 wf[NW][U];
        uint32_t sf[NW][U];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                wf[w][u] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp[w] + (s + u) * WSTEP));
                sf[w][u] = sp[w][(s + u) * SSTEP];
            }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            i32x4 a[NW][4];
#pragma unroll
            for (int w = 0; w < NW; ++w) fp4_widen32<T>(wf[w][u], sf[w][u], a[w]);
#pragma unroll
            for (int h = 0; h < 4; ++h)
#pragma unroll
                for (int gi = 0; gi < NBG; ++gi) {
                    const i32x4 xf =
                        *reinterpret_cast<const i32x4*>(xp[gi] + (s + u) * kMxfp4wSmallmWaveStep * 2 + 16 * h);
#pragma unroll
                    for (int w = 0; w < NW; ++w) acc[w][gi] = mfma16x16x32<T>(a[w][h], xf, acc[w][gi]);
                }
        }
    }
    for (; s < steps; ++s) {  // remainder steps
        i32x4 a[NW][4];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const i32x4 wf = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp[w] + s * WSTEP));
            fp4_widen32<T>(wf, sp[w][s * SSTEP], a[w]);
        }
#pragma unroll
        for (int h = 0; h < 4; ++h)
#pragma unroll
            for (int gi = 0; gi < NBG; ++gi) {
                const i32x4 xf = *reinterpret_cast<const i32x4*>(xp[gi] + s * kMxfp4wSmallmWaveStep * 2 + 16 * h);
#pragma unroll
                for (int w = 0; w < NW; ++w) acc[w][gi] = mfma16x16x32<T>(a[w][h], xf, acc[w][gi]);
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
                if constexpr (SWIGLU)
                    v[r] = silu_mul(v[r], part[0][gi][NW - 1][r][lane] + part[1][gi][NW - 1][r][lane] +
                                              part[2][gi][NW - 1][r][lane] + part[3][gi][NW - 1][r][lane]);
                if constexpr (BIAS) v[r] += elem<T>::to_f32(T{bias[nr + r]});
            }
            *reinterpret_cast<i32x2*>(C + (int64_t)bt * ldc + nr) =
                i32x2{(int)pack2<T>(v[0], v[1]), (int)pack2<T>(v[2], v[3])};
        }
    }
}

// ---------------------------------------------------------------------------
// mxfp4w_generic: one thread per output, any M / N / ld / alignment (K a
// multiple of 32), K = 0 (bias or 0).  Decodes with the header codec; the
// element value decode * scale is exact in fp32; fp32 fma in k order.
template <typename T, bool SWIGLU>
__global__ __launch_bounds__(256) void mxfp4w_generic(
    const T* __restrict__ X, const uint8_t* __restrict__ W, const uint8_t* __restrict__ S,
    const T* __restrict__ bias, T* __restrict__ C, int M, int N, int K, int64_t ldx, int64_t ldw, int64_t lds,
    int64_t ldc, const uint8_t* __restrict__ Wu, const uint8_t* __restrict__ Su, int64_t ldwu, int64_t ldsu) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)M * N) return;
    const int r = (int)(i / N), j = (int)(i % N);
    const T* x = X + (int64_t)r * ldx;
    float g = 0.f, u = 0.f;
    for (int kb = 0; kb < K; kb += kMxfp4Block) {
        const float sg = e8m0_decode(S[(int64_t)j * lds + kb / kMxfp4Block]);
        float su = 0.f;
        if constexpr (SWIGLU) su = e8m0_decode(Su[(int64_t)j * ldsu + kb / kMxfp4Block]);
        for (int kk = kb; kk < kb + kMxfp4Block; ++kk) {
            const float xv = elem<T>::to_f32(x[kk]);
            g = fmaf(fp4_e2m1_decode(fp4_nibble(W[(int64_t)j * ldw + kk / 2], kk)) * sg, xv, g);
            if constexpr (SWIGLU)
                u = fmaf(fp4_e2m1_decode(fp4_nibble(Wu[(int64_t)j * ldwu + kk / 2], kk)) * su, xv, u);
        }
    }
    float v = g;
    if constexpr (SWIGLU) v = silu_mul(g, u);
    if (bias) v += elem<T>::to_f32(bias[j]);
    C[(int64_t)r * ldc + j] = elem<T>::from_f32(v);
}

// ---------------------------------------------------------------------------
// mxfp4w_widen: out[j][i] = T( decode(code) * 2^(scale - 127) ), out
// contiguous [n][k]: exact under the scale contract, NaN for a 0xFF scale.
// VEC: one thread per block of 32 codes by the scaled conversion (ldw a
// multiple of 16, w4 16-byte aligned), else one per element by the header codec.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void mxfp4w_widen(const uint8_t* __restrict__ W, const uint8_t* __restrict__ S,
                                                    uint16_t* __restrict__ out, int N, int K, int64_t ldw,
                                                    int64_t lds) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if constexpr (VEC) {
        const int bpr = K / kMxfp4Block;  // blocks per row
        if (i >= (int64_t)N * bpr) return;
        const int j = (int)(i / bpr), b = (int)(i % bpr);
        const uint32_t s = S[(int64_t)j * lds + b];
        i32x4 o[4];
        fp4_widen32<T>(*reinterpret_cast<const i32x4*>(W + (int64_t)j * ldw + (int64_t)b * 16), s, o);
        i32x4* dst = reinterpret_cast<i32x4*>(out + (int64_t)j * K + (int64_t)b * kMxfp4Block);
#pragma unroll
        for (int h = 0; h < 4; ++h) {  // the GEMM consumes the elements separately: all 32 are NaN for a 0xFF scale
#pragma unroll
            for (int e = 0; e < 4; ++e) o[h][e] = fp4_poison<T>(s, o[h][e]);
            dst[h] = o[h];
        }
    } else {
        if (i >= (int64_t)N * K) return;
        const int j = (int)(i / K), c = (int)(i % K);
        const float v = fp4_e2m1_decode(fp4_nibble(W[(int64_t)j * ldw + c / 2], c)) *
                        e8m0_decode(S[(int64_t)j * lds + c / kMxfp4Block]);
        out[i] = __builtin_bit_cast(uint16_t, elem<T>::from_f32(v));
    }
}

// ------------------------------------------------------------------ launch --
struct Mxfp4wArgs {
    const void *x, *w, *bias, *wu;
    const uint8_t *s, *su;
    void* c;
    int m, n, k;
    int64_t ldx, ldw, lds, ldwu, ldsu, ldc;
    bool swiglu;
};

template <typename T, int NB, int ROWS, int CPL, bool SWIGLU>
int launch_vec_cfg(const Mxfp4wArgs& a, hipStream_t s) {
    const dim3 grid(mxfp4w_vec_grid(a.n, ROWS)), block(kMxfp4wVecWaves * 64);
    const int nch = a.k / kMxfp4Block;
#define PLI_MXFP4W_VEC(BIAS)                                                                                  \
    hipLaunchKernelGGL((mxfp4w_vec<T, NB, ROWS, CPL, SWIGLU, BIAS>), grid, block, 0, s, (const char*)a.x,     \
                       (const char*)a.w, a.s, (const uint16_t*)a.bias, (uint16_t*)a.c, a.m, a.n, nch, a.ldx,  \
                       a.ldw, a.lds, a.ldc, (const char*)a.wu, a.su, a.ldwu, a.ldsu)
    if constexpr (SWIGLU) {
        PLI_MXFP4W_VEC(false);
        return launch_status("mxfp4w_vec<swiglu>");
    } else {
        if (a.bias) PLI_MXFP4W_VEC(true);
        else PLI_MXFP4W_VEC(false);
        return launch_status("mxfp4w_vec");
    }
#undef PLI_MXFP4W_VEC
}

template <typename T, int NB, bool SWIGLU>
int launch_vec_nb(const Mxfp4wArgs& a, hipStream_t s) {
    constexpr int R = SWIGLU ? 4 : 8;  // mxfp4w_vec_cfg: rows x cpl = R
    switch (mxfp4w_vec_cfg(a.k, SWIGLU).cpl) {
        case 1: return launch_vec_cfg<T, NB, R, 1, SWIGLU>(a, s);
        case 2: return launch_vec_cfg<T, NB, R / 2, 2, SWIGLU>(a, s);
        default: return launch_vec_cfg<T, NB, R / 4, 4, SWIGLU>(a, s);
    }
}

template <typename T, bool SWIGLU>
int launch_vec(const Mxfp4wArgs& a, hipStream_t s) {
    if (a.m <= 1) return launch_vec_nb<T, 1, SWIGLU>(a, s);
    if (a.m <= 2) return launch_vec_nb<T, 2, SWIGLU>(a, s);
    if (a.m <= 4) return launch_vec_nb<T, 4, SWIGLU>(a, s);
    if (a.m <= 8) return launch_vec_nb<T, 8, SWIGLU>(a, s);
    return launch_vec_nb<T, 16, SWIGLU>(a, s);
}

template <typename T, int NBG, bool SWIGLU>
int launch_smallm_nbg(const Mxfp4wArgs& a, hipStream_t s) {
    const dim3 grid(a.n / 16), block(256);
#define PLI_MXFP4W_SMALLM(BIAS)                                                                                \
    hipLaunchKernelGGL((mxfp4w_smallm<T, NBG, SWIGLU, BIAS>), grid, block, 0, s, (const char*)a.x,             \
                       (const char*)a.w, a.s, (const uint16_t*)a.bias, (uint16_t*)a.c, a.m, a.n, a.k, a.ldx,   \
                       a.ldw, a.lds, a.ldc, (const char*)a.wu, a.su, a.ldwu, a.ldsu)
    if constexpr (SWIGLU) {
        PLI_MXFP4W_SMALLM(false);
        return launch_status("mxfp4w_smallm<swiglu>");
    } else {
        if (a.bias) PLI_MXFP4W_SMALLM(true);
        else PLI_MXFP4W_SMALLM(false);
        return launch_status("mxfp4w_smallm");
    }
#undef PLI_MXFP4W_SMALLM
}

template <typename T, bool SWIGLU>
int launch_smallm(const Mxfp4wArgs& a, hipStream_t s) {
    switch (mxfp4w_smallm_nbg(a.m)) {
        case 1: return launch_smallm_nbg<T, 1, SWIGLU>(a, s);
        case 2: return launch_smallm_nbg<T, 2, SWIGLU>(a, s);
        case 4: return launch_smallm_nbg<T, 4, SWIGLU>(a, s);
        default: return launch_smallm_nbg<T, 8, SWIGLU>(a, s);
    }
}

template <typename T, bool SWIGLU>
int launch_generic(const Mxfp4wArgs& a, hipStream_t s) {
    const int64_t blocks = ((int64_t)a.m * a.n + 255) / 256;
    hipLaunchKernelGGL((mxfp4w_generic<T, SWIGLU>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)a.x,
                       (const uint8_t*)a.w, a.s, (const T*)a.bias, (T*)a.c, a.m, a.n, a.k, a.ldx, a.ldw, a.lds,
                       a.ldc, (const uint8_t*)a.wu, a.su, a.ldwu, a.ldsu);
    return launch_status(SWIGLU ? "mxfp4w_generic<swiglu>" : "mxfp4w_generic");
}

template <typename T>
int launch_widen(const void* w, const uint8_t* sc, void* out, int n, int k, int64_t ldw, int64_t lds,
                 hipStream_t s) {
    const bool vec = ldw % 16 == 0 && aligned16(w);
    const int64_t items = vec ? (int64_t)n * (k / kMxfp4Block) : (int64_t)n * k;
    const dim3 grid((unsigned)((items + 255) / 256)), block(256);
    if (vec)
        hipLaunchKernelGGL((mxfp4w_widen<T, true>), grid, block, 0, s, (const uint8_t*)w, sc, (uint16_t*)out, n, k,
                           ldw, lds);
    else
        hipLaunchKernelGGL((mxfp4w_widen<T, false>), grid, block, 0, s, (const uint8_t*)w, sc, (uint16_t*)out, n, k,
                           ldw, lds);
    return launch_status("mxfp4w_widen");
}

template <typename T, bool SWIGLU>
int run_route(int route, const Mxfp4wArgs& a, hipStream_t s) {
    switch (route) {
        case MXFP4W_SMALLM: return launch_smallm<T, SWIGLU>(a, s);
        case MXFP4W_VEC: return launch_vec<T, SWIGLU>(a, s);
        default: return launch_generic<T, SWIGLU>(a, s);
    }
}

// argument checks, route, launch.  `what` names the entry point in messages.
int dispatch(const char* what, const Mxfp4wArgs& a, int dtype, void* ws, size_t ws_bytes, void* stream) {
    clear_error();
    PLI_REQUIRE(a.m >= 0 && a.n >= 0 && a.k >= 0, "%s: bad shape m=%d n=%d k=%d", what, a.m, a.n, a.k);
    PLI_REQUIRE(dtype == PLI_F16 || dtype == PLI_BF16, "%s: bad dtype %d (fp16 / bf16 activations only)", what, dtype);
    PLI_REQUIRE(mxfp4w_shape_ok(a.k), "%s: k=%d is not a multiple of the MX block of 32", what, a.k);
    PLI_REQUIRE(a.ldx >= a.k && a.ldw >= a.k / 2 && a.lds >= a.k / kMxfp4Block && a.ldc >= a.n &&
                    (!a.swiglu || (a.ldwu >= a.k / 2 && a.ldsu >= a.k / kMxfp4Block)),
                "%s: leading dimension too small (ldx=%lld ldw=%lld lds=%lld ldwu=%lld ldsu=%lld ldc=%lld)", what,
                (long long)a.ldx, (long long)a.ldw, (long long)a.lds, (long long)a.ldwu, (long long)a.ldsu,
                (long long)a.ldc);
    if (a.m == 0 || a.n == 0) return PLI_OK;  // empty operands may be NULL
    PLI_REQUIRE(a.c && (a.k == 0 || (a.x && a.w && a.s && (!a.swiglu || (a.wu && a.su)))),
                "%s: null pointer (the scale bytes have no default)", what);
    PLI_REQUIRE(((int64_t)a.m * a.n + 255) / 256 <= 0x7fffffffLL, "%s: grid too large", what);
    const Mxfp4wCall call{a.m, a.n, a.k, a.ldx, a.ldw | (a.swiglu ? a.ldwu : 0), a.ldc,
                          (uintptr_t)a.w | (a.swiglu ? (uintptr_t)a.wu : 0), (uintptr_t)a.x, (uintptr_t)a.c,
                          (uintptr_t)a.bias, (uintptr_t)ws, ws_bytes, a.swiglu};
    const int route = mxfp4w_route(call);
    PLI_REQUIRE(route != MXFP4W_BAD_WORKSPACE,
                "%s: workspace must be 16-byte aligned and hold %zu bytes (got %zu at %p)", what,
                mxfp4w_workspace_need(a.n, a.k, a.swiglu), ws_bytes, ws);
    hipStream_t s = (hipStream_t)stream;
    if (route == MXFP4W_WIDEN) {
        // the widened weight(s), contiguous [n][k] of T, then the 16-bit GEMM
        char* wsg = (char*)ws;
        char* wsu = wsg + mxfp4w_widened_bytes(a.n, a.k);
        int rc = dtype == PLI_BF16 ? launch_widen<bf16_t>(a.w, a.s, wsg, a.n, a.k, a.ldw, a.lds, s)
                                   : launch_widen<f16_t>(a.w, a.s, wsg, a.n, a.k, a.ldw, a.lds, s);
        if (rc != PLI_OK) return rc;
        if (a.swiglu) {
            rc = dtype == PLI_BF16 ? launch_widen<bf16_t>(a.wu, a.su, wsu, a.n, a.k, a.ldwu, a.ldsu, s)
                                   : launch_widen<f16_t>(a.wu, a.su, wsu, a.n, a.k, a.ldwu, a.ldsu, s);
            if (rc != PLI_OK) return rc;
            rc = pli_gemm_swiglu(a.x, wsg, wsu, a.c, a.m, a.n, a.k, a.ldx, a.k, a.k, a.ldc, dtype, stream);
            if (rc == PLI_OK) route_prepend("mxfp4w_widen+mxfp4w_widen");
            return rc;
        }
        rc = pli_gemm(a.x, wsg, a.c, a.bias, a.m, a.n, a.k, a.ldx, a.k, a.ldc, 1, dtype, stream);
        if (rc == PLI_OK) route_prepend("mxfp4w_widen");  // pli_gemm started the route string anew
        return rc;
    }
    const int r = (a.k == 0) ? MXFP4W_GENERIC : route;
    if (a.swiglu)
        return dtype == PLI_BF16 ? run_route<bf16_t, true>(r, a, s) : run_route<f16_t, true>(r, a, s);
    return dtype == PLI_BF16 ? run_route<bf16_t, false>(r, a, s) : run_route<f16_t, false>(r, a, s);
}

}  // namespace
}  // namespace pli

extern "C" size_t pli_linear_mxfp4w_workspace_size(int m, int n, int k, int dtype) {
    if (dtype != PLI_BF16 && dtype != PLI_F16) return 0;
    return pli::mxfp4w_workspace_size(m, n, k, false);
}

extern "C" size_t pli_linear_swiglu_mxfp4w_workspace_size(int m, int n, int k, int dtype) {
    if (dtype != PLI_BF16 && dtype != PLI_F16) return 0;
    return pli::mxfp4w_workspace_size(m, n, k, true);
}

extern "C" int pli_linear_mxfp4w(const void* x, const void* w4, const void* w_exp, const void* bias, void* c, int m,
                                 int n, int k, int64_t ldx, int64_t ldw, int64_t lds, int64_t ldc, int dtype,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    const pli::Mxfp4wArgs a{x, w4, bias, nullptr, (const uint8_t*)w_exp, nullptr, c, m, n, k, ldx, ldw, lds, 0, 0, ldc,
                            false};
    return pli::dispatch("pli_linear_mxfp4w", a, dtype, workspace, workspace_bytes, stream);
}

// y = W x: pli_linear_mxfp4w with one X row and no bias, on the same kernel
extern "C" int pli_gemv_mxfp4w(const void* w4, const void* w_exp, const void* x, void* y, int m, int k, int64_t ldw,
                               int64_t lds, int dtype, void* stream) {
    const pli::Mxfp4wArgs a{x, w4, nullptr, nullptr, (const uint8_t*)w_exp, nullptr, y, 1, m, k, k, ldw, lds, 0, 0, m,
                            false};
    return pli::dispatch("pli_gemv_mxfp4w", a, dtype, nullptr, 0, stream);
}

extern "C" int pli_linear_swiglu_mxfp4w(const void* x, const void* wg4, const void* wg_exp, const void* wu4,
                                        const void* wu_exp, void* h, int m, int n, int k, int64_t ldx, int64_t ldwg,
                                        int64_t ldsg, int64_t ldwu, int64_t ldsu, int64_t ldh, int dtype,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    const pli::Mxfp4wArgs a{x, wg4, nullptr, wu4, (const uint8_t*)wg_exp, (const uint8_t*)wu_exp, h, m, n, k, ldx, ldwg,
                            ldsg, ldwu, ldsu, ldh, true};
    return pli::dispatch("pli_linear_swiglu_mxfp4w", a, dtype, workspace, workspace_bytes, stream);
}
