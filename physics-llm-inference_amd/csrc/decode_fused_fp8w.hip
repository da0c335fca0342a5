// Decode-step fusion over fp8 weights (W8A16) for gfx950: residual add +
// RMSNorm + the fp8-weight projection that consumes the normalised rows, in
// one launch.  pli_rms_gemm_nt_fp8w is pli_rms_gemm_nt (decode_fused.hip) with
// (codes, scale) pairs in place of the 16-bit weights: rms_gemm_skinny's norm
// phase in front of linear_fp8w_vec's dot phase (linear_fp8w.hip).  Per
// 256-thread workgroup:
//   1. the first trip of the workgroup's weight loads (HBM latency overlaps 2);
//   2. h = a (+ residual), sum of squares, y = h * (1 / sqrt(mean + eps)) * g
//      with the thread layout and operation order of rmsnorm_vec (norm.hip), so
//      y is bitwise the row pli_rmsnorm would write; y goes to LDS (never to
//      HBM), workgroup 0 writes h (the next residual);
//   3. a wave owns ROWS output rows: lane l streams the 16-byte chunks l,
//      l + 64, ... (16 e4m3fn codes, non-temporal) of each, widens them with
//      fp8_widen16 and runs linear_fp8w_vec's dot2 MACs against the 2 x 16
//      bytes of every y row in LDS -- the same per-lane chunk and accumulate
//      order, so the result is bitwise pli_rmsnorm -> pli_linear_fp8w's.
// Output groups as pli_rms_gemm_nt (q / k / v straight into the caches at a
// device-resident position), each with its own codes, scales and width; with
// wu8, SwiGLU (silu(sg g) * (su u)).  Index arithmetic: rms_fp8w_plan.h,
// checked on the CPU by tests/host/rms_fp8w_plan_check.cpp.
#include <cmath>

#include "fp8_kv.h"
#include "pli_common.h"
#include "rms_fp8w_plan.h"

namespace pli {
namespace {

struct RmsFp8wGroup {
    const char* w;
    const char* wu;
    const float* w_scale;
    const float* wu_scale;
    uint16_t* c;
    int64_t ldw, stride_batch, stride_token;
    const int* row_offset;
    int capacity;
};
struct RmsFp8wArgs {
    RmsFp8wGroup g[kRmsFp8wMaxGroups];
    int n[kRmsFp8wMaxGroups];
    int ngroups, ntot;
};

// linear_fp8w.hip's silu_mul, dot2 and dot8 (the same expressions, so the fused forms agree bit for bit)
__device__ __forceinline__ float silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

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

// block_sum of norm.hip (same order: wave butterfly, then the 4 wave partials in order)
__device__ __forceinline__ float rms_block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// group gi's descriptor without a dynamically indexed copy of the kernel arguments
__device__ __forceinline__ const RmsFp8wGroup& group_of(const RmsFp8wArgs& args, int gi) {
    return gi == 0 ? args.g[0] : gi == 1 ? args.g[1] : args.g[2];
}

template <typename T, int NB, int ROWS, int CPL, bool SW, int RPT>
__global__ __launch_bounds__(256) void rms_gemm_fp8w(const uint16_t* __restrict__ A, int64_t lda,
                                                     const uint16_t* __restrict__ R, int64_t ldr,
                                                     const uint16_t* __restrict__ G, float eps,
                                                     uint16_t* __restrict__ Hout, int64_t ldh, int M, int S,
                                                     int K, RmsFp8wArgs args) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];  // y [M][K]
    __shared__ float red[4];
    constexpr int NW = SW ? 2 : 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch8 = K / kRmsFp8wNormChunk;  // 16-byte chunks of a 16-bit row (norm phase)
    const int nchunks = K / kFp8wChunk;      // 16-byte chunks of a row of codes (dot phase)
    uint16_t* xs = reinterpret_cast<uint16_t*>(dsm);

    const int64_t row0 = fp8w_vec_row0(blockIdx.x, wave, ROWS);
    const bool active = row0 < args.ntot;  // inactive waves still join the norm's barriers
    const char* wrow[NW][ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const RmsFp8wRow lr = rms_fp8w_load_row(active ? row0 + r : 0, args.n, args.ngroups);
        const RmsFp8wGroup& Gp = group_of(args, lr.group);
        wrow[0][r] = Gp.w + fp8w_vec_w_off(lr.row, 0, Gp.ldw);
        if constexpr (SW) wrow[NW - 1][r] = Gp.wu + fp8w_vec_w_off(lr.row, 0, Gp.ldw);
    }
    i32x4 wv[NW][ROWS][CPL];
    auto load_w = [&](int c0) {
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
    };
    if (active) load_w(0);

    // ---- residual add + RMSNorm of the M rows into LDS (rmsnorm_vec's order)
    for (int bb = 0; bb < M; ++bb) {
        float v[RPT][8];
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int c = tid + 256 * i;
            if (c < nch8) {
                const i32x4 xv = *reinterpret_cast<const i32x4*>(A + bb * lda + 8 * c);
                i32x4 rv = {0, 0, 0, 0};
                if (R) rv = *reinterpret_cast<const i32x4*>(R + bb * ldr + 8 * c);
                uint32_t hw[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t xw = (uint32_t)xv[j], rw = (uint32_t)rv[j];
                    float a0 = elem<T>::to_f32(T{(uint16_t)(xw & 0xffff)});
                    float a1 = elem<T>::to_f32(T{(uint16_t)(xw >> 16)});
                    if (R) {
                        a0 = elem<T>::to_f32(elem<T>::from_f32(a0 + elem<T>::to_f32(T{(uint16_t)(rw & 0xffff)})));
                        a1 = elem<T>::to_f32(elem<T>::from_f32(a1 + elem<T>::to_f32(T{(uint16_t)(rw >> 16)})));
                    }
                    hw[j] = pack2<T>(a0, a1);
                    v[i][2 * j] = a0;
                    v[i][2 * j + 1] = a1;
                    ss = fmaf(a0, a0, fmaf(a1, a1, ss));
                }
                if (Hout && blockIdx.x == 0)
                    *reinterpret_cast<i32x4*>(Hout + bb * ldh + 8 * c) =
                        i32x4{(int)hw[0], (int)hw[1], (int)hw[2], (int)hw[3]};
            }
        }
        const float inv = 1.f / sqrtf(rms_block_sum(ss, red) / (float)K + eps);
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int c = tid + 256 * i;
            if (c < nch8) {
                const i32x4 gv = *reinterpret_cast<const i32x4*>(G + 8 * c);
                uint32_t o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t gw = (uint32_t)gv[j];
                    o[j] = pack2<T>(v[i][2 * j] * inv * elem<T>::to_f32(T{(uint16_t)(gw & 0xffff)}),
                                    v[i][2 * j + 1] * inv * elem<T>::to_f32(T{(uint16_t)(gw >> 16)}));
                }
                *reinterpret_cast<i32x4*>(xs + bb * K + 8 * c) =
                    i32x4{(int)o[0], (int)o[1], (int)o[2], (int)o[3]};
            }
        }
    }
    __syncthreads();
    if (!active) return;  // past the last barrier

    // ---- ROWS output rows per wave, x from LDS (linear_fp8w_vec's chunk and accumulate order)
    float acc[NW][ROWS][NB];
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int bb = 0; bb < NB; ++bb) acc[w][r][bb] = 0.f;
    for (int c0 = 0; c0 < nchunks; c0 += 64 * CPL) {
        if (c0 > 0) load_w(c0);
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
                        const uint16_t* xp = xs + rms_fp8w_x_off(bb, cc, K);
                        const i32x4 xl = *reinterpret_cast<const i32x4*>(xp);
                        const i32x4 xh = *reinterpret_cast<const i32x4*>(xp + 8);
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
        if (row0 + r >= args.ntot) break;  // wave-uniform
        const RmsFp8wRow orow = rms_fp8w_resolve(row0 + r, args.n, args.ngroups);
        const RmsFp8wGroup& Gp = group_of(args, orow.group);
        const float sg = fp8_scale_of(Gp.w_scale, orow.row);
        float su = 1.f;
        if constexpr (SW) su = fp8_scale_of(Gp.wu_scale, orow.row);
        const int off = Gp.row_offset ? *Gp.row_offset : 0;
#pragma unroll
        for (int bb = 0; bb < NB; ++bb) {
            if (bb < M) {
                float v = sg * wave_sum(acc[0][r][bb]);
                if constexpr (SW) v = silu_mul(v, su * wave_sum(acc[NW - 1][r][bb]));
                const int b = bb / S, srow = bb % S + off;
                if (lane == 0 && srow < Gp.capacity)
                    Gp.c[b * Gp.stride_batch + (int64_t)srow * Gp.stride_token + orow.row] =
                        __builtin_bit_cast(uint16_t, elem<T>::from_f32(v));
            }
        }
    }
}

struct RmsFp8wCall {
    const uint16_t *a, *r, *g;
    uint16_t* h;
    int64_t lda, ldr, ldh;
    float eps;
    int m, s, k;
};

template <typename T, int NB, int ROWS, int CPL, bool SW, int RPT>
void launch_one(const RmsFp8wCall& c, const RmsFp8wArgs& args, hipStream_t s) {
    const dim3 grid((unsigned)rms_fp8w_grid(args.ntot, ROWS));
    hipLaunchKernelGGL((rms_gemm_fp8w<T, NB, ROWS, CPL, SW, RPT>), grid, dim3(kFp8wVecWaves * 64),
                       rms_fp8w_lds_bytes(c.m, c.k), s, c.a, c.lda, c.r, c.ldr, c.g, c.eps, c.h, c.ldh, c.m, c.s, c.k,
                       args);
}

// (ROWS, CPL) is what fp8w_vec_cfg returns and the norm's RPT what rms_fp8w_norm_rpt returns: the instance launched
// is the one whose template constants equal them (short rows: K <= 2048 <=> RPT 1; long rows: RPT 2 / 4).  A
// combination without an instance is refused, never replaced by another form.
template <typename T, int NB, bool SW>
int launch_nb(const RmsFp8wCall& c, const RmsFp8wArgs& args, hipStream_t s) {
    const Fp8wVecCfg cfg = fp8w_vec_cfg(c.k, SW);
    const int rpt = rms_fp8w_norm_rpt(c.k);
#define PLI_RMS8(ROWS, CPL, RPT)                                  \
    if (cfg.rows == ROWS && cfg.cpl == CPL && rpt == RPT) {       \
        launch_one<T, NB, ROWS, CPL, SW, RPT>(c, args, s);        \
        return PLI_OK;                                            \
    }
    if constexpr (SW) {
        PLI_RMS8(2, 2, 1) PLI_RMS8(1, 4, 2) PLI_RMS8(1, 4, 4)
    } else {
        PLI_RMS8(4, 2, 1) PLI_RMS8(2, 4, 2) PLI_RMS8(2, 4, 4)
    }
#undef PLI_RMS8
    set_error("pli_rms_gemm_nt_fp8w: no kernel for rows %d, cpl %d, rpt %d at k %d", cfg.rows, cfg.cpl, rpt, c.k);
    return PLI_EUNSUPPORTED;
}

template <typename T, bool SW>
int launch_t(const RmsFp8wCall& c, const RmsFp8wArgs& args, hipStream_t s) {
    if (c.m <= 1) return launch_nb<T, 1, SW>(c, args, s);
    if (c.m <= 2) return launch_nb<T, 2, SW>(c, args, s);
    return launch_nb<T, 4, SW>(c, args, s);
}

}  // namespace
}  // namespace pli

extern "C" int pli_rms_gemm_nt_fp8w(const void* a, int64_t lda, const void* residual, int64_t ldr,
                                    const void* norm_weight, float eps, void* h_out, int64_t ldh, int m, int k,
                                    int tokens_per_batch, const void* const* w8, const float* const* w_scale,
                                    const void* const* wu8, const float* const* wu_scale, void* const* c,
                                    const int* n, const int64_t* ldw, const int64_t* stride_batch,
                                    const int64_t* stride_token, const int32_t* const* row_offset,
                                    const int* capacity, int ngroups, int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(a && norm_weight && w8 && c && n && ldw && stride_batch && stride_token && row_offset && capacity,
                "pli_rms_gemm_nt_fp8w: null pointer");
    PLI_REQUIRE(ngroups >= 1 && ngroups <= kRmsFp8wMaxGroups, "pli_rms_gemm_nt_fp8w: 1..3 groups, got %d", ngroups);
    PLI_REQUIRE(m >= 1 && m <= kRmsFp8wMaxM && tokens_per_batch >= 1 && m % tokens_per_batch == 0,
                "pli_rms_gemm_nt_fp8w: needs 1 <= m <= 4 rows (whole batches of tokens_per_batch)");
    PLI_REQUIRE(k > 0 && k % kFp8wChunk == 0 && k <= kRmsFp8wMaxK && lda >= k && lda % 8 == 0 &&
                    (!residual || (ldr >= k && ldr % 8 == 0)) && (!h_out || (ldh >= k && ldh % 8 == 0)) &&
                    aligned16(a) && aligned16(norm_weight) && (!residual || aligned16(residual)) &&
                    (!h_out || aligned16(h_out)),
                "pli_rms_gemm_nt_fp8w: needs k %% 16 == 0, k <= 8192, 16-byte aligned rows");
    PLI_REQUIRE(dtype == PLI_BF16 || dtype == PLI_F16, "pli_rms_gemm_nt_fp8w: bf16/fp16 only");
    PLI_REQUIRE(std::isfinite(eps) && eps >= 0.f, "pli_rms_gemm_nt_fp8w: bad eps");
    RmsFp8wArgs args{};
    for (int g = 0; g < ngroups; ++g) {
        PLI_REQUIRE(w8[g] && c[g] && n[g] > 0 && ldw[g] >= k && ldw[g] % 16 == 0 && aligned16(w8[g]) &&
                        (!wu8 || (wu8[g] && aligned16(wu8[g]))),
                    "pli_rms_gemm_nt_fp8w: bad group %d", g);
        PLI_REQUIRE(n[g] <= 0x7fffffff / kRmsFp8wMaxGroups, "pli_rms_gemm_nt_fp8w: group %d too wide", g);
        args.g[g] = RmsFp8wGroup{(const char*)w8[g],
                                 wu8 ? (const char*)wu8[g] : nullptr,
                                 w_scale ? w_scale[g] : nullptr,
                                 (wu8 && wu_scale) ? wu_scale[g] : nullptr,
                                 (uint16_t*)c[g],
                                 ldw[g],
                                 stride_batch[g],
                                 stride_token[g],
                                 row_offset[g],
                                 capacity[g]};
        args.n[g] = n[g];
    }
    args.ngroups = ngroups;
    args.ntot = rms_fp8w_total(args.n, ngroups);  // the grid's input: the text the host checker replays
    // y rows in dynamic LDS next to the 16 static bytes of red[]: at most 4 * 8192 * 2 + 16 = 65552 bytes of
    // gfx950's 163840 per workgroup (no opt-in is needed below the device's limit)
    const RmsFp8wCall call{(const uint16_t*)a, (const uint16_t*)residual, (const uint16_t*)norm_weight,
                           (uint16_t*)h_out,   lda, ldr, ldh, eps, m, tokens_per_batch, k};
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (dtype == PLI_BF16) rc = wu8 ? launch_t<bf16_t, true>(call, args, s) : launch_t<bf16_t, false>(call, args, s);
    else rc = wu8 ? launch_t<f16_t, true>(call, args, s) : launch_t<f16_t, false>(call, args, s);
    if (rc != PLI_OK) return rc;
    return launch_status(wu8 ? "rms_gemm_fp8w<swiglu>" : "rms_gemm_fp8w");
}
