// Grouped W4A4 GEMM over MoE experts on gfx950 (MI355X): MXFP4 activation rows
// against each expert's MXFP4 weights (pli_gemm_grouped_mxfp4_a4).  For every
// expert e and sorted row r in [offsets[e], offsets[e + 1]), t = gather ?
// gather[r] : r:
//   C[r, j] = round_T( x_scale[t] * sum_i decode_e2m1(X4[t, i]) * 2^(x_exp[t, i/32] - 127)
//                                       * decode_e2m1(W4_e[j, i]) * 2^(w_exp_e[j, i/32] - 127) )
// or, with the up tables (fused SwiGLU over W1 / W3), g and u those two
// finished fp32 values, C[r, j] = round_T(silu(g) * u): SiLU and the product
// in fp32, one rounding.  No atomics, no workspace; offsets, gather and the
// pointer tables are read on the device, so a captured call replays.
//
// Kernels (index arithmetic and route: grouped_mxfp4x_plan.h over
// grouped_mxfp4_plan.h, mxfp4x_plan.h and fp8a_plan.h, checked on the CPU by
// tests/host/grouped_mxfp4x_plan_check.cpp):
//   gemm_grouped_mxfp4_a4<T, SW>  gemm_mxfp4_a4_mx's skeleton (C^T, 128 x 128
//       tile, K-step of 256 codes, two LDS stages fed by 16-byte LDS-DMA, every
//       operand one ds_read_b128, cbsz = blgp = 4, both sides' E8M0 bytes as
//       stored) per (128 weight rows, slot of 128 sorted rows) as in
//       gemm_grouped_mxfp4: the slot's (expert, slab) comes from a scan of the
//       device offsets, the weight bases from the pointer tables, the X rows
//       and their scale dwords through gather.  SW: a stage holds the gate W,
//       the up W and the X image; a wave keeps 2 x 2 x 2 accumulator tiles and
//       reads each X fragment once for both matrices.
//   gemm_grouped_mxfp4_a4_generic<T, SW>  one thread per output element
//       through the header codecs, any shape, leading dimension and alignment
#include "fp4_codec.h"
#include "fp8_kv.h"
#include "grouped_mxfp4x_plan.h"
#include "mx_finish.h"
#include "pli_common.h"

namespace pli {
namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;
// The experts' bases come out of the device pointer tables as generic pointers; the weights live in global memory,
// so the kernel says so: loads through these types are global_load (vmcnt only), not flat_load (vmcnt and lgkmcnt)
typedef const __attribute__((address_space(1))) uint8_t* gmx4x_gptr;
typedef const __attribute__((address_space(1))) uint32_t* gmx4x_gptr32;

// gemm.hip's expression for the 16-bit grouped kernels
__device__ __forceinline__ float gmx4x_silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

// the scale dwords of the K-step in flight: [W matrix][tile][dword], [X tile][dword]
template <int NW> struct Gmx4xScales {
    uint32_t w[NW][2][2], x[2][2];
};

// step s has landed for this wave; the dwords pass through the statement so that nothing derived from them is
// scheduled in front of the wait
template <int NW> __device__ __forceinline__ void gmx4x_wait(Gmx4xScales<NW>& sc) {
    if constexpr (NW == 1)
        asm volatile("s_waitcnt vmcnt(0)"
                     : "+v"(sc.w[0][0][0]), "+v"(sc.w[0][0][1]), "+v"(sc.w[0][1][0]), "+v"(sc.w[0][1][1]),
                       "+v"(sc.x[0][0]), "+v"(sc.x[0][1]), "+v"(sc.x[1][0]), "+v"(sc.x[1][1])::"memory");
    else
        asm volatile("s_waitcnt vmcnt(0)"
                     : "+v"(sc.w[0][0][0]), "+v"(sc.w[0][0][1]), "+v"(sc.w[0][1][0]), "+v"(sc.w[0][1][1]),
                       "+v"(sc.w[NW - 1][0][0]), "+v"(sc.w[NW - 1][0][1]), "+v"(sc.w[NW - 1][1][0]),
                       "+v"(sc.w[NW - 1][1][1]), "+v"(sc.x[0][0]), "+v"(sc.x[0][1]), "+v"(sc.x[1][0]),
                       "+v"(sc.x[1][1])::"memory");
}

// ---------------------------------------------------------------------------
// gemm_grouped_mxfp4_a4: C^T tile [128 n][128 sorted rows] = W4_e tile x X4 slab^T
// (SW: both of W1_e and W3_e).  Per K-step of 256 codes every wave LDS-DMAs 4
// KiB of each image (4 pieces of 8 rows x 128 bytes, the swizzle on the source
// address) into stage (s + 1) % 2 and loads, for each of its W tiles and its two
// X tiles, the two dwords of its row's eight scale bytes, all in flight while
// the MFMAs run on stage s % 2: one vmcnt(0) and one barrier per step.  The X
// side's source rows and scale rows go through gather once, in front of the
// loop.  A wave multiplies its 64 x 64 block as 2 x 2 tiles of 32 x 32 per
// matrix, four k-quarters of 64 codes each: 16 (SW: 32) scaled MFMAs per step,
// an X fragment read once for both matrices.  The operand and scale-byte maps
// are gemm_mxfp4_a4_mx's: a 0xFF byte on the W side makes its column of C NaN,
// on the X side its sorted row.
template <typename T, bool SW>
__device__ __forceinline__ void gmx4x_body(
    const uint8_t* __restrict__ X4, const uint8_t* __restrict__ x_exp, const float* __restrict__ x_scale,
    const int32_t* __restrict__ gather, const uint8_t* const* __restrict__ Wt, const uint8_t* const* __restrict__ Et,
    const uint8_t* const* __restrict__ Wut, const uint8_t* const* __restrict__ Eut, uint16_t* __restrict__ C,
    const int32_t* __restrict__ offsets, int E, int N, int ks, int64_t ldx4, int64_t ldxs, int64_t ldw, int64_t lds,
    int64_t ldc) {
    constexpr int NW = gmx4x_w_images(SW);
    __shared__ __attribute__((aligned(1024))) char smem[gmx4x_lds_bytes(SW)];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave & 1, wm = wave >> 1;
    const int n0 = blockIdx.x * kGmx4TN;
    const Gmx4Slab sl = gmx4_slab(offsets, E, blockIdx.y);
    if (sl.expert < 0) return;  // whole block: before any barrier
    auto token = [&](int image_row) __attribute__((always_inline)) {
        const int r = gmx4_sorted_row(sl.rbeg, image_row, sl.rend);
        return gather ? gather[r] : r;
    };

    // per-lane sources at K-step 0 (step s: + one K-step's bytes each)
    gmx4x_gptr wsrc[NW][kFp8aPiecesPerWave], wssrc[NW][2];
    const uint8_t *xsrc[kFp8aPiecesPerWave], *xssrc[2];
#pragma unroll
    for (int m = 0; m < NW; ++m) {
        const gmx4x_gptr codes = (gmx4x_gptr)(m == 0 ? Wt[sl.expert] : Wut[sl.expert]);
        const gmx4x_gptr exps = (gmx4x_gptr)(m == 0 ? Et[sl.expert] : Eut[sl.expert]);
#pragma unroll
        for (int i = 0; i < kFp8aPiecesPerWave; ++i) {
            const int p = fp8a_stage_piece(wave, i);
            wsrc[m][i] = codes + fp8a_src_off(n0, fp8a_stage_row(p, lane), N, ldw, 0, fp8a_stage_chunk(p, lane));
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) wssrc[m][tt] = exps + mxfp4x_scale_off(n0, fp8a_frag_row(wn, tt, lane), N, lds, 0);
    }
#pragma unroll
    for (int i = 0; i < kFp8aPiecesPerWave; ++i) {
        const int p = fp8a_stage_piece(wave, i);
        xsrc[i] = X4 + gmx4x_x_off(token(fp8a_stage_row(p, lane)), ldx4, 0, fp8a_stage_chunk(p, lane));
    }
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) xssrc[tt] = x_exp + gmx4x_xscale_off(token(fp8a_frag_row(wm, tt, lane)), ldxs, 0, 0);

    Gmx4xScales<NW> next;
    auto stage = [&](int s) __attribute__((always_inline)) {
        char* img = smem + gmx4x_stage_off(SW, s);
#pragma unroll
        for (int i = 0; i < kFp8aPiecesPerWave; ++i) {
            // the LDS address is the wave's piece base: the hardware adds 16 x lane
            const int lds_off = fp8a_stage_lds(fp8a_stage_piece(wave, i), 0);
#pragma unroll
            for (int m = 0; m < NW; ++m)
                __builtin_amdgcn_global_load_lds(wsrc[m][i] + (int64_t)s * kFp8aRowBytes,
                                                 (lds_void*)(img + gmx4x_w_img_off(m) + lds_off), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(xsrc[i] + (int64_t)s * kFp8aRowBytes,
                                             (lds_void*)(img + gmx4x_x_img_off(SW) + lds_off), 16, 0, 0);
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int d = 0; d < 2; ++d) {
#pragma unroll
                for (int m = 0; m < NW; ++m)
                    next.w[m][tt][d] = *(gmx4x_gptr32)(wssrc[m][tt] + (int64_t)s * kMxfp4xStepScales + 4 * d);
                next.x[tt][d] =
                    *reinterpret_cast<const uint32_t*>(xssrc[tt] + (int64_t)s * kMxfp4xStepScales + 4 * d);
            }
    };

    // fragment read offsets inside a stage: [tile][k-quarter]; the W offsets are relative to their image
    int wrd[2][kMxfp4xQuarters], xrd[2][kMxfp4xQuarters];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int q = 0; q < kMxfp4xQuarters; ++q) {
            wrd[tt][q] = fp8a_frag_lds(fp8a_frag_row(wn, tt, lane), mxfp4x_frag_chunk(q, lane));
            xrd[tt][q] = gmx4x_x_img_off(SW) + fp8a_frag_lds(fp8a_frag_row(wm, tt, lane), mxfp4x_frag_chunk(q, lane));
        }
    const int shift0 = mxfp4x_scale_shift(0, lane), shift1 = mxfp4x_scale_shift(1, lane);

    f32x16 acc[NW][2][2];  // [matrix][nt][mt]
#pragma unroll
    for (int m = 0; m < NW; ++m)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][nt][mt][r] = 0.f;

    stage(0);
    for (int s = 0; s < ks; ++s) {
        // step s has landed (this wave's pieces and scale dwords; the barrier covers the others' pieces), and
        // every wave is done reading the stage that step s + 1 overwrites
        gmx4x_wait<NW>(next);
        __syncthreads();
        const Gmx4xScales<NW> cur = next;
        if (s + 1 < ks) stage(s + 1);
        const char* img = smem + gmx4x_stage_off(SW, s);
#pragma unroll
        for (int q = 0; q < kMxfp4xQuarters; ++q) {
            const int shift = q & 1 ? shift1 : shift0, d = mxfp4x_scale_dword(q);
            i32x8 wf[NW][2], xf[2];
            int ws[NW][2], xs[2];  // byte 0 is the block's scale
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const i32x4 x = lds_read_b128(img, xrd[tt][q]);
                xf[tt] = i32x8{x.x, x.y, x.z, x.w, 0, 0, 0, 0};  // cbsz = blgp = 4 read the first four registers
                xs[tt] = (int)(cur.x[tt][d] >> shift);
#pragma unroll
                for (int m = 0; m < NW; ++m) {
                    const i32x4 w = lds_read_b128(img, gmx4x_w_img_off(m) + wrd[tt][q]);
                    wf[m][tt] = i32x8{w.x, w.y, w.z, w.w, 0, 0, 0, 0};
                    ws[m][tt] = (int)(cur.w[m][tt][d] >> shift);
                }
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int m = 0; m < NW; ++m)
                        // cbsz = 4: e2m1 A; blgp = 4: e2m1 B; both scales: byte 0 of the lane's register
                        acc[m][nt][mt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
                            wf[m][nt], xf[mt], acc[m][nt][mt], 4, 4, 0, ws[m][nt], 0, xs[mt]);
        }
    }

    // epilogue: a lane holds, per tile and register group g, 4 consecutive n of one sorted row
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int row = sl.rbeg + fp8a_acc_m(wm, mt, lane);
        if (row >= sl.rend) continue;
        const float xs = fp8_scale_of(x_scale, gather ? gather[row] : row);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ncol = n0 + fp8a_acc_n(wn, nt, lane, 4 * g);
                if (ncol >= N) continue;  // N % 4 == 0: the group is inside or outside as a whole
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v[r] = mxfp4a_finish(acc[0][nt][mt][4 * g + r], xs);
                    if constexpr (SW) v[r] = gmx4x_silu_mul(v[r], mxfp4a_finish(acc[NW - 1][nt][mt][4 * g + r], xs));
                }
                *reinterpret_cast<i32x2*>(C + gmx4_c_index(row, ncol, ldc)) =
                    i32x2{(int)pack2<T>(v[0], v[1]), (int)pack2<T>(v[2], v[3])};
            }
    }
}

// The kernel instances gemm_grouped_mxfp4_a4<T, SW>, one plain __global__ function each over the body above.
#define PLI_GMX4X_KERNEL(NAME, T, SW)                                                                              \
    __global__ __launch_bounds__(256) void NAME(                                                                   \
        const uint8_t* __restrict__ X4, const uint8_t* __restrict__ x_exp, const float* __restrict__ x_scale,      \
        const int32_t* __restrict__ gather, const uint8_t* const* __restrict__ Wt,                                 \
        const uint8_t* const* __restrict__ Et, const uint8_t* const* __restrict__ Wut,                             \
        const uint8_t* const* __restrict__ Eut, uint16_t* __restrict__ C, const int32_t* __restrict__ offsets,     \
        int E, int N, int ks, int64_t ldx4, int64_t ldxs, int64_t ldw, int64_t lds, int64_t ldc) {                 \
        gmx4x_body<T, SW>(X4, x_exp, x_scale, gather, Wt, Et, Wut, Eut, C, offsets, E, N, ks, ldx4, ldxs, ldw,     \
                          lds, ldc);                                                                               \
    }
PLI_GMX4X_KERNEL(gmx4x_bf16, bf16_t, false)
PLI_GMX4X_KERNEL(gmx4x_bf16_sw, bf16_t, true)
PLI_GMX4X_KERNEL(gmx4x_f16, f16_t, false)
PLI_GMX4X_KERNEL(gmx4x_f16_sw, f16_t, true)
#undef PLI_GMX4X_KERNEL

// ---------------------------------------------------------------------------
// gemm_grouped_mxfp4_a4_generic: one thread per element of [rows_bound, N];
// rows at and past offsets[E] belong to no expert and are left alone.  Decodes
// with the header codecs; fp32 fma in k order (K = 0: the sum is 0); the two
// block scales multiply exactly inside the contracts.  A 0xFF scale byte on
// either side decodes to NaN and poisons the sum.
template <typename T, bool SW>
__global__ __launch_bounds__(256) void gemm_grouped_mxfp4_a4_generic(
    const uint8_t* __restrict__ X4, const uint8_t* __restrict__ x_exp, const float* __restrict__ x_scale,
    const int32_t* __restrict__ gather, const uint8_t* const* __restrict__ Wt, const uint8_t* const* __restrict__ Et,
    const uint8_t* const* __restrict__ Wut, const uint8_t* const* __restrict__ Eut, T* __restrict__ C,
    const int32_t* __restrict__ offsets, int E, int rows_bound, int N, int K, int64_t ldx4, int64_t ldxs, int64_t ldw,
    int64_t lds, int64_t ldc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rows_bound * N) return;
    const int r = (int)(i / N), j = (int)(i % N);
    const int e = gmx4_expert_of(offsets, E, r);
    if (e < 0) return;
    const int t = gather ? gather[r] : r;
    const uint8_t* x = X4 + (int64_t)t * ldx4;
    const uint8_t* xe = x_exp + (int64_t)t * ldxs;
    auto dot = [&](const uint8_t* const* wt, const uint8_t* const* et) {  // K = 0: the tables may be NULL
        float sum = 0.f;
        const uint8_t* w = K ? wt[e] + (int64_t)j * ldw : nullptr;
        const uint8_t* we = K ? et[e] + (int64_t)j * lds : nullptr;
        for (int b = 0; b < K / kMxfp4aBlock; ++b) {
            const float scale = e8m0_decode(we[b]) * e8m0_decode(xe[b]);
            for (int kk = b * kMxfp4aBlock; kk < (b + 1) * kMxfp4aBlock; ++kk)
                sum = fmaf(fp4_e2m1_decode(fp4_nibble(x[kk >> 1], kk)),
                           fp4_e2m1_decode(fp4_nibble(w[kk >> 1], kk)) * scale, sum);
        }
        return mxfp4a_finish(sum, fp8_scale_of(x_scale, t));
    };
    float v = dot(Wt, Et);
    if constexpr (SW) v = gmx4x_silu_mul(v, dot(Wut, Eut));
    C[gmx4_c_index(r, j, ldc)] = elem<T>::from_f32(v);
}

// ------------------------------------------------------------------ launch --
struct Gmx4xArgs {
    const uint8_t *x4, *x_exp;
    const float* x_scale;
    const int32_t *gather, *offsets;
    const uint8_t *const *w, *const *we, *const *wu, *const *wue;
    void* c;
    int experts, rows_bound, n, k;
    int64_t ldx4, ldxs, ldw, lds, ldc;
};

using Gmx4xKernel = void (*)(const uint8_t*, const uint8_t*, const float*, const int32_t*, const uint8_t* const*,
                             const uint8_t* const*, const uint8_t* const*, const uint8_t* const*, uint16_t*,
                             const int32_t*, int, int, int, int64_t, int64_t, int64_t, int64_t, int64_t);

int launch_mx(const Gmx4xArgs& a, bool bf16, hipStream_t s) {
    static const Gmx4xKernel kernels[2][2] = {{gmx4x_f16, gmx4x_f16_sw}, {gmx4x_bf16, gmx4x_bf16_sw}};  // [bf16][SwiGLU]
    const dim3 grid((unsigned)fp8a_tiles(a.n, kGmx4TN), (unsigned)gmx4_slots(a.rows_bound, a.experts));
    hipLaunchKernelGGL(kernels[bf16][a.wu != nullptr], grid, dim3(256), 0, s, a.x4, a.x_exp, a.x_scale, a.gather, a.w,
                       a.we, a.wu, a.wue, (uint16_t*)a.c, a.offsets, a.experts, a.n, a.k / kMxfp4xKStep, a.ldx4,
                       a.ldxs, a.ldw, a.lds, a.ldc);
    return launch_status("gemm_grouped_mxfp4_a4");
}

template <typename T, bool SW>
int launch_generic(const Gmx4xArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((gemm_grouped_mxfp4_a4_generic<T, SW>), dim3((unsigned)gmx4_generic_blocks(a.rows_bound, a.n)),
                       dim3(256), 0, s, a.x4, a.x_exp, a.x_scale, a.gather, a.w, a.we, a.wu, a.wue, (T*)a.c,
                       a.offsets, a.experts, a.rows_bound, a.n, a.k, a.ldx4, a.ldxs, a.ldw, a.lds, a.ldc);
    return launch_status("gemm_grouped_mxfp4_a4_generic");
}

template <typename T>
int launch_generic_form(const Gmx4xArgs& a, hipStream_t s) {
    return a.wu ? launch_generic<T, true>(a, s) : launch_generic<T, false>(a, s);
}

}  // namespace
}  // namespace pli

extern "C" int pli_gemm_grouped_mxfp4_a4(const void* x4, const void* x_exp, const float* x_scale,
                                         const int32_t* gather, const void* const* w4_ptrs,
                                         const void* const* wexp_ptrs, const void* const* wu4_ptrs,
                                         const void* const* wuexp_ptrs, void* c, const int32_t* offsets, int experts,
                                         int rows_bound, int n, int k, int64_t ldx4, int64_t ldxs, int64_t ldw,
                                         int64_t lds, int64_t ldc, int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(dtype == PLI_F16 || dtype == PLI_BF16,
                "pli_gemm_grouped_mxfp4_a4: bad dtype %d (fp16 / bf16 output only)", dtype);
    PLI_REQUIRE(experts > 0 && rows_bound >= 0 && n >= 0 && k >= 0,
                "pli_gemm_grouped_mxfp4_a4: bad shape E=%d rows=%d n=%d k=%d", experts, rows_bound, n, k);
    PLI_REQUIRE(mxfp4a_shape_ok(k), "pli_gemm_grouped_mxfp4_a4: k=%d is not a multiple of the MX block of 32", k);
    PLI_REQUIRE(ldx4 >= k / 2 && ldxs >= k / kMxfp4aBlock && ldw >= k / 2 && lds >= k / kMxfp4aBlock && ldc >= n,
                "pli_gemm_grouped_mxfp4_a4: leading dimension too small (ldx4=%lld ldxs=%lld ldw=%lld lds=%lld "
                "ldc=%lld)",
                (long long)ldx4, (long long)ldxs, (long long)ldw, (long long)lds, (long long)ldc);
    if (rows_bound == 0 || n == 0) return PLI_OK;  // empty operands may be NULL
    PLI_REQUIRE(c && offsets && (k == 0 || (x4 && x_exp && w4_ptrs && wexp_ptrs)),
                "pli_gemm_grouped_mxfp4_a4: null pointer (the scale bytes have no default)");
    PLI_REQUIRE((wu4_ptrs != nullptr) == (wuexp_ptrs != nullptr),
                "pli_gemm_grouped_mxfp4_a4: the up tables come as a pair (codes and scale bytes, or neither)");
    const Gmx4xCall call{experts, rows_bound, n, k, ldx4, ldxs, ldw, lds, ldc, (uintptr_t)x4, (uintptr_t)x_exp,
                         (uintptr_t)c};
    const bool mx = gmx4x_route(call) == GMX4X_MX;
    PLI_REQUIRE(mx || gmx4_generic_blocks(rows_bound, n) <= 0x7fffffffLL,
                "pli_gemm_grouped_mxfp4_a4: grid too large");
    const Gmx4xArgs a{(const uint8_t*)x4, (const uint8_t*)x_exp, x_scale, gather, offsets,
                      (const uint8_t* const*)w4_ptrs, (const uint8_t* const*)wexp_ptrs,
                      (const uint8_t* const*)wu4_ptrs, (const uint8_t* const*)wuexp_ptrs, c, experts, rows_bound, n, k,
                      ldx4, ldxs, ldw, lds, ldc};
    hipStream_t s = (hipStream_t)stream;
    if (mx) return launch_mx(a, dtype == PLI_BF16, s);
    return dtype == PLI_BF16 ? launch_generic_form<bf16_t>(a, s) : launch_generic_form<f16_t>(a, s);
}
