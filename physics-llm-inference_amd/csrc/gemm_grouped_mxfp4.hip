// Grouped W4A8 GEMM over MoE experts on gfx950 (MI355X): fp8 e4m3 activation
// rows against each expert's MXFP4 weights (pli_gemm_grouped_mxfp4).  For
// every expert e and sorted row r in [offsets[e], offsets[e + 1]), t = gather ?
// gather[r] : r:
//   C[r, j] = round_T( x_scale[t] * sum_i decode_e4m3(X8[t, i]) * decode_e2m1(W4_e[j, i]) * 2^(w_exp_e[j, i/32] - 127) )
// or, with the up tables (fused SwiGLU over W1 / W3), g and u those two
// finished fp32 values, C[r, j] = round_T(silu(g) * u): SiLU and the product
// in fp32, one rounding.  No atomics, no workspace; offsets, gather and the
// pointer tables are read on the device, so a captured call replays.
//
// Kernels (index arithmetic and route: grouped_mxfp4_plan.h over
// mx_splitk_plan.h, checked on the CPU by tests/host/grouped_mxfp4_plan_check.cpp):
//   gemm_grouped_mxfp4<T, MC, SW>  one workgroup of four waves per (128 weight
//       rows, slot of 128 sorted rows); the slot's (expert, slab) comes from a
//       scan of the device offsets.  Wave w owns weight rows 32 w .. 32 w + 31
//       of the expert (SW: of its gate and its up matrix): their codes and
//       scale dwords go from global memory straight into double-buffered
//       operand registers, as in gemm_mx_splitk<MXSK_E2M1>.  X is the only LDS
//       traffic: three stages of the first 32 MC rows of gemm_fp8_mx's swizzled
//       image, fed by 16-byte LDS-DMA from the gathered rows.  MC (SW: 2 MC)
//       accumulators per wave; both values of a SwiGLU element sit in one lane.
//   gemm_grouped_mxfp4_generic<T, SW>  one thread per output element through
//       the header codecs, any shape, leading dimension and alignment
#include "fp4_codec.h"
#include "fp8_kv.h"
#include "grouped_mxfp4_plan.h"
#include "mx_finish.h"
#include "pli_common.h"

namespace pli {
namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;
// The experts' bases come out of the device pointer tables as generic pointers; the weights live in global memory,
// so the kernel says so: loads through these types are global_load (vmcnt only), not flat_load (vmcnt and lgkmcnt)
typedef const __attribute__((address_space(1))) uint8_t* gmx4_gptr;
typedef const __attribute__((address_space(1))) i32x4* gmx4_gptr128;
typedef const __attribute__((address_space(1))) uint32_t* gmx4_gptr32;

// gemm.hip's expression for the 16-bit grouped kernels
__device__ __forceinline__ float gmx4_silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

// the W operand registers of one K-step: per matrix (gate, up) the e2m1 chunk of each k-half and the scale dword
template <int NW> struct Gmx4W {
    i32x4 q[NW][2];
    uint32_t sc[NW];
};

// everything but the last N vector-memory operations of this wave has landed; the registers in flight pass
// through the statement, so nothing derived from them is scheduled in front of it
#define PLI_GMX4_WAIT(N_STR)                                                                                        \
    if constexpr (NW == 1)                                                                                          \
        asm volatile("s_waitcnt vmcnt(" N_STR ")" : "+v"(w.q[0][0]), "+v"(w.q[0][1]), "+v"(w.sc[0])::"memory");     \
    else                                                                                                            \
        asm volatile("s_waitcnt vmcnt(" N_STR ")"                                                                   \
                     : "+v"(w.q[0][0]), "+v"(w.q[0][1]), "+v"(w.sc[0]), "+v"(w.q[NW - 1][0]), "+v"(w.q[NW - 1][1]), \
                       "+v"(w.sc[NW - 1])::"memory")

template <int NW, int N> __device__ __forceinline__ void gmx4_wait_n(Gmx4W<NW>& w) {
    static_assert(N >= 0 && N <= 4, "one counted wait per MC");
    if constexpr (N == 0) { PLI_GMX4_WAIT("0"); }
    else if constexpr (N == 1) { PLI_GMX4_WAIT("1"); }
    else if constexpr (N == 2) { PLI_GMX4_WAIT("2"); }
    else if constexpr (N == 3) { PLI_GMX4_WAIT("3"); }
    else { PLI_GMX4_WAIT("4"); }
}
#undef PLI_GMX4_WAIT

// ---------------------------------------------------------------------------
// gemm_grouped_mxfp4.  Per K-step of 128 codes a wave issues its W loads for
// step s + 1 (per matrix two 16-byte loads and the scale dword) and its MC
// LDS-DMA pieces of X for step s + 2, then multiplies step s: per k-half one W
// operand per matrix against MC X fragments (two ds_read_b128 each, shared by
// gate and up).  Vector-memory operations are issued in the order
//   X(0) W(0) X(1) | W(1) X(2) | W(2) X(3) | ...
// so in front of step s exactly the MC pieces of X(s + 1) may still be in
// flight: one s_waitcnt vmcnt(MC) (vmcnt(0) on the last step) and one barrier
// per step.  The barrier also says every wave is done reading the stage of
// step s - 1, which is the one X(s + 2) overwrites.  As compiled, the loop head
// also carries a compiler-placed vmcnt(0) (where it copies next to cur), as in
// gemm_mx_splitk: the loads of step s are hidden under one step of MFMAs.
template <typename T, int MC, bool SW>
__device__ __forceinline__ void gmx4_body(
    const uint8_t* __restrict__ X8, const float* __restrict__ x_scale, const int32_t* __restrict__ gather,
    const uint8_t* const* __restrict__ Wt, const uint8_t* const* __restrict__ Et,
    const uint8_t* const* __restrict__ Wut, const uint8_t* const* __restrict__ Eut, uint16_t* __restrict__ C,
    const int32_t* __restrict__ offsets, int E, int N, int ks, int64_t ldx8, int64_t ldw, int64_t lds, int64_t ldc) {
    constexpr int NW = SW ? 2 : 1;
    constexpr int kStageBytes = MC * kMxskBlockBytes;
    __shared__ __attribute__((aligned(1024))) char smem[kMxskStages * kStageBytes];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n0 = blockIdx.x * kGmx4TN;
    const Gmx4Slab sl = gmx4_slab(offsets, E, blockIdx.y);
    if (sl.expert < 0) return;  // whole block: before any barrier

    // per-lane sources at K-step 0 (step s: + one K-step's bytes each); the source rows go through gather once
    const uint8_t* xsrc[MC];
#pragma unroll
    for (int i = 0; i < MC; ++i) {
        const int p = mxsk_x_piece(wave, i);
        const int r = gmx4_sorted_row(sl.rbeg, fp8a_stage_row(p, lane), sl.rend);
        xsrc[i] = X8 + gmx4_x_off(gather ? gather[r] : r, ldx8, 0, fp8a_stage_chunk(p, lane));
    }
    const int wrow = mxsk_w_row(wave, lane);
    gmx4_gptr wsrc[NW][2];
    gmx4_gptr ssrc[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const gmx4_gptr codes = (gmx4_gptr)(w == 0 ? Wt[sl.expert] : Wut[sl.expert]);
        const gmx4_gptr exps = (gmx4_gptr)(w == 0 ? Et[sl.expert] : Eut[sl.expert]);
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) wsrc[w][kh] = codes + mxsk_w_off(MXSK_E2M1, n0, wrow, N, ldw, 0, kh, lane, 0);
        ssrc[w] = exps + mxfp4a_scale_off(n0, wrow, N, lds, 0);
    }

    // the wave's MC LDS-DMA pieces of X for step S into stage BUF (the LDS address is the wave's piece base: the
    // hardware adds 16 x lane)
#define PLI_GMX4_STAGE_X(S, BUF)                                                                                    \
    _Pragma("unroll") for (int i = 0; i < MC; ++i) __builtin_amdgcn_global_load_lds(                                \
        xsrc[i] + (int64_t)(S) * kFp8aKStep,                                                                        \
        (lds_void*)(smem + (BUF) * kStageBytes + fp8a_stage_lds(mxsk_x_piece(wave, i), 0)), 16, 0, 0)
    auto load_w = [&](Gmx4W<NW>& w, int s) __attribute__((always_inline)) {
#pragma unroll
        for (int m = 0; m < NW; ++m) {
#pragma unroll
            for (int kh = 0; kh < 2; ++kh)
                w.q[m][kh] = *(gmx4_gptr128)(wsrc[m][kh] + (int64_t)s * kMxfp4aWRowBytes);
            w.sc[m] = *(gmx4_gptr32)(ssrc[m] + (int64_t)s * (kMxfp4aKStep / kMxfp4aBlock));
        }
    };

    // X fragment read offsets inside a stage: [m block][k-half][16-byte half], the halves crosswise
    int xrd[MC][2][2];
#pragma unroll
    for (int b = 0; b < MC; ++b)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int h = 0; h < 2; ++h)
                xrd[b][kh][h] = fp8a_frag_lds(mxsk_x_row(b, lane), mxsk_x_chunk(MXSK_E2M1, kh, lane, h));
    const int shift0 = mxfp4a_scale_shift(0, lane), shift1 = mxfp4a_scale_shift(1, lane);

    f32x16 acc[NW][MC];
#pragma unroll
    for (int m = 0; m < NW; ++m)
#pragma unroll
        for (int b = 0; b < MC; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][b][r] = 0.f;

    Gmx4W<NW> next, cur;
    int buf = 0;  // the stage of step s
    // One K-step is begin(more_w); [the X pieces of step s + 2]; multiply().  more_w: step s + 1 exists, so X(s + 1) is
    // in flight in front of the wait and W(s + 1) is loaded.  The flag is a literal at every call and the lambdas
    // are inlined, so every path through the steps has one fixed issue order.
    auto begin = [&](int s, bool more_w) __attribute__((always_inline)) {
        if (more_w) gmx4_wait_n<NW, MC>(next);
        else gmx4_wait_n<NW, 0>(next);
        __builtin_amdgcn_s_barrier();
        cur = next;
        if (more_w) load_w(next, s + 1);
        __builtin_amdgcn_sched_barrier(0);  // the W loads stay in front of the X pieces: the count relies on it
    };
    auto multiply = [&]() __attribute__((always_inline)) {
        const char* img = smem + buf * kStageBytes;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            i32x8 wf[NW];
            int sc[NW];
#pragma unroll
            for (int m = 0; m < NW; ++m) {
                wf[m] = i32x8{cur.q[m][kh].x, cur.q[m][kh].y, cur.q[m][kh].z, cur.q[m][kh].w, 0, 0, 0, 0};  // cbsz = 4
                sc[m] = (int)(cur.sc[m] >> (kh ? shift1 : shift0));  // byte 0 is the block's scale
            }
#pragma unroll
            for (int b = 0; b < MC; ++b) {
                const i32x4 xl = lds_read_b128(img, xrd[b][kh][0]), xh = lds_read_b128(img, xrd[b][kh][1]);
                const i32x8 xf = i32x8{xl.x, xl.y, xl.z, xl.w, xh.x, xh.y, xh.z, xh.w};
#pragma unroll
                for (int m = 0; m < NW; ++m)
                    // A = W e2m1 (cbsz 4), its scale byte 0 of the lane's register; B = X e4m3 at 2^0
                    acc[m][b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[m], xf, acc[m][b], 4, 0, 0, sc[m], 0, 127);
            }
        }
        buf = buf + 1 < kMxskStages ? buf + 1 : 0;
    };
    PLI_GMX4_STAGE_X(0, 0);
    load_w(next, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (ks == 1) {
        begin(0, false);
        multiply();
    } else {
        PLI_GMX4_STAGE_X(1, 1);
        int s = 0;
        for (; s + 2 < ks; ++s) {
            begin(s, true);
            PLI_GMX4_STAGE_X(s + 2, buf >= 1 ? buf - 1 : kMxskStages - 1);  // stage (buf + 2) % 3: step s - 1's, read by all
            multiply();
        }
        begin(s, true);
        multiply();
        begin(s + 1, false);
        multiply();
    }
#undef PLI_GMX4_STAGE_X

    // epilogue: a lane holds, per m block and register group g, 4 consecutive n of one sorted row
#pragma unroll
    for (int b = 0; b < MC; ++b) {
        const int row = sl.rbeg + mxsk_acc_m(b, lane);
        if (row >= sl.rend) continue;
        const float xs = fp8_scale_of(x_scale, gather ? gather[row] : row);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ncol = n0 + mxsk_acc_n(wave, lane, 4 * g);
            if (ncol >= N) continue;  // N % 4 == 0: the group is inside or outside as a whole
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = mxfp4a_finish(acc[0][b][4 * g + r], xs);
                if constexpr (SW) v[r] = gmx4_silu_mul(v[r], mxfp4a_finish(acc[NW - 1][b][4 * g + r], xs));
            }
            *reinterpret_cast<i32x2*>(C + gmx4_c_index(row, ncol, ldc)) =
                i32x2{(int)pack2<T>(v[0], v[1]), (int)pack2<T>(v[2], v[3])};
        }
    }
}

// The kernel instances gemm_grouped_mxfp4<T, MC, SW>, one plain __global__ function each over the body above.
#define PLI_GMX4_KERNEL(NAME, T, MC, SW)                                                                            \
    __global__ __launch_bounds__(256) void NAME(                                                                    \
        const uint8_t* __restrict__ X8, const float* __restrict__ x_scale, const int32_t* __restrict__ gather,      \
        const uint8_t* const* __restrict__ Wt, const uint8_t* const* __restrict__ Et,                               \
        const uint8_t* const* __restrict__ Wut, const uint8_t* const* __restrict__ Eut, uint16_t* __restrict__ C,   \
        const int32_t* __restrict__ offsets, int E, int N, int ks, int64_t ldx8, int64_t ldw, int64_t lds,          \
        int64_t ldc) {                                                                                              \
        gmx4_body<T, MC, SW>(X8, x_scale, gather, Wt, Et, Wut, Eut, C, offsets, E, N, ks, ldx8, ldw, lds, ldc);     \
    }
#define PLI_GMX4_KERNELS(TAG, T)                         \
    PLI_GMX4_KERNEL(gmx4_##TAG##_mc1, T, 1, false)       \
    PLI_GMX4_KERNEL(gmx4_##TAG##_mc2, T, 2, false)       \
    PLI_GMX4_KERNEL(gmx4_##TAG##_mc3, T, 3, false)       \
    PLI_GMX4_KERNEL(gmx4_##TAG##_mc4, T, 4, false)       \
    PLI_GMX4_KERNEL(gmx4_##TAG##_mc1_sw, T, 1, true)     \
    PLI_GMX4_KERNEL(gmx4_##TAG##_mc2_sw, T, 2, true)     \
    PLI_GMX4_KERNEL(gmx4_##TAG##_mc3_sw, T, 3, true)     \
    PLI_GMX4_KERNEL(gmx4_##TAG##_mc4_sw, T, 4, true)
PLI_GMX4_KERNELS(bf16, bf16_t)
PLI_GMX4_KERNELS(f16, f16_t)
#undef PLI_GMX4_KERNELS
#undef PLI_GMX4_KERNEL

// ---------------------------------------------------------------------------
// gemm_grouped_mxfp4_generic: one thread per element of [rows_bound, N]; rows
// at and past offsets[E] belong to no expert and are left alone.  Decodes with
// the header codecs; fp32 fma in k order (K = 0: the sum is 0).  A 0xFF scale
// byte decodes to NaN and poisons the sum.
template <typename T, bool SW>
__global__ __launch_bounds__(256) void gemm_grouped_mxfp4_generic(
    const uint8_t* __restrict__ X8, const float* __restrict__ x_scale, const int32_t* __restrict__ gather,
    const uint8_t* const* __restrict__ Wt, const uint8_t* const* __restrict__ Et,
    const uint8_t* const* __restrict__ Wut, const uint8_t* const* __restrict__ Eut, T* __restrict__ C,
    const int32_t* __restrict__ offsets, int E, int rows_bound, int N, int K, int64_t ldx8, int64_t ldw, int64_t lds,
    int64_t ldc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rows_bound * N) return;
    const int r = (int)(i / N), j = (int)(i % N);
    const int e = gmx4_expert_of(offsets, E, r);
    if (e < 0) return;
    const int t = gather ? gather[r] : r;
    const uint8_t* x = X8 + (int64_t)t * ldx8;
    auto dot = [&](const uint8_t* const* wt, const uint8_t* const* et) {  // K = 0: the tables may be NULL
        float sum = 0.f;
        const uint8_t* w = K ? wt[e] + (int64_t)j * ldw : nullptr;
        const uint8_t* ex = K ? et[e] + (int64_t)j * lds : nullptr;
        for (int b = 0; b < K / kMxfp4aBlock; ++b) {
            const float scale = e8m0_decode(ex[b]);
            for (int kk = b * kMxfp4aBlock; kk < (b + 1) * kMxfp4aBlock; ++kk)
                sum = fmaf(fp8_e4m3_decode(x[kk]), fp4_e2m1_decode(fp4_nibble(w[kk >> 1], kk)) * scale, sum);
        }
        return mxfp4a_finish(sum, fp8_scale_of(x_scale, t));
    };
    float v = dot(Wt, Et);
    if constexpr (SW) v = gmx4_silu_mul(v, dot(Wut, Eut));
    C[gmx4_c_index(r, j, ldc)] = elem<T>::from_f32(v);
}

// ------------------------------------------------------------------ launch --
struct Gmx4Args {
    const uint8_t* x8;
    const float* x_scale;
    const int32_t *gather, *offsets;
    const uint8_t *const *w, *const *we, *const *wu, *const *wue;
    void* c;
    int experts, rows_bound, n, k;
    int64_t ldx8, ldw, lds, ldc;
};

using Gmx4Kernel = void (*)(const uint8_t*, const float*, const int32_t*, const uint8_t* const*, const uint8_t* const*,
                            const uint8_t* const*, const uint8_t* const*, uint16_t*, const int32_t*, int, int, int, int64_t,
                            int64_t, int64_t, int64_t);

int launch_mx(const Gmx4Args& a, bool bf16, hipStream_t s) {
    static const Gmx4Kernel kernels[2][2][kMxskMaxMC] = {  // [bf16][SwiGLU][MC - 1]
        {{gmx4_f16_mc1, gmx4_f16_mc2, gmx4_f16_mc3, gmx4_f16_mc4},
         {gmx4_f16_mc1_sw, gmx4_f16_mc2_sw, gmx4_f16_mc3_sw, gmx4_f16_mc4_sw}},
        {{gmx4_bf16_mc1, gmx4_bf16_mc2, gmx4_bf16_mc3, gmx4_bf16_mc4},
         {gmx4_bf16_mc1_sw, gmx4_bf16_mc2_sw, gmx4_bf16_mc3_sw, gmx4_bf16_mc4_sw}}};
    const dim3 grid((unsigned)fp8a_tiles(a.n, kGmx4TN), (unsigned)gmx4_slots(a.rows_bound, a.experts));
    hipLaunchKernelGGL(kernels[bf16][a.wu != nullptr][gmx4_mc(a.rows_bound) - 1], grid, dim3(256), 0, s, a.x8,
                       a.x_scale, a.gather, a.w, a.we, a.wu, a.wue, (uint16_t*)a.c, a.offsets, a.experts, a.n,
                       a.k / kMxfp4aKStep, a.ldx8, a.ldw, a.lds, a.ldc);
    return launch_status("gemm_grouped_mxfp4");
}

template <typename T, bool SW>
int launch_generic(const Gmx4Args& a, hipStream_t s) {
    hipLaunchKernelGGL((gemm_grouped_mxfp4_generic<T, SW>), dim3((unsigned)gmx4_generic_blocks(a.rows_bound, a.n)),
                       dim3(256), 0, s, a.x8, a.x_scale, a.gather, a.w, a.we, a.wu, a.wue, (T*)a.c, a.offsets,
                       a.experts, a.rows_bound, a.n, a.k, a.ldx8, a.ldw, a.lds, a.ldc);
    return launch_status("gemm_grouped_mxfp4_generic");
}

template <typename T>
int launch_generic_form(const Gmx4Args& a, hipStream_t s) {
    return a.wu ? launch_generic<T, true>(a, s) : launch_generic<T, false>(a, s);
}

}  // namespace
}  // namespace pli

extern "C" int pli_gemm_grouped_mxfp4(const void* x8, const float* x_scale, const int32_t* gather,
                                      const void* const* w4_ptrs, const void* const* wexp_ptrs,
                                      const void* const* wu4_ptrs, const void* const* wuexp_ptrs, void* c,
                                      const int32_t* offsets, int experts, int rows_bound, int n, int k, int64_t ldx8,
                                      int64_t ldw, int64_t lds, int64_t ldc, int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(dtype == PLI_F16 || dtype == PLI_BF16, "pli_gemm_grouped_mxfp4: bad dtype %d (fp16 / bf16 output only)",
                dtype);
    PLI_REQUIRE(experts > 0 && rows_bound >= 0 && n >= 0 && k >= 0,
                "pli_gemm_grouped_mxfp4: bad shape E=%d rows=%d n=%d k=%d", experts, rows_bound, n, k);
    PLI_REQUIRE(mxfp4a_shape_ok(k), "pli_gemm_grouped_mxfp4: k=%d is not a multiple of the MX block of 32", k);
    PLI_REQUIRE(ldx8 >= k && ldw >= k / 2 && lds >= k / kMxfp4aBlock && ldc >= n,
                "pli_gemm_grouped_mxfp4: leading dimension too small (ldx8=%lld ldw=%lld lds=%lld ldc=%lld)",
                (long long)ldx8, (long long)ldw, (long long)lds, (long long)ldc);
    if (rows_bound == 0 || n == 0) return PLI_OK;  // empty operands may be NULL
    PLI_REQUIRE(c && offsets && (k == 0 || (x8 && w4_ptrs && wexp_ptrs)),
                "pli_gemm_grouped_mxfp4: null pointer (the scale bytes have no default)");
    PLI_REQUIRE((wu4_ptrs != nullptr) == (wuexp_ptrs != nullptr),
                "pli_gemm_grouped_mxfp4: the up tables come as a pair (codes and scale bytes, or neither)");
    const Gmx4Call call{experts, rows_bound, n, k, ldx8, ldw, lds, ldc, (uintptr_t)x8, (uintptr_t)c};
    const bool mx = gmx4_route(call) == GMX4_MX;
    PLI_REQUIRE(mx || gmx4_generic_blocks(rows_bound, n) <= 0x7fffffffLL, "pli_gemm_grouped_mxfp4: grid too large");
    const Gmx4Args a{(const uint8_t*)x8, x_scale, gather, offsets, (const uint8_t* const*)w4_ptrs,
                     (const uint8_t* const*)wexp_ptrs, (const uint8_t* const*)wu4_ptrs,
                     (const uint8_t* const*)wuexp_ptrs, c, experts, rows_bound, n, k, ldx8, ldw, lds, ldc};
    hipStream_t s = (hipStream_t)stream;
    if (mx) return launch_mx(a, dtype == PLI_BF16, s);
    return dtype == PLI_BF16 ? launch_generic_form<bf16_t>(a, s) : launch_generic_form<f16_t>(a, s);
}
