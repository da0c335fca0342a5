// Split-K grouped W4A8 GEMM for MoE decode on gfx950 (MI355X): at most 32
// sorted rows (1 .. 16 tokens at top-2) of fp8 e4m3 activations against the
// experts' MXFP4 weights, with a caller workspace (pli_gemm_grouped_mxfp4_ws).
// At so few rows the layer only streams weights, and only the two or so experts
// that have rows: gemm_grouped_mxfp4 gives them 64 workgroups, each walking K
// alone with one K-step of loads in flight.  Here every (128 weight rows,
// K chunk, expert) is a workgroup, a workgroup puts the W loads of its whole
// chunk in flight before its first MFMA, and a second kernel sums the fp32
// partials in chunk order and finishes them exactly as gemm_grouped_mxfp4
// finishes its sums.  No atomics; offsets, gather and the pointer tables are
// read on the device, so a captured call replays.
//
// Kernels (index arithmetic, route and split rule: grouped_mxfp4_splitk_plan.h,
// checked on the CPU by tests/host/grouped_mxfp4_splitk_plan_check.cpp):
//   gemm_grouped_mxfp4_splitk<SW>        partial of 128 weight rows (SW: of the
//       gate and of the up matrix) x the expert's rows over one K chunk on
//       v_mfma_scale_f32_32x32x64_f8f6f4.  A chunk runs in passes of up to 8
//       K-steps.  A pass first stages its whole X (one 4 KiB image per K-step,
//       16-byte LDS-DMA from the gathered rows) and issues every W load of its
//       steps straight into operand registers, then waits for X alone, meets
//       one barrier, and multiplies step after step as the W registers land:
//       no barrier, no X traffic and no load in the multiply sequence.
//   gemm_grouped_mxfp4_splitk_reduce<T, SW>  one thread per 4 n of one sorted
//       row: partials summed in chunk order, mxfp4a_finish, SwiGLU in fp32,
//       one rounding
#include "fp8_kv.h"
#include "grouped_mxfp4_splitk_plan.h"
#include "mx_finish.h"
#include "pli_common.h"

namespace pli {
namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;
// the weights live in global memory and the kernel says so: global_load (vmcnt only), not flat_load
typedef const __attribute__((address_space(1))) uint8_t* gsk4_gptr;
typedef const __attribute__((address_space(1))) i32x4* gsk4_gptr128;
typedef const __attribute__((address_space(1))) uint32_t* gsk4_gptr32;

// gemm.hip's expression for the 16-bit grouped kernels
__device__ __forceinline__ float gsk4_silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

// the W operand registers of one K-step: per matrix (gate, up) the e2m1 chunk of each k-half and the scale dword
template <int NW> struct Gsk4W {
    i32x4 q[NW][2];
    uint32_t sc[NW];
};

// the s_waitcnt immediate of gfx9 for vmcnt(n), lgkmcnt(0), expcnt untouched: vmcnt in bits 3:0 and 15:14, expcnt
// 6:4, lgkmcnt 11:8
constexpr int gsk4_waitcnt_vm(int n) { return (n & 15) | ((n >> 4) << 14) | (7 << 4); }

// what a pass needs besides its step range: per-lane sources at K-step 0 of the operand and the fragment offsets
template <int NW> struct Gsk4Lane {
    const uint8_t* xsrc;  // the lane's 16 bytes of the wave's X piece
    gsk4_gptr wsrc[NW][2];
    gsk4_gptr ssrc[NW];
    int xrd[2][2];  // X fragment offsets inside an image: [k-half][16-byte half], the halves crosswise
    int shift0, shift1;
};

// ---------------------------------------------------------------------------
// One pass of LEN K-steps from absolute step `step0`.  Vector-memory operations
// of a wave, in issue order: LEN LDS-DMA pieces of X, then kGsk4WLoads NW LEN W
// loads.  The counter retires in order, so vmcnt(kGsk4WLoads NW LEN) says the
// wave's X pieces have landed while every W load may still be in flight; after
// the barrier all four waves' pieces are there.  The multiply sequence is
// straight-line code over registers, so the compiler's own counted waits in
// front of step i are vmcnt(kGsk4WLoads NW (LEN - 1 - i)): descending, 0 only at
// the last step.
template <int NW, int LEN>
__device__ __forceinline__ void gsk4_pass(const Gsk4Lane<NW>& ln, char* smem, int wave, int step0, f32x16 (&acc)[NW]) {
    static_assert(kGsk4WLoads * NW * kGsk4StageSteps < 64 && LEN <= kGsk4StageSteps, "vmcnt holds 6 bits");
#pragma unroll
    for (int i = 0; i < LEN; ++i)  // the LDS address is the wave's piece base: the hardware adds 16 x lane
        __builtin_amdgcn_global_load_lds(ln.xsrc + (int64_t)(step0 + i) * kFp8aKStep,
                                         (lds_void*)(smem + gsk4_stage_lds(i, wave, 0)), 16, 0, 0);
    __builtin_amdgcn_sched_barrier(0);  // X in front of W: the count relies on it
    Gsk4W<NW> w[LEN];
#pragma unroll
    for (int i = 0; i < LEN; ++i)
#pragma unroll
        for (int m = 0; m < NW; ++m) {
#pragma unroll
            for (int kh = 0; kh < 2; ++kh)
                w[i].q[m][kh] = *(gsk4_gptr128)(ln.wsrc[m][kh] + (int64_t)(step0 + i) * kMxfp4aWRowBytes);
            w[i].sc[m] = *(gsk4_gptr32)(ln.ssrc[m] + (int64_t)(step0 + i) * (kMxfp4aKStep / kMxfp4aBlock));
        }
    __builtin_amdgcn_sched_barrier(0);  // every load of the pass is issued before the first MFMA
    // The wait is the builtin, not inline assembly, so that the compiler's own counter model sees it: while it
    // believes an LDS-DMA may be pending it turns every later counted wait into vmcnt(0).  lgkmcnt(0) belongs to
    // the same model (an LDS-DMA is a load and an LDS access to it) and costs nothing here.
    __builtin_amdgcn_s_waitcnt(gsk4_waitcnt_vm(kGsk4WLoads * NW * LEN));
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int i = 0; i < LEN; ++i)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            const i32x4 xl = lds_read_b128(smem, i * kGsk4ImgBytes + ln.xrd[kh][0]);
            const i32x4 xh = lds_read_b128(smem, i * kGsk4ImgBytes + ln.xrd[kh][1]);
            const i32x8 xf = i32x8{xl.x, xl.y, xl.z, xl.w, xh.x, xh.y, xh.z, xh.w};
#pragma unroll
            for (int m = 0; m < NW; ++m) {
                const i32x4 q = w[i].q[m][kh];
                const i32x8 wf = i32x8{q.x, q.y, q.z, q.w, 0, 0, 0, 0};                // cbsz = 4: four registers
                const int sc = (int)(w[i].sc[m] >> (kh ? ln.shift1 : ln.shift0));  // byte 0 is the block's scale
                // A = W e2m1 (cbsz 4), its scale byte 0 of the lane's register; B = X e4m3 at 2^0
                acc[m] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf, xf, acc[m], 4, 0, 0, sc, 0, 127);
            }
        }
}

template <bool SW>
__global__ __launch_bounds__(256) void gemm_grouped_mxfp4_splitk(
    const uint8_t* __restrict__ X8, const int32_t* __restrict__ gather, const uint8_t* const* __restrict__ Wt,
    const uint8_t* const* __restrict__ Et, const uint8_t* const* __restrict__ Wut,
    const uint8_t* const* __restrict__ Eut, float* __restrict__ ws, const int32_t* __restrict__ offsets,
    int rows_bound, int N, int ks, int per, int64_t ldx8, int64_t ldw, int64_t lds) {
    constexpr int NW = SW ? 2 : 1;
    __shared__ __attribute__((aligned(1024))) char smem[kGsk4LdsBytes];
    const int e = blockIdx.z;
    const int rbeg = offsets[e], rend = offsets[e + 1];
    if (rbeg >= rend) return;  // whole block: before any barrier, table entry or load
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n0 = blockIdx.x * kGmx4TN, c = blockIdx.y;
    const int s0 = mxsk_chunk_begin(c, per), len = mxsk_chunk_end(c, per, ks) - s0;

    Gsk4Lane<NW> ln;
    {  // the source row goes through gather once
        const int r = gmx4_sorted_row(rbeg, fp8a_stage_row(wave, lane), rend);
        ln.xsrc = X8 + gmx4_x_off(gather ? gather[r] : r, ldx8, 0, fp8a_stage_chunk(wave, lane));
    }
    const int wrow = mxsk_w_row(wave, lane);
#pragma unroll
    for (int m = 0; m < NW; ++m) {
        const gsk4_gptr codes = (gsk4_gptr)(m == 0 ? Wt[e] : Wut[e]);
        const gsk4_gptr exps = (gsk4_gptr)(m == 0 ? Et[e] : Eut[e]);
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) ln.wsrc[m][kh] = codes + mxsk_w_off(MXSK_E2M1, n0, wrow, N, ldw, 0, kh, lane, 0);
        ln.ssrc[m] = exps + mxfp4a_scale_off(n0, wrow, N, lds, 0);
    }
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int h = 0; h < 2; ++h)
            ln.xrd[kh][h] = fp8a_frag_lds(mxsk_x_row(0, lane), mxsk_x_chunk(MXSK_E2M1, kh, lane, h));
    ln.shift0 = mxfp4a_scale_shift(0, lane);
    ln.shift1 = mxfp4a_scale_shift(1, lane);

    f32x16 acc[NW];
#pragma unroll
    for (int m = 0; m < NW; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

    for (int p = 0; p < gsk4_passes(len); ++p) {
        if (p) __builtin_amdgcn_s_barrier();  // every wave is done reading the stage the next fill overwrites
        const int first = s0 + p * kGsk4StageSteps;
        switch (gsk4_pass_len(len, p)) {  // uniform: one unrolled sequence per length
            case 1: gsk4_pass<NW, 1>(ln, smem, wave, first, acc); break;
            case 2: gsk4_pass<NW, 2>(ln, smem, wave, first, acc); break;
            case 3: gsk4_pass<NW, 3>(ln, smem, wave, first, acc); break;
            case 4: gsk4_pass<NW, 4>(ln, smem, wave, first, acc); break;
            case 5: gsk4_pass<NW, 5>(ln, smem, wave, first, acc); break;
            case 6: gsk4_pass<NW, 6>(ln, smem, wave, first, acc); break;
            case 7: gsk4_pass<NW, 7>(ln, smem, wave, first, acc); break;
            default: gsk4_pass<NW, 8>(ln, smem, wave, first, acc); break;
        }
    }

    // the partial as it is: a lane holds, per matrix and register group g, 4 consecutive n of one sorted row
    const int row = rbeg + mxsk_acc_m(0, lane);
    if (row >= rend || row >= rows_bound) return;
#pragma unroll
    for (int m = 0; m < NW; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ncol = n0 + mxsk_acc_n(wave, lane, 4 * g);
            if (ncol >= N) continue;  // N % 4 == 0: the group is inside or outside as a whole
            *reinterpret_cast<f32x4*>(ws + gsk4_ws_index(c, row, m, ncol, rows_bound, N, NW)) =
                f32x4{acc[m][4 * g], acc[m][4 * g + 1], acc[m][4 * g + 2], acc[m][4 * g + 3]};
        }
}

// ---------------------------------------------------------------------------
// gemm_grouped_mxfp4_splitk_reduce: partials summed in the order c = 0 .. S - 1,
// then gemm_grouped_mxfp4's epilogue: mxfp4a_finish with the token's row scale,
// SiLU and the product in fp32, one rounding and one 8-byte store.
template <typename T, bool SW>
__global__ __launch_bounds__(kMxskReduceThreads) void gemm_grouped_mxfp4_splitk_reduce(
    const float* __restrict__ ws, const float* __restrict__ x_scale, const int32_t* __restrict__ gather,
    uint16_t* __restrict__ C, const int32_t* __restrict__ offsets, int E, int rows_bound, int N, int S, int64_t ldc) {
    constexpr int NW = SW ? 2 : 1;
    const int64_t i = (int64_t)blockIdx.x * kMxskReduceThreads + threadIdx.x;
    if (i >= mxsk_reduce_items(rows_bound, N)) return;
    const int r = gsk4_reduce_row(i, N), j = gsk4_reduce_col(i, N);
    if (r >= offsets[E]) return;  // no expert's row: left alone
    f32x4 sum[NW];
#pragma unroll
    for (int m = 0; m < NW; ++m) {
        sum[m] = *reinterpret_cast<const f32x4*>(ws + gsk4_ws_index(0, r, m, j, rows_bound, N, NW));
        for (int c = 1; c < S; ++c)
            sum[m] += *reinterpret_cast<const f32x4*>(ws + gsk4_ws_index(c, r, m, j, rows_bound, N, NW));
    }
    const float xs = fp8_scale_of(x_scale, gather ? gather[r] : r);
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v[q] = mxfp4a_finish(sum[0][q], xs);
        if constexpr (SW) v[q] = gsk4_silu_mul(v[q], mxfp4a_finish(sum[NW - 1][q], xs));
    }
    *reinterpret_cast<i32x2*>(C + gmx4_c_index(r, j, ldc)) = i32x2{(int)pack2<T>(v[0], v[1]), (int)pack2<T>(v[2], v[3])};
}

// ------------------------------------------------------------------ launch --
struct Gsk4Args {
    const uint8_t* x8;
    const float* x_scale;
    const int32_t *gather, *offsets;
    const uint8_t *const *w, *const *we, *const *wu, *const *wue;
    void* c;
    float* ws;
    int experts, rows_bound, n, k;
    int64_t ldx8, ldw, lds, ldc;
};

template <typename T, bool SW>
int launch_splitk(const Gsk4Args& a, const Gsk4Plan& p, hipStream_t s) {
    const dim3 grid((unsigned)fp8a_tiles(a.n, kGmx4TN), (unsigned)p.splits, (unsigned)a.experts);
    hipLaunchKernelGGL((gemm_grouped_mxfp4_splitk<SW>), grid, dim3(256), 0, s, a.x8, a.gather, a.w, a.we, a.wu, a.wue,
                       a.ws, a.offsets, a.rows_bound, a.n, a.k / kMxfp4aKStep, p.per, a.ldx8, a.ldw, a.lds);
    if (const int rc = launch_status("gemm_grouped_mxfp4_splitk")) return rc;
    hipLaunchKernelGGL((gemm_grouped_mxfp4_splitk_reduce<T, SW>), dim3((unsigned)mxsk_reduce_blocks(a.rows_bound, a.n)),
                       dim3(kMxskReduceThreads), 0, s, a.ws, a.x_scale, a.gather, (uint16_t*)a.c, a.offsets, a.experts,
                       a.rows_bound, a.n, p.splits, a.ldc);
    return launch_status("gemm_grouped_mxfp4_splitk_reduce");
}

}  // namespace
}  // namespace pli

extern "C" size_t pli_gemm_grouped_mxfp4_workspace_size(int experts, int rows_bound, int n, int k, int swiglu,
                                                        int splits) {
    return pli::gsk4_workspace_size(experts, rows_bound, n, k, swiglu, splits);
}

extern "C" int pli_gemm_grouped_mxfp4_ws(const void* x8, const float* x_scale, const int32_t* gather,
                                         const void* const* w4_ptrs, const void* const* wexp_ptrs,
                                         const void* const* wu4_ptrs, const void* const* wuexp_ptrs, void* c,
                                         const int32_t* offsets, int experts, int rows_bound, int n, int k,
                                         int64_t ldx8, int64_t ldw, int64_t lds, int64_t ldc, int dtype,
                                         void* workspace, size_t workspace_bytes, int splits, void* stream) {
    using namespace pli;
    clear_error();
    // pli_gemm_grouped_mxfp4's rules in its order, then splits
    PLI_REQUIRE(dtype == PLI_F16 || dtype == PLI_BF16,
                "pli_gemm_grouped_mxfp4_ws: bad dtype %d (fp16 / bf16 output only)", dtype);
    PLI_REQUIRE(experts > 0 && rows_bound >= 0 && n >= 0 && k >= 0,
                "pli_gemm_grouped_mxfp4_ws: bad shape E=%d rows=%d n=%d k=%d", experts, rows_bound, n, k);
    PLI_REQUIRE(mxfp4a_shape_ok(k), "pli_gemm_grouped_mxfp4_ws: k=%d is not a multiple of the MX block of 32", k);
    PLI_REQUIRE(ldx8 >= k && ldw >= k / 2 && lds >= k / kMxfp4aBlock && ldc >= n,
                "pli_gemm_grouped_mxfp4_ws: leading dimension too small (ldx8=%lld ldw=%lld lds=%lld ldc=%lld)",
                (long long)ldx8, (long long)ldw, (long long)lds, (long long)ldc);
    const Gmx4Call call{experts, rows_bound, n, k, ldx8, ldw, lds, ldc, (uintptr_t)x8, (uintptr_t)c};
    const bool mx = gmx4_route(call) == GMX4_MX;
    if (rows_bound != 0 && n != 0) {  // empty operands may be NULL
        PLI_REQUIRE(c && offsets && (k == 0 || (x8 && w4_ptrs && wexp_ptrs)),
                    "pli_gemm_grouped_mxfp4_ws: null pointer (the scale bytes have no default)");
        PLI_REQUIRE((wu4_ptrs != nullptr) == (wuexp_ptrs != nullptr),
                    "pli_gemm_grouped_mxfp4_ws: the up tables come as a pair (codes and scale bytes, or neither)");
        PLI_REQUIRE(mx || gmx4_generic_blocks(rows_bound, n) <= 0x7fffffffLL,
                    "pli_gemm_grouped_mxfp4_ws: grid too large");
    }
    PLI_REQUIRE(splits >= 0, "pli_gemm_grouped_mxfp4_ws: bad splits %d (0: the rule chooses, >= 1: forced)", splits);
    if (rows_bound == 0 || n == 0) return PLI_OK;
    const Gsk4Plan p = gsk4_plan(mx, experts, rows_bound, n, k, wu4_ptrs != nullptr, splits, (uintptr_t)workspace,
                                 workspace_bytes);
    if (p.splits < 2)
        return pli_gemm_grouped_mxfp4(x8, x_scale, gather, w4_ptrs, wexp_ptrs, wu4_ptrs, wuexp_ptrs, c, offsets, experts,
                                      rows_bound, n, k, ldx8, ldw, lds, ldc, dtype, stream);
    const Gsk4Args a{(const uint8_t*)x8, x_scale, gather, offsets, (const uint8_t* const*)w4_ptrs,
                     (const uint8_t* const*)wexp_ptrs, (const uint8_t* const*)wu4_ptrs,
                     (const uint8_t* const*)wuexp_ptrs, c, (float*)workspace, experts, rows_bound, n, k, ldx8, ldw,
                     lds, ldc};
    hipStream_t s = (hipStream_t)stream;
    const bool bf16 = dtype == PLI_BF16;
    if (a.wu) return bf16 ? launch_splitk<bf16_t, true>(a, p, s) : launch_splitk<f16_t, true>(a, p, s);
    return bf16 ? launch_splitk<bf16_t, false>(a, p, s) : launch_splitk<f16_t, false>(a, p, s);
}
