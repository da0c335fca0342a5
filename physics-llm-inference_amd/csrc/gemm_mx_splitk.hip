// Split-K block-scaled GEMM for 17 .. 256 rows on gfx950 (MI355X): fp8 e4m3
// activation rows against fp8 e4m3 weights (pli_gemm_fp8_ws) or MXFP4 weights
// (pli_gemm_mxfp4_ws), with a caller workspace.  A call of so few rows is one
// or two rows of 128 x 128 tiles, far fewer workgroups than the device has
// CUs, each walking the whole K alone; here K is cut into S chunks, every
// (n tile, chunk, m tile) is a workgroup that writes an fp32 partial, and a
// second kernel sums the partials in a fixed order and finishes them exactly as
// the plain kernels finish their sums.
//
// Kernels (index arithmetic, route and split rule: mx_splitk_plan.h, checked on
// the CPU by tests/host/mx_splitk_plan_check.cpp):
//   gemm_mx_splitk<WFMT, MC>     C^T partial of 128 W rows x 32 MC X rows over one
//                                K chunk on v_mfma_scale_f32_32x32x64_f8f6f4.  The
//                                four waves split n, so a wave's W rows are its
//                                own: W (and the E8M0 scale dword) goes from
//                                global memory straight into double-buffered
//                                operand registers, each byte read once per call
//                                by one lane.  X is shared by the waves: three LDS
//                                stages of gemm_fp8_mx's swizzled image fed by
//                                16-byte LDS-DMA.
//   gemm_mx_splitk_reduce<T, B>  one thread per 4 n of one m: partials summed in
//                                chunk order, fp8a_finish, + bias, one rounding
#include "fp8_kv.h"
#include "mx_finish.h"
#include "mx_splitk_plan.h"
#include "pli_common.h"

namespace pli {
namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// the W operand registers of one K-step: e4m3 [k-half][16-byte half], e2m1 [k-half] and the scale dword
template <int WFMT> struct MxskW {
    i32x4 q[WFMT == MXSK_E2M1 ? 2 : 4];
    uint32_t sc;
};

// everything but the last N vector-memory operations of this wave has landed; the registers in flight pass
// through the statement, so nothing derived from them is scheduled in front of it
#define PLI_MXSK_WAIT(N_STR)                                                                                     \
    if constexpr (WFMT == MXSK_E2M1)                                                                             \
        asm volatile("s_waitcnt vmcnt(" N_STR ")" : "+v"(w.q[0]), "+v"(w.q[1]), "+v"(w.sc)::"memory");           \
    else                                                                                                         \
        asm volatile("s_waitcnt vmcnt(" N_STR ")" : "+v"(w.q[0]), "+v"(w.q[1]), "+v"(w.q[2]), "+v"(w.q[3])::"memory")

template <int WFMT, int N> __device__ __forceinline__ void mxsk_wait_n(MxskW<WFMT>& w) {
    static_assert(N >= 0 && N <= 4, "one counted wait per MC");
    if constexpr (N == 0) { PLI_MXSK_WAIT("0"); }
    else if constexpr (N == 1) { PLI_MXSK_WAIT("1"); }
    else if constexpr (N == 2) { PLI_MXSK_WAIT("2"); }
    else if constexpr (N == 3) { PLI_MXSK_WAIT("3"); }
    else { PLI_MXSK_WAIT("4"); }
}
#undef PLI_MXSK_WAIT

// ---------------------------------------------------------------------------
// gemm_mx_splitk.  Per K-step of 128 codes a wave issues its W loads for step
// s + 1 (e4m3: four 16-byte loads, e2m1: two and the scale dword) and its MC
// LDS-DMA pieces of X for step s + 2, then multiplies step s: per k-half one W
// operand against MC X fragments (two ds_read_b128 each), 2 MC scaled MFMAs per
// step into MC accumulators.  Vector-memory operations are issued in the order
//   X(0) W(0) X(1) | W(1) X(2) | W(2) X(3) | ...
// so in front of step s exactly the MC pieces of X(s + 1) may still be in
// flight: one s_waitcnt vmcnt(MC) (vmcnt(0) on the chunk's last step) and one
// barrier per step.  The barrier also says every wave is done reading the
// stage of step s - 1, which is the one X(s + 2) overwrites.
template <int WFMT, int MC>
__device__ __forceinline__ void mxsk_partial(const uint8_t* __restrict__ X8, const uint8_t* __restrict__ W,
                                             const uint8_t* __restrict__ w_exp, float* __restrict__ ws, int M, int N,
                                             int ks, int per, int64_t ldx8, int64_t ldw, int64_t lds) {
    constexpr int kStageBytes = MC * kMxskBlockBytes;
    constexpr int kNQ = WFMT == MXSK_E2M1 ? 2 : 4;
    __shared__ __attribute__((aligned(1024))) char smem[kMxskStages * kStageBytes];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n0 = blockIdx.x * kFp8aTN, c = blockIdx.y, m0 = blockIdx.z * kFp8aTM;
    const int s0 = mxsk_chunk_begin(c, per), len = mxsk_chunk_end(c, per, ks) - s0;

    // per-lane sources at the chunk's first K-step (local step s: + one K-step's bytes each)
    const uint8_t* xsrc[MC];
#pragma unroll
    for (int i = 0; i < MC; ++i) {
        const int p = mxsk_x_piece(wave, i);
        xsrc[i] = X8 + fp8a_src_off(m0, fp8a_stage_row(p, lane), M, ldx8, s0, fp8a_stage_chunk(p, lane));
    }
    const int wrow = mxsk_w_row(wave, lane);
    const uint8_t* wsrc[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q)  // e4m3: q = 2 kh + h; e2m1: q = kh
        wsrc[q] = W + (WFMT == MXSK_E2M1 ? mxsk_w_off(WFMT, n0, wrow, N, ldw, s0, q, lane, 0)
                                         : mxsk_w_off(WFMT, n0, wrow, N, ldw, s0, q >> 1, lane, q & 1));
    const uint8_t* ssrc = WFMT == MXSK_E2M1 ? w_exp + mxfp4a_scale_off(n0, wrow, N, lds, s0) : nullptr;
    constexpr int kWStep = WFMT == MXSK_E2M1 ? kMxfp4aWRowBytes : kFp8aKStep;

    // the wave's MC LDS-DMA pieces of X for local step S into stage BUF (the LDS address is the wave's piece base:
    // the hardware adds 16 x lane)
#define PLI_MXSK_STAGE_X(S, BUF)                                                                                    \
    _Pragma("unroll") for (int i = 0; i < MC; ++i) __builtin_amdgcn_global_load_lds(                                \
        xsrc[i] + (int64_t)(S) * kFp8aKStep,                                                                        \
        (lds_void*)(smem + (BUF) * kStageBytes + fp8a_stage_lds(mxsk_x_piece(wave, i), 0)), 16, 0, 0)
    auto load_w = [&](MxskW<WFMT>& w, int s) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < kNQ; ++q) w.q[q] = *reinterpret_cast<const i32x4*>(wsrc[q] + (int64_t)s * kWStep);
        if constexpr (WFMT == MXSK_E2M1)
            w.sc = *reinterpret_cast<const uint32_t*>(ssrc + (int64_t)s * (kMxfp4aKStep / kMxfp4aBlock));
        else
            w.sc = 0;
    };

    // X fragment read offsets inside a stage: [m block][k-half][16-byte half]
    int xrd[MC][2][2];
#pragma unroll
    for (int b = 0; b < MC; ++b)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int h = 0; h < 2; ++h)
                xrd[b][kh][h] = fp8a_frag_lds(mxsk_x_row(b, lane), mxsk_x_chunk(WFMT, kh, lane, h));
    const int shift0 = mxfp4a_scale_shift(0, lane), shift1 = mxfp4a_scale_shift(1, lane);

    f32x16 acc[MC];
#pragma unroll
    for (int b = 0; b < MC; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

    MxskW<WFMT> next, cur;
    int buf = 0;  // the stage of step s
    // One K-step is begin(more_w); [the X pieces of step s + 2]; multiply().  more_w: step s + 1 exists, so X(s + 1) is
    // in flight in front of the wait and W(s + 1) is loaded.  The flag is a literal at every call and the lambdas
    // are inlined, so every path through the steps has one fixed issue order.
    auto begin = [&](int s, bool more_w) __attribute__((always_inline)) {
        if (more_w) mxsk_wait_n<WFMT, MC>(next);
        else mxsk_wait_n<WFMT, 0>(next);
        __builtin_amdgcn_s_barrier();
        cur = next;
        if (more_w) load_w(next, s + 1);
        __builtin_amdgcn_sched_barrier(0);  // the W loads stay in front of the X pieces: the count relies on it
    };
    auto multiply = [&]() __attribute__((always_inline)) {
        const char* img = smem + buf * kStageBytes;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            i32x8 wf;
            int sc = 127;  // E8M0 2^0
            if constexpr (WFMT == MXSK_E2M1) {
                wf = i32x8{cur.q[kh].x, cur.q[kh].y, cur.q[kh].z, cur.q[kh].w, 0, 0, 0, 0};  // cbsz = 4: four registers
                sc = (int)(cur.sc >> (kh ? shift1 : shift0));  // byte 0 is the block's scale
            } else {
                const i32x4 lo = cur.q[2 * kh], hi = cur.q[2 * kh + 1];
                wf = i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            }
#pragma unroll
            for (int b = 0; b < MC; ++b) {
                const i32x4 xl = lds_read_b128(img, xrd[b][kh][0]), xh = lds_read_b128(img, xrd[b][kh][1]);
                const i32x8 xf = i32x8{xl.x, xl.y, xl.z, xl.w, xh.x, xh.y, xh.z, xh.w};
                // A = W (cbsz 4: e2m1, 0: e4m3), its scale byte 0 of the lane's register; B = X e4m3 at 2^0
                acc[b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf, xf, acc[b], WFMT == MXSK_E2M1 ? 4 : 0, 0,
                                                                         0, sc, 0, 127);
            }
        }
        buf = buf + 1 < kMxskStages ? buf + 1 : 0;
    };
    PLI_MXSK_STAGE_X(0, 0);
    load_w(next, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (len == 1) {
        begin(0, false);
        multiply();
    } else {
        PLI_MXSK_STAGE_X(1, 1);
        int s = 0;
        for (; s + 2 < len; ++s) {
            begin(s, true);
            PLI_MXSK_STAGE_X(s + 2, buf >= 1 ? buf - 1 : kMxskStages - 1);  // stage (buf + 2) % 3: step s - 1's, read by all
            multiply();
        }
        begin(s, true);
        multiply();
        begin(s + 1, false);
        multiply();
    }

#undef PLI_MXSK_STAGE_X
    // the partial as it is: a lane holds, per m block and register group g, 4 consecutive n of one m
#pragma unroll
    for (int b = 0; b < MC; ++b) {
        const int mrow = m0 + mxsk_acc_m(b, lane);
        if (mrow >= M) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ncol = n0 + mxsk_acc_n(wave, lane, 4 * g);
            if (ncol >= N) continue;  // N % 4 == 0: the group is inside or outside as a whole
            *reinterpret_cast<f32x4*>(ws + mxsk_ws_index(c, mrow, ncol, M, N)) =
                f32x4{acc[b][4 * g], acc[b][4 * g + 1], acc[b][4 * g + 2], acc[b][4 * g + 3]};
        }
    }
}

// The kernel instances gemm_mx_splitk<WFMT, MC>, one plain __global__ function each over the body above.
#define PLI_MXSK_KERNEL(NAME, WFMT, MC)                                                                            \
    __global__ __launch_bounds__(256) void NAME(const uint8_t* __restrict__ X8, const uint8_t* __restrict__ W,      \
                                                const uint8_t* __restrict__ w_exp, float* __restrict__ ws, int M,   \
                                                int N, int ks, int per, int64_t ldx8, int64_t ldw, int64_t lds) {   \
        mxsk_partial<WFMT, MC>(X8, W, w_exp, ws, M, N, ks, per, ldx8, ldw, lds);                                    \
    }
PLI_MXSK_KERNEL(gemm_mx_splitk_e4m3_mc1, MXSK_E4M3, 1)
PLI_MXSK_KERNEL(gemm_mx_splitk_e4m3_mc2, MXSK_E4M3, 2)
PLI_MXSK_KERNEL(gemm_mx_splitk_e4m3_mc3, MXSK_E4M3, 3)
PLI_MXSK_KERNEL(gemm_mx_splitk_e4m3_mc4, MXSK_E4M3, 4)
PLI_MXSK_KERNEL(gemm_mx_splitk_e2m1_mc1, MXSK_E2M1, 1)
PLI_MXSK_KERNEL(gemm_mx_splitk_e2m1_mc2, MXSK_E2M1, 2)
PLI_MXSK_KERNEL(gemm_mx_splitk_e2m1_mc3, MXSK_E2M1, 3)
PLI_MXSK_KERNEL(gemm_mx_splitk_e2m1_mc4, MXSK_E2M1, 4)
#undef PLI_MXSK_KERNEL

// ---------------------------------------------------------------------------
// gemm_mx_splitk_reduce: partials summed in the order c = 0 .. S - 1, then the
// plain kernels' finishing expression (w_scale NULL, as for MXFP4 weights: ones),
// the bias, one rounding and one 8-byte store.
template <typename T, bool BIAS>
__global__ __launch_bounds__(kMxskReduceThreads) void gemm_mx_splitk_reduce(
    const float* __restrict__ ws, const float* __restrict__ x_scale, const float* __restrict__ w_scale,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ C, int M, int N, int S, int64_t ldc) {
    const int64_t i = (int64_t)blockIdx.x * kMxskReduceThreads + threadIdx.x;
    if (i >= mxsk_reduce_items(M, N)) return;
    const int nq = N / kFp8aStoreN;
    const int r = (int)(i / nq), j = (int)(i % nq) * kFp8aStoreN;
    f32x4 sum = *reinterpret_cast<const f32x4*>(ws + mxsk_ws_index(0, r, j, M, N));
    for (int c = 1; c < S; ++c) sum += *reinterpret_cast<const f32x4*>(ws + mxsk_ws_index(c, r, j, M, N));
    const float xs = fp8_scale_of(x_scale, r);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = fp8a_finish(sum[e], xs, fp8_scale_of(w_scale, j + e));
        if constexpr (BIAS) v[e] += elem<T>::to_f32(T{bias[j + e]});
    }
    *reinterpret_cast<i32x2*>(C + (int64_t)r * ldc + j) = i32x2{(int)pack2<T>(v[0], v[1]), (int)pack2<T>(v[2], v[3])};
}

// ------------------------------------------------------------------ launch --
struct MxskArgs {
    const void *x8, *w, *w_exp, *bias;
    const float *x_scale, *w_scale;
    void* c;
    float* ws;
    int m, n, k;
    int64_t ldx8, ldw, lds, ldc;
};

template <int WFMT, typename T>
int launch_splitk(const MxskArgs& a, const MxskPlan& p, hipStream_t s) {
    using Kernel = void (*)(const uint8_t*, const uint8_t*, const uint8_t*, float*, int, int, int, int, int64_t,
                            int64_t, int64_t);
    static const Kernel kernels[2][kMxskMaxMC] = {
        {gemm_mx_splitk_e4m3_mc1, gemm_mx_splitk_e4m3_mc2, gemm_mx_splitk_e4m3_mc3, gemm_mx_splitk_e4m3_mc4},
        {gemm_mx_splitk_e2m1_mc1, gemm_mx_splitk_e2m1_mc2, gemm_mx_splitk_e2m1_mc3, gemm_mx_splitk_e2m1_mc4}};
    hipLaunchKernelGGL(kernels[WFMT][p.mc - 1], dim3(p.tiles_n, p.splits, p.tiles_m), dim3(256), 0, s,
                       (const uint8_t*)a.x8, (const uint8_t*)a.w, (const uint8_t*)a.w_exp, a.ws, a.m, a.n,
                       a.k / kFp8aKStep, p.per, a.ldx8, a.ldw, a.lds);
    if (const int rc = launch_status("gemm_mx_splitk")) return rc;
    const unsigned blocks = (unsigned)mxsk_reduce_blocks(a.m, a.n);
#define PLI_MXSK_REDUCE(BIAS)                                                                                     \
    hipLaunchKernelGGL((gemm_mx_splitk_reduce<T, BIAS>), dim3(blocks), dim3(kMxskReduceThreads), 0, s, a.ws,      \
                       a.x_scale, a.w_scale, (const uint16_t*)a.bias, (uint16_t*)a.c, a.m, a.n, p.splits, a.ldc)
    if (a.bias) PLI_MXSK_REDUCE(true);
    else PLI_MXSK_REDUCE(false);
#undef PLI_MXSK_REDUCE
    return launch_status("gemm_mx_splitk_reduce");
}

}  // namespace
}  // namespace pli

extern "C" size_t pli_gemm_fp8_workspace_size(int m, int n, int k, int splits) {
    return pli::mxsk_workspace_size(m, n, k, splits);
}

extern "C" size_t pli_gemm_mxfp4_workspace_size(int m, int n, int k, int splits) {
    return pli::mxsk_workspace_size(m, n, k, splits);
}

extern "C" int pli_gemm_fp8_ws(const void* x8, const float* x_scale, const void* w8, const float* w_scale,
                               const void* bias, void* c, int m, int n, int k, int64_t ldx8, int64_t ldw, int64_t ldc,
                               int dtype, void* workspace, size_t workspace_bytes, int splits, void* stream) {
    using namespace pli;
    clear_error();
    // pli_gemm_fp8's rules in its order, then splits
    PLI_REQUIRE(dtype == PLI_F16 || dtype == PLI_BF16, "pli_gemm_fp8_ws: bad dtype %d (fp16 / bf16 output only)", dtype);
    PLI_REQUIRE(m >= 0 && n >= 0 && k >= 0, "pli_gemm_fp8_ws: bad shape m=%d n=%d k=%d", m, n, k);
    PLI_REQUIRE(ldx8 >= k && ldw >= k && ldc >= n,
                "pli_gemm_fp8_ws: leading dimension too small (ldx8=%lld ldw=%lld ldc=%lld)", (long long)ldx8,
                (long long)ldw, (long long)ldc);
    if (m != 0 && n != 0) {  // empty operands may be NULL
        PLI_REQUIRE(c && (k == 0 || (x8 && w8)), "pli_gemm_fp8_ws: null pointer");
        PLI_REQUIRE(((int64_t)m * n + 255) / 256 <= 0x7fffffffLL, "pli_gemm_fp8_ws: grid too large");
    }
    PLI_REQUIRE(splits >= 0, "pli_gemm_fp8_ws: bad splits %d (0: the rule chooses, >= 1: forced)", splits);
    if (m == 0 || n == 0) return PLI_OK;
    const Fp8aCall call{m, n, k, ldx8, ldw, ldc, (uintptr_t)x8, (uintptr_t)w8, (uintptr_t)c};
    const MxskPlan p = mxsk_plan(fp8a_route(call) == FP8A_MX, m, n, k, splits, (uintptr_t)workspace, workspace_bytes);
    if (p.splits < 2) return pli_gemm_fp8(x8, x_scale, w8, w_scale, bias, c, m, n, k, ldx8, ldw, ldc, dtype, stream);
    const MxskArgs a{x8, w8, nullptr, bias, x_scale, w_scale, c, (float*)workspace, m, n, k, ldx8, ldw, 0, ldc};
    hipStream_t s = (hipStream_t)stream;
    return dtype == PLI_BF16 ? launch_splitk<MXSK_E4M3, bf16_t>(a, p, s) : launch_splitk<MXSK_E4M3, f16_t>(a, p, s);
}

extern "C" int pli_gemm_mxfp4_ws(const void* x8, const float* x_scale, const void* w4, const void* w_exp,
                                 const void* bias, void* c, int m, int n, int k, int64_t ldx8, int64_t ldw,
                                 int64_t lds, int64_t ldc, int dtype, void* workspace, size_t workspace_bytes,
                                 int splits, void* stream) {
    using namespace pli;
    clear_error();
    // pli_gemm_mxfp4's rules in its order, then splits
    PLI_REQUIRE(dtype == PLI_F16 || dtype == PLI_BF16, "pli_gemm_mxfp4_ws: bad dtype %d (fp16 / bf16 output only)",
                dtype);
    PLI_REQUIRE(m >= 0 && n >= 0 && k >= 0, "pli_gemm_mxfp4_ws: bad shape m=%d n=%d k=%d", m, n, k);
    PLI_REQUIRE(mxfp4a_shape_ok(k), "pli_gemm_mxfp4_ws: k=%d is not a multiple of the MX block of 32", k);
    PLI_REQUIRE(ldx8 >= k && ldw >= k / 2 && lds >= k / kMxfp4aBlock && ldc >= n,
                "pli_gemm_mxfp4_ws: leading dimension too small (ldx8=%lld ldw=%lld lds=%lld ldc=%lld)",
                (long long)ldx8, (long long)ldw, (long long)lds, (long long)ldc);
    if (m != 0 && n != 0) {  // empty operands may be NULL
        PLI_REQUIRE(c && (k == 0 || (x8 && w4 && w_exp)),
                    "pli_gemm_mxfp4_ws: null pointer (the scale bytes have no default)");
        PLI_REQUIRE(((int64_t)m * n + 255) / 256 <= 0x7fffffffLL, "pli_gemm_mxfp4_ws: grid too large");
    }
    PLI_REQUIRE(splits >= 0, "pli_gemm_mxfp4_ws: bad splits %d (0: the rule chooses, >= 1: forced)", splits);
    if (m == 0 || n == 0) return PLI_OK;
    const Mxfp4aCall call{m, n, k, ldx8, ldw, lds, ldc, (uintptr_t)x8, (uintptr_t)w4, (uintptr_t)w_exp, (uintptr_t)c};
    const MxskPlan p =
        mxsk_plan(mxfp4a_route(call) == MXFP4A_MX, m, n, k, splits, (uintptr_t)workspace, workspace_bytes);
    if (p.splits < 2)
        return pli_gemm_mxfp4(x8, x_scale, w4, w_exp, bias, c, m, n, k, ldx8, ldw, lds, ldc, dtype, stream);
    const MxskArgs a{x8, w4, w_exp, bias, x_scale, nullptr, c, (float*)workspace, m, n, k, ldx8, ldw, lds, ldc};
    hipStream_t s = (hipStream_t)stream;
    return dtype == PLI_BF16 ? launch_splitk<MXSK_E2M1, bf16_t>(a, p, s) : launch_splitk<MXSK_E2M1, f16_t>(a, p, s);
}
