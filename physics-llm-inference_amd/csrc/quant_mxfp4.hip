// MXFP4 activations on gfx950 (MI355X): the row quantiser of the W4A4 GEMM.
//   x [m, k] bf16 / fp16 -> x4 [m, k / 2] e2m1 code pairs, x_exp [m, k / 32] E8M0
//   bytes, x_scale fp32 [m];  value = decode_e2m1(code) * 2^(x_exp - 127) * x_scale[row]
// Per row:   E_r = floor(log2(amax_row)) - 2 over the finite elements (0 for a row
//            without a finite non-zero one), x_scale = 2^E_r.
// Per block: e_b = floor(log2(amax_block)) - 2 - E_r clamped from below at the
//            contract's lower end (mxfp4x_plan.h), byte 127 + e_b (127 for an
//            all-zero block), code = e2m1 round-to-nearest-even of
//            clamp(x / 2^(E_r + e_b), -6, 6): fp4_e2m1_encode, the rounding of
//            the Python quantize_weight_mxfp4.
// +-inf gives +-6 and enters neither amax; a NaN element gets code 0, enters
// neither amax and sets its block's byte to 0xFF.  Every step is exact: the
// exponents are integer arithmetic on the fp32 bits, the scaling is a power of
// two (v_ldexp_f32; a result below 2^-126 encodes to 0 whether it is kept as a
// subnormal or not), the rounding is a compare chain on exact thresholds.
//
// Kernel quant_rows_mxfp4<T, VEC> (index arithmetic: mxfp4x_plan.h), one
// workgroup of 256 threads per row.
//   VEC = 1  a lane holds chunks of 8 elements (one 16-byte load), a block of 32
//            is four adjacent lanes: block amax and NaN flag by two cross-lane
//            exchanges, row amax by a wave reduction and one pass through LDS.
//            The first four chunks of a lane stay in registers between the two
//            amax levels and the encode (rows up to 8192 elements are read
//            once).  Eight codes are one dword store per lane; the scale bytes
//            of four blocks are gathered into one dword store by the lane that
//            owns the first of them (a ragged last group: byte stores by the
//            owners).
//   VEC = 0  any alignment and leading dimension: a thread takes whole blocks,
//            reads them once per pass and stores bytes.
#include "fp4_codec.h"
#include "mxfp4x_plan.h"
#include "pli_common.h"

namespace pli {
namespace {

struct QuantStat {
    float amax;  // over the finite elements
    int nan;
};

__device__ __forceinline__ void quant4_note(float x, QuantStat& s) {
    const float a = fabsf(x);
    s.amax = fmaxf(s.amax, a < __builtin_inff() ? a : 0.f);  // the comparison is false for NaN and inf
    s.nan |= x != x;
}
// the code of x at block scale 2^e
__device__ __forceinline__ uint32_t quant4_code(float x, int e) {
    return x != x ? 0u : (uint32_t)fp4_e2m1_encode(__builtin_ldexpf(x, -e));
}

template <typename T> __device__ __forceinline__ void quant4_unpack8(i32x4 v, float (&x)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[2 * i] = elem<T>::to_f32(T{(uint16_t)((uint32_t)v[i] & 0xffffu)});
        x[2 * i + 1] = elem<T>::to_f32(T{(uint16_t)((uint32_t)v[i] >> 16)});
    }
}
// a chunk's statistics, merged over the four lanes of its block
template <typename T> __device__ __forceinline__ QuantStat quant4_block_stat(i32x4 v) {
    float x[8];
    quant4_unpack8<T>(v, x);
    QuantStat s{0.f, 0};
#pragma unroll
    for (int i = 0; i < 8; ++i) quant4_note(x[i], s);
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
        s.amax = fmaxf(s.amax, __shfl_xor(s.amax, o, 64));
        s.nan |= __shfl_xor(s.nan, o, 64);
    }
    return s;
}

// Encode chunk c (held in v, statistics s of its block) and store its codes and,
// from the owning lanes, the scale bytes.  Called by all 256 threads (the
// exchanges are unconditional); live: c < items.
template <typename T>
__device__ __forceinline__ void quant4_emit(i32x4 v, QuantStat s, int row_exp, int c, int items, int tid,
                                            uint8_t* __restrict__ x4, uint8_t* __restrict__ xe) {
    const int eb = mxfp4x_block_exp(__float_as_uint(s.amax), row_exp);
    const uint32_t byte = mxfp4x_block_byte(eb, s.nan != 0);
    float x[8];
    quant4_unpack8<T>(v, x);
    uint32_t codes = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) codes |= quant4_code(x[i], row_exp + eb) << (4 * i);
    // the bytes of the four blocks of this group of 16 lanes, in block order
    const int base = tid & ~15;
    const uint32_t four = (uint32_t)__shfl((int)byte, base, 64) | (uint32_t)__shfl((int)byte, base + 4, 64) << 8 |
                          (uint32_t)__shfl((int)byte, base + 8, 64) << 16 |
                          (uint32_t)__shfl((int)byte, base + 12, 64) << 24;
    if (c >= items) return;
    *reinterpret_cast<uint32_t*>(x4 + (int64_t)c * 4) = codes;
    const int c0 = c & ~15;
    if (c0 + 16 <= items) {
        if ((tid & 15) == 0) *reinterpret_cast<uint32_t*>(xe + (c0 >> 2)) = four;
    } else if ((tid & 3) == 0) {
        xe[c >> 2] = (uint8_t)byte;
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kMxfp4xQuantThreads) void quant_rows_mxfp4(const uint16_t* __restrict__ X, int64_t ldx,
                                                                       uint8_t* __restrict__ X4, int64_t ldx4,
                                                                       uint8_t* __restrict__ XE, int64_t ldxs,
                                                                       float* __restrict__ x_scale, int K) {
    __shared__ float part[kMxfp4xQuantThreads / 64];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const uint16_t* x = X + row * ldx;
    uint8_t* x4 = X4 + row * ldx4;
    uint8_t* xe = XE + row * ldxs;
    const int items = VEC ? K / 8 : K / kMxfp4aBlock;  // chunks (k % 32 == 0: whole blocks of four) or blocks
    const int trips = mxfp4x_quant_trips(items);
    float amax = 0.f;
    i32x4 held[kMxfp4xQuantHeld];
    QuantStat stat[kMxfp4xQuantHeld];
    if constexpr (VEC) {
#pragma unroll
        for (int u = 0; u < kMxfp4xQuantHeld; ++u) {
            const int c = mxfp4x_quant_item(tid, u);
            held[u] = i32x4{0, 0, 0, 0};
            if (c < items) held[u] = *reinterpret_cast<const i32x4*>(x + (int64_t)c * 8);
            stat[u] = quant4_block_stat<T>(held[u]);
            amax = fmaxf(amax, stat[u].amax);
        }
        for (int u = kMxfp4xQuantHeld; u < trips; ++u) {
            const int c = mxfp4x_quant_item(tid, u);
            if (c < items) {
                float v[8];
                quant4_unpack8<T>(*reinterpret_cast<const i32x4*>(x + (int64_t)c * 8), v);
                QuantStat s{amax, 0};
#pragma unroll
                for (int i = 0; i < 8; ++i) quant4_note(v[i], s);
                amax = s.amax;
            }
        }
    } else {
        for (int u = 0; u < trips; ++u) {
            const int b = mxfp4x_quant_item(tid, u);
            if (b < items) {
                QuantStat s{amax, 0};
                for (int i = 0; i < kMxfp4aBlock; ++i) quant4_note(elem<T>::to_f32(T{x[b * kMxfp4aBlock + i]}), s);
                amax = s.amax;
            }
        }
    }
    amax = wave_max(amax);
    if ((tid & 63) == 0) part[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
    const int row_exp = mxfp4x_row_exp(__float_as_uint(amax));
    if (tid == 0) x_scale[row] = __uint_as_float(mxfp4x_pow2_bits(row_exp));
    if constexpr (VEC) {
#pragma unroll
        for (int u = 0; u < kMxfp4xQuantHeld; ++u)
            if (kMxfp4xQuantThreads * u < items)  // uniform: the exchanges inside need every lane
                quant4_emit<T>(held[u], stat[u], row_exp, mxfp4x_quant_item(tid, u), items, tid, x4, xe);
        for (int u = kMxfp4xQuantHeld; u < trips; ++u) {
            const int c = mxfp4x_quant_item(tid, u);
            i32x4 v = i32x4{0, 0, 0, 0};
            if (c < items) v = *reinterpret_cast<const i32x4*>(x + (int64_t)c * 8);
            quant4_emit<T>(v, quant4_block_stat<T>(v), row_exp, c, items, tid, x4, xe);
        }
    } else {
        for (int u = 0; u < trips; ++u) {
            const int b = mxfp4x_quant_item(tid, u);
            if (b >= items) continue;
            const uint16_t* xb = x + b * kMxfp4aBlock;
            QuantStat s{0.f, 0};
            for (int i = 0; i < kMxfp4aBlock; ++i) quant4_note(elem<T>::to_f32(T{xb[i]}), s);
            const int eb = mxfp4x_block_exp(__float_as_uint(s.amax), row_exp);
            xe[b] = mxfp4x_block_byte(eb, s.nan != 0);
            for (int i = 0; i < kMxfp4aBlock; i += 2)
                x4[(b * kMxfp4aBlock + i) >> 1] =
                    (uint8_t)(quant4_code(elem<T>::to_f32(T{xb[i]}), row_exp + eb) |
                              quant4_code(elem<T>::to_f32(T{xb[i + 1]}), row_exp + eb) << 4);
        }
    }
}

template <typename T>
int launch_quant(const void* x, int64_t ldx, void* x4, int64_t ldx4, void* x_exp, int64_t ldxs, float* x_scale, int m,
                 int k, hipStream_t s) {
#define PLI_QUANT_MXFP4(VEC)                                                                                       \
    hipLaunchKernelGGL((quant_rows_mxfp4<T, VEC>), dim3(m), dim3(kMxfp4xQuantThreads), 0, s, (const uint16_t*)x, \
                       ldx, (uint8_t*)x4, ldx4, (uint8_t*)x_exp, ldxs, x_scale, k)
    if (mxfp4x_quant_vec(ldx, ldx4, ldxs, (uintptr_t)x, (uintptr_t)x4, (uintptr_t)x_exp)) PLI_QUANT_MXFP4(true);
    else PLI_QUANT_MXFP4(false);
#undef PLI_QUANT_MXFP4
    return launch_status("quant_rows_mxfp4");
}

}  // namespace
}  // namespace pli

extern "C" int pli_quantize_rows_mxfp4(const void* x, int64_t ldx, void* x4, int64_t ldx4, void* x_exp, int64_t ldxs,
                                       float* x_scale, int m, int k, int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(dtype == PLI_F16 || dtype == PLI_BF16,
                "pli_quantize_rows_mxfp4: bad dtype %d (fp16 / bf16 rows only)", dtype);
    PLI_REQUIRE(m >= 0 && k >= 0, "pli_quantize_rows_mxfp4: bad shape m=%d k=%d", m, k);
    PLI_REQUIRE(mxfp4a_shape_ok(k), "pli_quantize_rows_mxfp4: k=%d is not a multiple of the MX block of 32", k);
    PLI_REQUIRE(ldx >= k && ldx4 >= k / 2 && ldxs >= k / kMxfp4aBlock,
                "pli_quantize_rows_mxfp4: leading dimension too small (ldx=%lld ldx4=%lld ldxs=%lld)", (long long)ldx,
                (long long)ldx4, (long long)ldxs);
    if (m == 0) return PLI_OK;  // empty operands may be NULL
    PLI_REQUIRE(x_scale && (k == 0 || (x && x4 && x_exp)), "pli_quantize_rows_mxfp4: null pointer");
    // k == 0: the kernel reads and writes no element and stores scale 1.0
    hipStream_t s = (hipStream_t)stream;
    return dtype == PLI_BF16 ? launch_quant<bf16_t>(x, ldx, x4, ldx4, x_exp, ldxs, x_scale, m, k, s)
                             : launch_quant<f16_t>(x, ldx, x4, ldx4, x_exp, ldxs, x_scale, m, k, s);
}
