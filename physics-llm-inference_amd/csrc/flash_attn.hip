// Fused attention forward for gfx950 (MI355X).
//
// Replaces the Python tile loop of ch06/flash_attention.py:14-74 (about 12
// torch launches per (q-block, k-block) pair, every intermediate through HBM)
// with ONE launch: Q stays in registers, K/V tiles stream through LDS, the
// online softmax runs in registers with fp32 statistics.
//
// MFMA kernels (bf16 / fp16, head_dim 64 or 128), one wave = 32 query rows:
//   S^T = K Q^T      v_mfma_f32_32x32x16  A = K tile (ds_read_b128, LDS),
//                                         B = Q fragment (registers)
//   -> lane l owns query row l&31; its 64 tile scores sit in 32 registers
//      split over the two half-waves, so the row max is lane-local plus one
//      cross-half exchange (no LDS, no per-tile cross-lane sum).
//   O^T += V^T P^T   v_mfma_f32_32x32x16  A = V^T (ds_read_b64_tr_b16 from the
//                                         row-major V tile), B = P straight
//                                         from the S^T accumulator registers
//   -> O^T keeps the query row on the lane too, so the online-softmax rescale
//      and the final 1/l are lane-local.
// attn_fwd_v7 (flash_v7.hip, the default) and attn_fwd_v2 (below, the
// previous default, kept as the A/B baseline) share that mapping; v7 moves
// the score scaling into the MFMA and the row sum onto the matrix core.
// Blocks are remapped so each XCD works through a contiguous range of heads:
// a head's K/V is then read from HBM once and re-read from that XCD's L2 by
// all of the head's query blocks.
//
// Generic kernel (fp32, or any head_dim <= 128, or unaligned operands):
// LDS-tiled VALU kernel with the same online recurrence, fp32 accumulate.
#include <cmath>

#include "flash_v7.h"
#include "pli_common.h"

namespace pli {
namespace {

constexpr int KT = 64;  // keys per LDS tile
constexpr int QW = 32;  // query rows per wave

// --------------------------------------------------------------------------
// attn_fwd_v2: attn_fwd_mfma's fragment mapping and register staging, with
// the per-tile overheads removed:
//  * padded LDS rows instead of an XOR swizzle -- K rows 2D+16 B, V rows
//    2D+64 B.  K's b128 reads of 16 consecutive rows land on 16 distinct
//    16-byte slots (stride = 17 slots mod 16); V's tr_b16 reads of 4 rows x
//    64 B land on 4 disjoint 16-bank quarters (stride = 80 dwords = 16 mod 64).
//    Every fragment address is then one per-lane base register + an
//    immediate offset: no per-read address arithmetic in the loop.
//  * global staging addresses are one per-lane base + scalar tile offset;
//    the clamp for rows past Nk only runs on a ragged last tile.
//  * the O rescale is skipped (exactly) when no row's max moved this tile.
// (A software-pipelined variant that issued QK^T(t+1) beside softmax(t) with
// LDS-DMA staging spilled at D=128 and ran 1.5-2.5x slower: every spill
// reload's vmcnt(0) also drained the in-flight DMA.  See DESIGN.md.)
template <int D, int KTL = KT> struct PadLayout {
    static constexpr int KS = 2 * D + 16;  // K row stride (bytes)
    static constexpr int VS = 2 * D + 64;  // V row stride (bytes)
    static constexpr int KSZ = KTL * KS, VSZ = KTL * VS, BUF = KSZ + VSZ;
};

// OPT bits (A/B levers on the v2 body, variants 16-20):
//  1: the xor-32 row-max exchange as v_permlane32_swap instead of ds_bpermute
//  2: static s_setprio 1 for the younger half of the workgroup (waves NW/2..)
//  4: defer-max: keep the running max unless a tile raises it by > 8 (log2
//     units), so P <= 2^8 and the O rescale almost never runs after tile 0
//  8: row sum over the bf16/f16-ROUNDED P (v_dot2c with {1,1}), so l
//     normalises exactly the weights P.V used.  Needed with 4: a dominant
//     weight is no longer exactly 1 and its rounding would otherwise go
//     uncorrected (measured 1.05e-2 on the spike test without it).
// 16: epilogue: pair the two half-waves' 8-byte pieces of a row with
//     v_permlane32_swap so each lane stores 16 B (8 dwordx4 instead of 16 dwordx2)
// 32 / 64: __builtin_amdgcn_iglp_opt(0) / (1) in the tile loop (the compiler's
//     MFMA + DS interleave strategies)
// 128: batched fragment reads (all K fragments of the tile, V^T one block
//     ahead) so LDS latency overlaps the MFMAs instead of pairing each read
//     with the MFMA that consumes it
constexpr int kOptPermlane = 1, kOptPrio = 2, kOptDefer = 4, kOptRoundedSum = 8, kOptWideStore = 16,
              kOptIglp0 = 32, kOptIglp1 = 64, kOptBatchReads = 128;
constexpr float kDeferThr = 8.f;

__device__ __forceinline__ float xor32_max(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xor32_sum(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

template <typename T, int D, int NW, bool LAZY, int OPT = 0, int KTL = KT>
__global__ __launch_bounds__(NW * 64, 2) void attn_fwd_v2(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, uint16_t* __restrict__ o, int H, int group,
    int Nq, int Nk, V7Strides st, float c, int causal, int qblocks,
    int nblocks) {
    using L = PadLayout<D, KTL>;
    constexpr int NS = KTL / 32;        // 32-key sub-tiles per tile
    constexpr int NT = NW * 64;
    constexpr int CPR = D / 8;          // 16-byte chunks per row
    constexpr int RPI = NT / CPR;       // rows covered by one staging step
    constexpr int CPT = KTL / RPI;      // staging steps per tile
    static_assert(NT % CPR == 0 && KTL % RPI == 0, "staging must tile evenly");
    __shared__ __attribute__((aligned(16))) char smem[2 * L::BUF];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h32 = lane >> 5, l32 = lane & 31;
    const int lb = xcd_remap(blockIdx.x, nblocks);
    const int bh = lb / qblocks;
    // causal: a query block's work grows with its index; start each head's
    // heaviest blocks first so the grid drains on light ones
    const int qblk = causal ? qblocks - 1 - lb % qblocks : lb % qblocks;
    const int b = bh / H, hq = bh % H, hk = hq / group;
    const int qbase = qblk * (NW * QW);
    const int q0 = qbase + wave * QW;
    const int off_diag = Nk - Nq;

    const uint16_t* qp = q + b * st.qb + hq * st.qh;
    const uint16_t* kp = k + b * st.kb + hk * st.kh;
    const uint16_t* vp = v + b * st.vb + hk * st.vh;

    i32x4 qf[D / 16];
    {
        const int qr = q0 + l32;
        const bool ok = qr < Nq;
        const uint16_t* src = qp + (int64_t)(ok ? qr : 0) * st.qn + 8 * h32;
#pragma unroll
        for (int kk = 0; kk < D / 16; ++kk) {
            const i32x4 x = *reinterpret_cast<const i32x4*>(src + 16 * kk);
            qf[kk] = ok ? x : i32x4{0, 0, 0, 0};
        }
    }

    int kv_end = Nk;
    if (causal) kv_end = min(Nk, qbase + NW * QW + off_diag);
    const int nt = kv_end > 0 ? cdiv(kv_end, KTL) : 0;
    const int t_full = Nk / KTL;  // tiles [0, t_full) need no row clamp
    int t_mask = t_full;         // first tile this wave must mask
    if (causal) t_mask = min(t_mask, max(0, (q0 + off_diag + 1) / KTL));

    // staging: thread owns chunk `sch` of rows srow + i*RPI
    const int srow = tid / CPR, sch = tid % CPR;
    const uint16_t* kg = kp + (int64_t)srow * st.kn + sch * 8;
    const uint16_t* vg = vp + (int64_t)srow * st.vn + sch * 8;
    const int kw = srow * L::KS + sch * 16, vw = L::KSZ + srow * L::VS + sch * 16;
    i32x4 kst[CPT], vst[CPT];
    auto load_tile = [&](int t) {
        if (t < t_full) {
#pragma unroll
            for (int i = 0; i < CPT; ++i) {
                const int64_t r = (int64_t)t * KTL + i * RPI;
                kst[i] = *reinterpret_cast<const i32x4*>(kg + r * st.kn);
                vst[i] = *reinterpret_cast<const i32x4*>(vg + r * st.vn);
            }
        } else {
#pragma unroll
            for (int i = 0; i < CPT; ++i) {
                const int key = t * KTL + i * RPI + srow;
                const int64_t r = min(key, Nk - 1) - srow;
                const i32x4 kx = *reinterpret_cast<const i32x4*>(kg + r * st.kn);
                const i32x4 vx = *reinterpret_cast<const i32x4*>(vg + r * st.vn);
                kst[i] = key < Nk ? kx : i32x4{0, 0, 0, 0};
                vst[i] = key < Nk ? vx : i32x4{0, 0, 0, 0};
            }
        }
    };
    auto store_tile = [&](int buf) {
        char* base = smem + buf * L::BUF;
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            lds_write_b128(base, kw + i * RPI * L::KS, kst[i]);
            lds_write_b128(base, vw + i * RPI * L::VS, vst[i]);
        }
    };

    // per-lane fragment bases (byte offsets inside one buffer)
    const int g = lane >> 4, i16 = lane & 15, qq = i16 >> 2, pp = i16 & 3;
    const int kr = l32 * L::KS + h32 * 16;
    const int vr = L::KSZ + (4 * h32 + qq) * L::VS + (2 * (g & 1) + (pp >> 1)) * 16 + 8 * (pp & 1);

    f32x16 oacc[D / 32];
#pragma unroll
    for (int d = 0; d < D / 32; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
    float m_run = -1e30f, l_run = 0.f;

    if (nt > 0) {
        load_tile(0);
        store_tile(0);
    }
    __syncthreads();
    if constexpr ((OPT & kOptPrio) != 0) {
        if (wave >= NW / 2) __builtin_amdgcn_s_setprio(1);
    }

    for (int t = 0; t < nt; ++t) {
        if constexpr ((OPT & kOptIglp0) != 0) __builtin_amdgcn_iglp_opt(0);
        if constexpr ((OPT & kOptIglp1) != 0) __builtin_amdgcn_iglp_opt(1);
        if (t + 1 < nt) load_tile(t + 1);
        const char* kb = smem + (t & 1) * L::BUF + kr;
        const char* vb = smem + (t & 1) * L::BUF + vr;

        f32x16 s[NS];
        if constexpr ((OPT & kOptBatchReads) != 0) {
            // every K fragment of the tile in flight before the first MFMA
            i32x4 kfr[NS][D / 16];
#pragma unroll
            for (int tt = 0; tt < NS; ++tt)
#pragma unroll
                for (int kk = 0; kk < D / 16; ++kk) kfr[tt][kk] = lds_read_b128(kb, tt * 32 * L::KS + kk * 32);
            __builtin_amdgcn_sched_barrier(0);  // keep the batch ahead of the MFMAs
#pragma unroll
            for (int tt = 0; tt < NS; ++tt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[tt][r] = 0.f;
#pragma unroll
                for (int kk = 0; kk < D / 16; ++kk) s[tt] = mfma32x32x16<T>(kfr[tt][kk], qf[kk], s[tt]);
            }
        } else {
#pragma unroll
        for (int tt = 0; tt < NS; ++tt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[tt][r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < D / 16; ++kk) {
                const i32x4 kf = lds_read_b128(kb, tt * 32 * L::KS + kk * 32);
                s[tt] = mfma32x32x16<T>(kf, qf[kk], s[tt]);
            }
        }
        }

        if (t >= t_mask) {
            const int lim = causal ? q0 + l32 + off_diag : Nk;
#pragma unroll
            for (int tt = 0; tt < NS; ++tt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = t * KTL + tt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h32;
                    if (key >= Nk || key > lim) s[tt][r] = -INFINITY;
                }
        }

        float mx, my;
        if constexpr (NS == 2) {
            mx = max3(s[0][0], s[1][0], s[0][1]);
            my = max3(s[1][1], s[0][2], s[1][2]);
#pragma unroll
            for (int r = 3; r < 15; r += 2) {
                mx = max3(mx, s[0][r], s[1][r]);
                my = max3(my, s[0][r + 1], s[1][r + 1]);
            }
            mx = max3(mx, my, max3(s[0][15], s[1][15], mx));
        } else {
            mx = max3(s[0][0], s[0][1], s[0][2]);
            my = max3(s[0][3], s[0][4], s[0][5]);
#pragma unroll
            for (int i = 6; i + 3 < NS * 16; i += 4) {
                mx = max3(mx, s[i / 16][i % 16], s[(i + 1) / 16][(i + 1) % 16]);
                my = max3(my, s[(i + 2) / 16][(i + 2) % 16], s[(i + 3) / 16][(i + 3) % 16]);
            }
            mx = max3(mx, my, max3(s[NS - 1][14], s[NS - 1][15], mx));
        }
        if constexpr ((OPT & kOptPermlane) != 0) mx = xor32_max(mx);
        else mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float m_new = fmaxf(m_run, mx * c);
        if constexpr ((OPT & kOptDefer) != 0) m_new = mx * c > m_run + kDeferThr ? m_new : m_run;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        float rs = 0.f;
#pragma unroll
        for (int tt = 0; tt < NS; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(fmaf(s[tt][r], c, -m_new));
                s[tt][r] = p;
                if constexpr ((OPT & kOptRoundedSum) == 0) rs += p;
            }
        if constexpr ((OPT & kOptRoundedSum) == 0) l_run = fmaf(l_run, alpha, rs);
        if (!LAZY || __ballot(alpha != 1.f)) {
#pragma unroll
            for (int d = 0; d < D / 32; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[d][r] *= alpha;
        }

        i32x4 pb[NS][2];
#pragma unroll
        for (int tt = 0; tt < NS; ++tt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const int r0 = 8 * s2;
                pb[tt][s2] = i32x4{(int)pack2<T>(s[tt][r0 + 0], s[tt][r0 + 1]),
                                   (int)pack2<T>(s[tt][r0 + 2], s[tt][r0 + 3]),
                                   (int)pack2<T>(s[tt][r0 + 4], s[tt][r0 + 5]),
                                   (int)pack2<T>(s[tt][r0 + 6], s[tt][r0 + 7])};
            }
        if constexpr ((OPT & kOptRoundedSum) != 0) {
            float r0 = 0.f, r1 = 0.f;
#pragma unroll
            for (int tt = 0; tt < NS; ++tt)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    r0 = add_pair<T>((uint32_t)pb[tt][s2][0], r0);
                    r1 = add_pair<T>((uint32_t)pb[tt][s2][1], r1);
                    r0 = add_pair<T>((uint32_t)pb[tt][s2][2], r0);
                    r1 = add_pair<T>((uint32_t)pb[tt][s2][3], r1);
                }
            l_run = fmaf(l_run, alpha, r0 + r1);
        }
        if constexpr ((OPT & kOptBatchReads) != 0) {
            // V^T fragments of one 32-column block read as a batch, the next
            // block's batch issued before this block's MFMAs
            i32x4 vf[2][NS][2];
            auto read_v = [&](int dblk, i32x4 (&dst)[NS][2]) {
#pragma unroll
                for (int tt = 0; tt < NS; ++tt)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        const int ro = (tt * 32 + 16 * s2) * L::VS + dblk * 64;
                        const i32x2 lo = lds_read_tr16(vb, ro);
                        const i32x2 hi = lds_read_tr16(vb, ro + 8 * L::VS);
                        dst[tt][s2] = i32x4{lo.x, lo.y, hi.x, hi.y};
                    }
            };
            read_v(0, vf[0]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int dblk = 0; dblk < D / 32; ++dblk) {
                if (dblk + 1 < D / 32) read_v(dblk + 1, vf[(dblk + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int tt = 0; tt < NS; ++tt)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2)
                        oacc[dblk] = mfma32x32x16<T>(vf[dblk & 1][tt][s2], pb[tt][s2], oacc[dblk]);
            }
        } else {
#pragma unroll
        for (int dblk = 0; dblk < D / 32; ++dblk)
#pragma unroll
            for (int tt = 0; tt < NS; ++tt)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const int ro = (tt * 32 + 16 * s2) * L::VS + dblk * 64;
                    const i32x2 lo = lds_read_tr16(vb, ro);
                    const i32x2 hi = lds_read_tr16(vb, ro + 8 * L::VS);
                    oacc[dblk] = mfma32x32x16<T>(i32x4{lo.x, lo.y, hi.x, hi.y}, pb[tt][s2], oacc[dblk]);
                }
        }

        if (t + 1 < nt) store_tile((t + 1) & 1);
        __syncthreads();
    }

    if constexpr ((OPT & kOptPrio) != 0) __builtin_amdgcn_s_setprio(0);
    float l;
    if constexpr ((OPT & kOptPermlane) != 0) l = xor32_sum(l_run);
    else l = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = l > 0.f ? 1.f / l : 0.f;
    const int qr = q0 + l32;
    if (qr < Nq) {
        uint16_t* op = o + b * st.ob + hq * st.oh + (int64_t)qr * st.on;
        if constexpr ((OPT & kOptWideStore) != 0) {
            // group k = 4*dblk + i holds columns 8k+4*h32 .. +3 of row qr; after
            // swapping (k, k+1): lower lanes hold cols 8k..8k+7, upper 8k+8..8k+15
#pragma unroll
            for (int dblk = 0; dblk < D / 32; ++dblk)
#pragma unroll
                for (int i = 0; i < 4; i += 2) {
                    const f32x16& a = oacc[dblk];
                    uint32_t ax = pack2<T>(a[4 * i] * inv, a[4 * i + 1] * inv);
                    uint32_t ay = pack2<T>(a[4 * i + 2] * inv, a[4 * i + 3] * inv);
                    uint32_t bx = pack2<T>(a[4 * i + 4] * inv, a[4 * i + 5] * inv);
                    uint32_t by = pack2<T>(a[4 * i + 6] * inv, a[4 * i + 7] * inv);
                    const auto rx = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
                    const auto ry = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
                    const int d = dblk * 32 + 8 * i + 8 * h32;
                    *reinterpret_cast<i32x4*>(op + d) =
                        i32x4{(int)rx[0], (int)ry[0], (int)rx[1], (int)ry[1]};
                }
        } else {
#pragma unroll
            for (int dblk = 0; dblk < D / 32; ++dblk)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int d = dblk * 32 + 8 * i + 4 * h32;
                    const i32x2 w = {(int)pack2<T>(oacc[dblk][4 * i] * inv, oacc[dblk][4 * i + 1] * inv),
                                     (int)pack2<T>(oacc[dblk][4 * i + 2] * inv, oacc[dblk][4 * i + 3] * inv)};
                    *reinterpret_cast<i32x2*>(op + d) = w;
                }
        }
    }
}

// --------------------------------------------------------------------------
// Generic kernel: 256 threads own 32 query rows (8 threads per row, each
// thread owns columns sub + 8u of the score tile and d = sub + 8u of O).
constexpr int GQ = 32, GK = 64, GDMAX = 128;

template <typename T>
__global__ __launch_bounds__(256) void attn_fwd_generic(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
    T* __restrict__ o, int H, int group, int Nq, int Nk, int D, V7Strides st,
    float scale, int causal, int qblocks) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    const int ldq = D + 1;
    float* Qs = gsm;                 // [GQ][D+1]
    float* Ks = Qs + GQ * ldq;       // [GK][D+1]
    float* Vs = Ks + GK * ldq;       // [GK][D]
    float* Ps = Vs + GK * D;         // [GQ][GK+1]

    const int tid = threadIdx.x, row = tid >> 3, sub = tid & 7;
    const int bh = blockIdx.x / qblocks, qblk = blockIdx.x % qblocks;
    const int b = bh / H, hq = bh % H, hk = hq / group;
    const int q0 = qblk * GQ;
    const int off_diag = Nk - Nq;
    const T* qp = q + b * st.qb + hq * st.qh;
    const T* kp = k + b * st.kb + hk * st.kh;
    const T* vp = v + b * st.vb + hk * st.vh;

    for (int i = tid; i < GQ * D; i += 256) {
        const int r = i / D, d = i % D;
        Qs[r * ldq + d] = (q0 + r < Nq) ? elem<T>::to_f32(qp[(int64_t)(q0 + r) * st.qn + d]) : 0.f;
    }

    float acc[GDMAX / 8];
#pragma unroll
    for (int u = 0; u < GDMAX / 8; ++u) acc[u] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const int qi = q0 + row;
    const int lim = causal ? qi + off_diag : Nk - 1;
    int kv_end = Nk;
    if (causal) kv_end = min(Nk, q0 + GQ + off_diag);

    for (int k0 = 0; k0 < kv_end; k0 += GK) {
        __syncthreads();
        for (int i = tid; i < GK * D; i += 256) {
            const int r = i / D, d = i % D;
            const bool ok = k0 + r < Nk;
            Ks[r * ldq + d] = ok ? elem<T>::to_f32(kp[(int64_t)(k0 + r) * st.kn + d]) : 0.f;
            Vs[r * D + d] = ok ? elem<T>::to_f32(vp[(int64_t)(k0 + r) * st.vn + d]) : 0.f;
        }
        __syncthreads();
        float sc[GK / 8];
        float mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < GK / 8; ++u) {
            const int j = sub + 8 * u;
            float dot = 0.f;
            for (int d = 0; d < D; ++d) dot = fmaf(Qs[row * ldq + d], Ks[j * ldq + d], dot);
            const int key = k0 + j;
            dot = (key < Nk && key <= lim) ? dot * scale : -INFINITY;
            sc[u] = dot;
            mx = fmaxf(mx, dot);
        }
#pragma unroll
        for (int o2 = 1; o2 < 8; o2 <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o2, 64));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = (m_new == -INFINITY) ? 1.f : expf(m_run - m_new);
        float rs = 0.f;
#pragma unroll
        for (int u = 0; u < GK / 8; ++u) {
            const float p = (m_new == -INFINITY) ? 0.f : expf(sc[u] - m_new);
            Ps[row * (GK + 1) + sub + 8 * u] = p;
            rs += p;
        }
#pragma unroll
        for (int o2 = 1; o2 < 8; o2 <<= 1) rs += __shfl_xor(rs, o2, 64);
        l_run = l_run * alpha + rs;
        m_run = m_new;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < GDMAX / 8; ++u) {
            const int d = sub + 8 * u;
            if (d < D) {
                float a = acc[u] * alpha;
                for (int j = 0; j < GK; ++j) a = fmaf(Ps[row * (GK + 1) + j], Vs[j * D + d], a);
                acc[u] = a;
            }
        }
    }
    if (qi < Nq) {
        const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
        T* op = o + b * st.ob + hq * st.oh + (int64_t)qi * st.on;
#pragma unroll
        for (int u = 0; u < GDMAX / 8; ++u) {
            const int d = sub + 8 * u;
            if (d < D) op[d] = elem<T>::from_f32(acc[u] * inv);
        }
    }
}

// attn_fwd_v2 (variant 21), the end of plan_flash's chain; a variant number no
// stage of the chain knows ends here too, as an error
template <typename T, int D>
int launch_v2(const FlashCall& f, const FlashPlan& plan, const void* q, const void* k, const void* v, void* o,
              hipStream_t stream) {
    constexpr int nw = 8;
    const int qblocks = cdiv(f.Nq, nw * QW);
    const int64_t nb = (int64_t)f.B * f.H * qblocks;
    PLI_REQUIRE(nb < (1ll << 31), "pli_flash_attn_fwd: grid too large");
    PLI_REQUIRE(plan.family == FlashFamily::v2, "pli_flash_attn_fwd: unknown variant %d", plan.variant);
    const float c = f.scale * 1.4426950408889634f;  // fold log2(e) into the scale
    hipLaunchKernelGGL((attn_fwd_v2<T, D, nw, true, 13>), dim3((unsigned)nb), dim3(nw * 64), 0, stream,
                       (const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v, (uint16_t*)o, f.H, f.group, f.Nq,
                       f.Nk, f.st, c, (int)f.causal, qblocks, (int)nb);
    return launch_status("attn_fwd_v2");
}

// the MFMA families of a plan (flash_plan.h plan_flash holds the routing rules)
int launch_mfma(const FlashCall& f, const FlashPlan& plan, const void* q, const void* k, const void* v, void* o,
                hipStream_t stream) {
    switch (plan.family) {
        case FlashFamily::pp64:
        case FlashFamily::v13:
            return launch_attn_v13(f, plan, q, k, v, o, stream);
        case FlashFamily::v12:
            return launch_attn_v12(f, plan, q, k, v, o, stream);
        case FlashFamily::v7:
            return launch_attn_v7(f, plan, q, k, v, o, stream);
        default:
            if (!f.fp16)
                return f.D == 128 ? launch_v2<bf16_t, 128>(f, plan, q, k, v, o, stream)
                                  : launch_v2<bf16_t, 64>(f, plan, q, k, v, o, stream);
            return f.D == 128 ? launch_v2<f16_t, 128>(f, plan, q, k, v, o, stream)
                              : launch_v2<f16_t, 64>(f, plan, q, k, v, o, stream);
    }
}

template <typename T>
int launch_generic(const FlashCall& f, const void* q, const void* k, const void* v, void* o, hipStream_t stream) {
    const int D = f.D, qblocks = cdiv(f.Nq, GQ);
    const int64_t nb = (int64_t)f.B * f.H * qblocks;
    PLI_REQUIRE(nb < (1ll << 31), "pli_flash_attn_fwd: grid too large");
    const size_t lds = sizeof(float) * ((size_t)GQ * (D + 1) + (size_t)GK * (D + 1) +
                                        (size_t)GK * D + (size_t)GQ * (GK + 1));
    hipLaunchKernelGGL((attn_fwd_generic<T>), dim3((unsigned)nb), dim3(256), lds, stream,
                       (const T*)q, (const T*)k, (const T*)v, (T*)o, f.H, f.group, f.Nq, f.Nk, D, f.st,
                       f.scale, (int)f.causal, qblocks);
    return launch_status("attn_fwd_generic");
}

}  // namespace
}  // namespace pli

// Same contract as pli_flash_attn_fwd plus an explicit kernel variant
// (include/pli.h tuning section); variant < 0 selects the default.
extern "C" int pli_flash_attn_fwd_variant(const void* q, const void* k, const void* v, void* o,
                                          int batch, int heads, int kv_heads, int n_q, int n_kv,
                                          int head_dim, const int64_t* strides, float scale,
                                          int causal, int dtype, void* stream, int variant) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(batch >= 0 && heads > 0 && kv_heads > 0 && n_q >= 0 && n_kv >= 0 && head_dim > 0,
                "pli_flash_attn_fwd: bad shape B=%d H=%d Hkv=%d Nq=%d Nk=%d D=%d", batch, heads,
                kv_heads, n_q, n_kv, head_dim);
    PLI_REQUIRE(heads % kv_heads == 0, "pli_flash_attn_fwd: heads %d not a multiple of kv_heads %d",
                heads, kv_heads);
    PLI_REQUIRE(dtype == PLI_F32 || dtype == PLI_F16 || dtype == PLI_BF16,
                "pli_flash_attn_fwd: bad dtype %d", dtype);
    PLI_REQUIRE(std::isfinite(scale), "pli_flash_attn_fwd: non-finite scale");
    // empty operands may be NULL (pli.h): no output rows -> nothing to do; no
    // keys -> O = 0 (the generic kernel reads no K / V)
    if (batch == 0 || n_q == 0) return PLI_OK;
    PLI_REQUIRE(q && o && strides && (n_kv == 0 || (k && v)), "pli_flash_attn_fwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    FlashCall f{batch, heads, heads / kv_heads, n_q, n_kv, head_dim, dtype == PLI_F16, causal != 0,
                V7Strides{strides[0], strides[1], strides[2], strides[3], strides[4], strides[5],
                          strides[6], strides[7], strides[8], strides[9], strides[10], strides[11]},
                scale, 0};
    f.mfma_operands = dtype != PLI_F32 && aligned16(q) && aligned16(k) && aligned16(v) && aligned16(o);
    if (f.mfma_operands) f.cus = cu_count(s);
    const FlashPlan plan = plan_flash(f, variant);
    if (plan.family != FlashFamily::generic) return launch_mfma(f, plan, q, k, v, o, s);
    if (head_dim > GDMAX) {
        set_error("pli_flash_attn_fwd: head_dim %d > %d unsupported on the generic path", head_dim,
                  GDMAX);
        return PLI_EUNSUPPORTED;
    }
    if (dtype == PLI_F32) return launch_generic<float>(f, q, k, v, o, s);
    return f.fp16 ? launch_generic<f16_t>(f, q, k, v, o, s) : launch_generic<bf16_t>(f, q, k, v, o, s);
}

extern "C" int pli_flash_attn_fwd(const void* q, const void* k, const void* v, void* o,
                                  int batch, int heads, int kv_heads, int n_q, int n_kv,
                                  int head_dim, const int64_t* strides, float scale,
                                  int causal, int dtype, void* stream) {
    return pli_flash_attn_fwd_variant(q, k, v, o, batch, heads, kv_heads, n_q, n_kv, head_dim,
                                      strides, scale, causal, dtype, stream, -1);
}
