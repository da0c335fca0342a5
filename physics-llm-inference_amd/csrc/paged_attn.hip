// Decode attention over a paged KV pool, and the paged append that feeds it,
// for gfx950.
//
// The device half of ch07/paged_memory.py:16-51 (PagedKVCache allocates the
// pools k_cache / v_cache [num_blocks, num_layers, block_size, num_heads,
// head_dim]) that the reference leaves unwritten (:171-175: "Attention kernel
// reads from scattered blocks / uses block table for indirection").
//
// attn_decode_paged<T, D> is attn_decode_chunk<T, D, 13> (decode_attn.hip)
// with two changes: a row's address comes from the block table
// (paged_plan.h), and the valid length is per sequence,
// n_kv(b) = clamp(seq_lens[b] + n_kv_add, 0, max_kv), read on the device, so
// the call replays in a captured graph.
//   * one workgroup = (batch, chunk, kv head), kv head innermost; 4 waves of
//     32-key steps; whole-row non-temporal 16-byte loads into wave-private LDS
//     tiles; S^T = K . Q^T and O^T += V^T . P^T by v_mfma_f32_16x16x32; fp32
//     statistics; waves merge in LDS; fp32 partials to the workspace when
//     splits > 1, merged by attn_decode_paged_combine.
//   * a step's 32 keys start at a multiple of 32, so with a power-of-two block
//     size >= 16 they lie in at most two pages: the pages of block(key0) and
//     block(key0 + 16).  Both indices are wave-uniform and are fetched two
//     steps ahead of the K/V loads that need them (the pages of step t + 2
//     while step t computes), so the dependent table read is off the critical
//     path; load_step only selects between the two prefetched values.
//   * every load runs with a clamped address (key <= n_kv - 1, block index
//     inside the table row, page inside the pool) and the scores are masked
//     afterwards; no load sits behind a runtime select.
//   * chunks wholly past a sequence's length run no step and write the
//     (m = -1e30, l = 0, O = 0) partial; a sequence of length 0 gives O = 0.
// attn_decode_paged_generic covers every other case (fp32, other head dims,
// any block size, more rows per kv head): one wave per (batch, head, query
// row), online softmax in fp32 -- a correctness path, not tuned.
// attn_decode_paged_fp8 / attn_decode_paged_generic_fp8 / kv_append_paged_fp8
// are the same three over 1-byte pools of fp8 e4m3 codes (below, "1-byte
// pools"); the 16-bit kernels are not touched by them.
#include <cmath>

#include "fp8_kv.h"
#include "paged_plan.h"
#include "pli_common.h"

namespace pli {
namespace {

inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// element strides: q / o {batch, head, row}; pools {page, token, head}
struct PagedStrides {
    int64_t qb, qh, qn, ob, oh, on;
    PagedPool k, v;
};

template <int D> struct PagedLayout {
    static constexpr int KS = 2 * D + 16;             // K row stride in LDS (bytes)
    static constexpr int VS = 2 * D + 32;             // V row stride in LDS (bytes)
    static constexpr int KBYTES = DEC_STEP * KS;
    static constexpr int WAVE_BYTES = KBYTES + DEC_STEP * VS;  // per-wave K + V tile
    static constexpr int MERGE_BYTES = DEC_WAVES * (DEC_MAXM * D + 2 * DEC_MAXM) * 4;
    static constexpr int LDS = WAVE_BYTES * DEC_WAVES > MERGE_BYTES ? WAVE_BYTES * DEC_WAVES
                                                                     : MERGE_BYTES;
};

template <typename T, int D>
__global__ __launch_bounds__(256, 2) void attn_decode_paged(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, uint16_t* __restrict__ o, float* __restrict__ part_o,
    float2* __restrict__ part_ml, const int32_t* __restrict__ table,
    const int32_t* __restrict__ seq_lens, int Hkv, int G, int Nq, int M, PagedStrides st,
    PagedTable tb, float c, int causal, int chunk, int splits, int max_kv, int nk_add) {
    using L = PagedLayout<D>;
    constexpr int KSTEPS = D / 32;  // 32-d k-steps of K.Q^T
    constexpr int DB = D / 16;      // 16-d blocks of O
    __shared__ __attribute__((aligned(16))) char smem[L::LDS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, g = lane >> 4;
    // block order: (b, split, hk) with the kv head innermost, so co-resident
    // workgroups sweep the same keys (the same pages) of all heads
    const int hk = blockIdx.x % Hkv;
    const int split = (blockIdx.x / Hkv) % splits;
    const int b = blockIdx.x / (Hkv * splits);
    const int bh = b * Hkv + hk;
    const int Nk = paged_seq_len(seq_lens[b], nk_add, max_kv);

    // query row of this lane's MFMA column
    const int m_row = l16;
    const bool row_ok = m_row < M;
    const int qi = row_ok ? m_row / G : 0, gi = row_ok ? m_row % G : 0;
    const int hq = hk * G + gi;
    i32x4 qf[KSTEPS];
    {
        const uint16_t* src = q + b * st.qb + hq * st.qh + (int64_t)qi * st.qn + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const i32x4 x = *reinterpret_cast<const i32x4*>(src + 32 * ks);
            qf[ks] = row_ok ? x : i32x4{0, 0, 0, 0};
        }
    }
    // bottom-right causal per sequence: row qi sees keys <= n_kv(b) - Nq + qi
    const int lim = causal ? Nk - Nq + qi : Nk - 1;

    const int c0 = split * chunk;
    const int per_wave = chunk / DEC_WAVES;
    const int w0 = c0 + wave * per_wave;
    const int w1 = min(w0 + per_wave, Nk);
    const int nsteps = w1 > w0 ? cdiv(w1 - w0, DEC_STEP) : 0;

    // row-major loads: lane loads 16-byte chunk rch of row i*RPI + rrow of the
    // step for instruction i = kb*KSTEPS + ks
    constexpr int CPR = D / 8, RPI = 64 / CPR;
    const int rrow = lane / CPR, rch = lane % CPR;
    const uint16_t* kp = k + 8 * rch;
    const uint16_t* vp = v + 8 * rch;
    i32x4 kc[2][KSTEPS], vc[2][KSTEPS];
    auto ld = [](const uint16_t* p) {
        return __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(p));
    };
    // the table entries of the two pages a step starting at key0 (a multiple
    // of 32) can touch, raw: clamping here would wait for the load at once
    auto pages = [&](int key0, int& e0, int& e1) {
        e0 = table[paged_table_index(b, paged_block_pow2(key0, tb), tb)];
        e1 = table[paged_table_index(b, paged_block_pow2(key0 + 16, tb), tb)];
    };
    auto load_step = [&](int key0, int e0, int e1, i32x4 (&kr)[2][KSTEPS], i32x4 (&vr)[2][KSTEPS]) {
        const int blk0 = paged_block_pow2(key0, tb);
        const int p0 = paged_clamp_page(e0, tb), p1 = paged_clamp_page(e1, tb);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) {
                const int key = min(key0 + (kb * KSTEPS + ks) * RPI + rrow, Nk - 1);
                const int page = paged_block_pow2(key, tb) == blk0 ? p0 : p1;
                kr[kb][ks] = ld(kp + paged_offset_pow2(page, key, hk, tb, st.k));
                vr[kb][ks] = ld(vp + paged_offset_pow2(page, key, hk, tb, st.v));
            }
        }
    };

    char* kt = smem + wave * L::WAVE_BYTES;
    char* vt = kt + L::KBYTES;
    const int vw = rrow * L::VS + rch * 16;
    const int kw = rrow * L::KS + rch * 16;                     // K row-major write
    const int kr_off = l16 * L::KS + g * 16;                    // K fragment read
    const int qq = l16 >> 2, pp = lane & 3;
    const int vr_off = (4 * g + qq) * L::VS + 8 * pp;           // tr read: key 4g+qq, col 4pp

    f32x4 oacc[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d) oacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;

    // pn0 / pn1: the table entries of the step after the one whose loads are in flight
    int pn0 = 0, pn1 = 0;
    if (nsteps > 0) {
        int p0, p1;
        pages(w0, p0, p1);
        pages(w0 + DEC_STEP, pn0, pn1);
        load_step(w0, p0, p1, kc, vc);
    }
    for (int it = 0; it < nsteps; ++it) {
        const int key0 = w0 + it * DEC_STEP;
        i32x4 kn[2][KSTEPS], vn[2][KSTEPS];
        if (it + 1 < nsteps) {
            // step t+2's table entries first (consumed a whole step later),
            // then step t+1's K/V rows with the entries fetched a step ago
            int f0, f1;
            pages(key0 + 2 * DEC_STEP, f0, f1);
            load_step(key0 + DEC_STEP, pn0, pn1, kn, vn);
            pn0 = f0, pn1 = f1;
        }

        // K and V step -> LDS (row-major, padded)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) {
                const int row0 = (kb * KSTEPS + ks) * RPI;
                lds_write_b128(vt, vw + row0 * L::VS, vc[kb][ks]);
                lds_write_b128(kt, kw + row0 * L::KS, kc[kb][ks]);
            }
        // the tile is wave-private and a wave's LDS operations execute in
        // order; the fence only stops the compiler moving the transposed reads
        // (a different pointer type) above these writes
        asm volatile("" ::: "memory");

        f32x4 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            s[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) {
                const i32x4 kf = lds_read_b128(kt, kr_off + 16 * kb * L::KS + 64 * ks);
                s[kb] = mfma16x16x32<T>(kf, qf[ks], s[kb]);
            }
        }
        // mask: keys past this wave's range / the sequence / the causal limit
        const int hi = min(w1 - 1, lim);
        if (key0 + DEC_STEP - 1 > hi) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (key0 + 16 * kb + 4 * g + r > hi) s[kb][r] = -INFINITY;
        }
        float mx = max3(s[0][0], s[0][1], s[0][2]);
        mx = max3(mx, s[0][3], s[1][0]);
        mx = max3(mx, s[1][1], s[1][2]);
        mx = fmaxf(mx, s[1][3]);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx * c);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[kb][r] = __builtin_amdgcn_exp2f(fmaf(s[kb][r], c, -m_new));
        const uint32_t p0 = pack2<T>(s[0][0], s[0][1]), p1 = pack2<T>(s[0][2], s[0][3]);
        const uint32_t p2 = pack2<T>(s[1][0], s[1][1]), p3 = pack2<T>(s[1][2], s[1][3]);
        const i32x4 pb = {(int)p0, (int)p1, (int)p2, (int)p3};
        l_run = fmaf(l_run, alpha, add_pair<T>(p0, add_pair<T>(p1, add_pair<T>(p2, add_pair<T>(p3, 0.f)))));

#pragma unroll
        for (int d = 0; d < DB; ++d) {
            const i32x2 lo = lds_read_tr16(vt, vr_off + 32 * d);
            const i32x2 hi2 = lds_read_tr16(vt, vr_off + 32 * d + 16 * L::VS);
            oacc[d] = mfma16x16x32<T>(i32x4{lo.x, lo.y, hi2.x, hi2.y}, pb, oacc[d] * alpha);
        }
        asm volatile("" ::: "memory");  // next step's writes stay below these reads
        if (it + 1 < nsteps) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int ks = 0; ks < KSTEPS; ++ks) {
                    kc[kb][ks] = kn[kb][ks];
                    vc[kb][ks] = vn[kb][ks];
                }
        }
    }
    // row sum over the 4 lane groups holding the row
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);

    // ---- merge the 4 waves in LDS: [wave][row][D] O, then [wave][row] (m, l)
    __syncthreads();  // every wave is done with its tiles
    float* mo = reinterpret_cast<float*>(smem);
    float* mml = mo + DEC_WAVES * DEC_MAXM * D;
#pragma unroll
    for (int d = 0; d < DB; ++d)
        *reinterpret_cast<f32x4*>(mo + (wave * DEC_MAXM + l16) * D + 16 * d + 4 * g) = oacc[d];
    if (g == 0) {
        mml[(wave * DEC_MAXM + l16) * 2] = m_run;
        mml[(wave * DEC_MAXM + l16) * 2 + 1] = l_run;
    }
    __syncthreads();
    constexpr int CH = D / 4;  // float4 chunks per row
    for (int item = tid; item < M * CH; item += 256) {
        const int row = item / CH, cc = item % CH;
        float mw[DEC_WAVES], mt = -1e30f;
#pragma unroll
        for (int w = 0; w < DEC_WAVES; ++w) {
            mw[w] = mml[(w * DEC_MAXM + row) * 2];
            mt = fmaxf(mt, mw[w]);
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        float lt = 0.f;
#pragma unroll
        for (int w = 0; w < DEC_WAVES; ++w) {
            const float wgt = __builtin_amdgcn_exp2f(mw[w] - mt);
            lt = fmaf(mml[(w * DEC_MAXM + row) * 2 + 1], wgt, lt);
            acc += *reinterpret_cast<const f32x4*>(mo + (w * DEC_MAXM + row) * D + 4 * cc) * wgt;
        }
        if (splits == 1) {
            // a row that saw no key (empty sequence, causal row above the
            // diagonal) has l = 0: it is written as 0
            const float inv = lt > 0.f ? 1.f / lt : 0.f;
            const int rqi = row / G, rgi = row % G;
            uint16_t* op = o + b * st.ob + (hk * G + rgi) * st.oh + (int64_t)rqi * st.on + 4 * cc;
            *reinterpret_cast<i32x2*>(op) =
                i32x2{(int)pack2<T>(acc[0] * inv, acc[1] * inv), (int)pack2<T>(acc[2] * inv, acc[3] * inv)};
        } else {
            const int64_t prow = ((int64_t)bh * splits + split) * M + row;
            *reinterpret_cast<f32x4*>(part_o + prow * D + 4 * cc) = acc;
            if (cc == 0) part_ml[prow] = float2{mt, lt};
        }
    }
}

// Merge `splits` partial (m, l, O) rows per (batch, kv head, row) into the
// output: attn_decode_combine of decode_attn.hip (which lives in that file's
// unnamed namespace), same arithmetic.  One workgroup per (bh, row); thread =
// (16-byte chunk of the row, split lane).  Empty chunks' (-1e30, 0, 0)
// partials fold in with weight 1 on a zero sum: no branch.
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_decode_paged_combine(
    const float* __restrict__ part_o, const float2* __restrict__ part_ml, uint16_t* __restrict__ o,
    int Hkv, int G, int M, PagedStrides st, int splits) {
    constexpr int CH = D / 4, LANES = 256 / CH;
    __shared__ f32x4 red_o[LANES][CH];
    __shared__ float2 red_ml[LANES][CH];
    const int tid = threadIdx.x, cc = tid % CH, sl = tid / CH;
    const int row = blockIdx.x % M, bh = blockIdx.x / M;
    const int b = bh / Hkv, hk = bh % Hkv;
    const int64_t base = (int64_t)bh * splits * M + row;  // + s*M
    float mt = -1e30f, lt = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int s = sl; s < splits; s += LANES) {
        const int64_t pr = base + (int64_t)s * M;
        const float2 ml = part_ml[pr];
        const f32x4 po = *reinterpret_cast<const f32x4*>(part_o + pr * D + 4 * cc);
        const float mn = fmaxf(mt, ml.x);
        const float wa = __builtin_amdgcn_exp2f(mt - mn), wb = __builtin_amdgcn_exp2f(ml.x - mn);
        acc = acc * wa + po * wb;
        lt = lt * wa + ml.y * wb;
        mt = mn;
    }
    red_o[sl][cc] = acc;
    red_ml[sl][cc] = float2{mt, lt};
    __syncthreads();
    if (sl == 0) {
        for (int j = 1; j < LANES; ++j) {
            const float2 ml = red_ml[j][cc];
            const float mn = fmaxf(mt, ml.x);
            const float wa = __builtin_amdgcn_exp2f(mt - mn), wb = __builtin_amdgcn_exp2f(ml.x - mn);
            acc = acc * wa + red_o[j][cc] * wb;
            lt = lt * wa + ml.y * wb;
            mt = mn;
        }
        const float inv = lt > 0.f ? 1.f / lt : 0.f;
        const int rqi = row / G, rgi = row % G;
        uint16_t* op = o + b * st.ob + (hk * G + rgi) * st.oh + (int64_t)rqi * st.on + 4 * cc;
        *reinterpret_cast<i32x2*>(op) =
            i32x2{(int)pack2<T>(acc[0] * inv, acc[1] * inv), (int)pack2<T>(acc[2] * inv, acc[3] * inv)};
    }
}

// Any dtype, head_dim <= 256, any block size, any group size: one wave per
// (batch, head, query row); lane l owns dims l, l + 64, ...; keys in order,
// fp32 online softmax.  Correctness path only.
constexpr int GEN_MAXD = 256, GEN_DPL = GEN_MAXD / 64;
template <typename T>
__global__ __launch_bounds__(64) void attn_decode_paged_generic(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ o,
    const int32_t* __restrict__ table, const int32_t* __restrict__ seq_lens, int H, int G, int Nq,
    int D, PagedStrides st, PagedTable tb, float scale, int causal, int max_kv, int nk_add) {
    const int lane = threadIdx.x;
    const int qi = blockIdx.x % Nq;
    const int h = (blockIdx.x / Nq) % H;
    const int b = blockIdx.x / (Nq * H);
    const int hk = h / G;
    const int Nk = paged_seq_len(seq_lens[b], nk_add, max_kv);
    // keys this row sees: j <= lim (bottom-right causal per sequence)
    const int nvis = min(Nk, causal ? Nk - Nq + qi + 1 : Nk);
    const T* qrow = q + b * st.qb + h * st.qh + (int64_t)qi * st.qn;
    float qv[GEN_DPL], acc[GEN_DPL];
#pragma unroll
    for (int i = 0; i < GEN_DPL; ++i) {
        const int d = lane + 64 * i;
        qv[i] = d < D ? elem<T>::to_f32(qrow[d]) : 0.f;
        acc[i] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int j = 0; j < nvis; ++j) {
        const T* krow = k + paged_key_offset(table, b, j, hk, tb, st.k);
        const T* vrow = v + paged_key_offset(table, b, j, hk, tb, st.v);
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < GEN_DPL; ++i) {
            const int d = lane + 64 * i;
            if (d < D) dot = fmaf(qv[i], elem<T>::to_f32(krow[d]), dot);
        }
        const float s = wave_sum(dot) * scale;
        const float m_new = fmaxf(m, s);
        const float a = __expf(m - m_new), p = __expf(s - m_new);
        l = fmaf(l, a, p);
#pragma unroll
        for (int i = 0; i < GEN_DPL; ++i) {
            const int d = lane + 64 * i;
            if (d < D) acc[i] = fmaf(acc[i], a, p * elem<T>::to_f32(vrow[d]));
        }
        m = m_new;
    }
    const float inv = l > 0.f ? 1.f / l : 0.f;  // no visible key: O = 0
    T* orow = o + b * st.ob + h * st.oh + (int64_t)qi * st.on;
#pragma unroll
    for (int i = 0; i < GEN_DPL; ++i) {
        const int d = lane + 64 * i;
        if (d < D) orow[d] = elem<T>::from_f32(acc[i] * inv);
    }
}

// Append n_new tokens of K and V per sequence at logical positions
// seq_lens[b] + t, through the block table; positions past the table row's
// max_blocks_per_seq * block_size tokens are dropped.  One thread per 16-byte
// chunk; every stride here is in bytes.  seq_lens is not advanced.
struct AppendStrides {
    int64_t kb, kh, kn, vb, vh, vn;  // the new tensors: batch, head, token
    PagedPool k, v;
};
__global__ __launch_bounds__(256) void kv_append_paged_kernel(
    const char* __restrict__ kn, const char* __restrict__ vn, char* __restrict__ kpool,
    char* __restrict__ vpool, const int32_t* __restrict__ table,
    const int32_t* __restrict__ seq_lens, int B, int T, int Hkv, int cpr, AppendStrides st,
    PagedTable tb) {
    const int64_t total = (int64_t)B * T * Hkv * cpr;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = idx % cpr;
    const int h = (idx / cpr) % Hkv;
    const int t = (idx / ((int64_t)cpr * Hkv)) % T;
    const int b = idx / ((int64_t)cpr * Hkv * T);
    const int64_t pos = (int64_t)seq_lens[b] + t;
    if (pos < 0 || pos >= (int64_t)tb.max_blocks_per_seq * tb.block_size) return;
    const char* ks = kn + b * st.kb + h * st.kh + (int64_t)t * st.kn + 16 * ch;
    const char* vs = vn + b * st.vb + h * st.vh + (int64_t)t * st.vn + 16 * ch;
    char* kd = kpool + paged_key_offset(table, b, (int)pos, h, tb, st.k) + 16 * ch;
    char* vd = vpool + paged_key_offset(table, b, (int)pos, h, tb, st.v) + 16 * ch;
    *reinterpret_cast<i32x4*>(kd) = *reinterpret_cast<const i32x4*>(ks);
    *reinterpret_cast<i32x4*>(vd) = *reinterpret_cast<const i32x4*>(vs);
}

// ---- 1-byte pools: OCP fp8 e4m3fn codes, value = code * scale[kv head] --------
// attn_decode_paged_fp8<T, D> is attn_decode_paged<T, D> with the pools read as
// bytes: a lane's 16-byte load holds 16 codes, which v_cvt_scalef32_pk_*_fp8
// widens (exactly) to 16 T between the load and the LDS write, so a row-major
// step of 32 keys takes D/4 loads of K and V per wave instead of D/2, the
// staging registers halve, and the LDS image, the MFMA loop and the softmax are
// those of the 16-bit kernel.  k_scale[hk] is folded into the softmax constant
// c, v_scale[hk] into the final 1/l (one split) or into the partial's l (split-K:
// attn_decode_paged_combine, unchanged, divides by the sum of l / v_scale).
// Pool strides are in bytes.  The scales are read on the device; a scale that is
// not finite and > 0 spoils its head's rows and touches no address.
template <typename T, int D>
__global__ __launch_bounds__(256, 2) void attn_decode_paged_fp8(
    const uint16_t* __restrict__ q, const uint8_t* __restrict__ k, const uint8_t* __restrict__ v,
    uint16_t* __restrict__ o, float* __restrict__ part_o, float2* __restrict__ part_ml,
    const int32_t* __restrict__ table, const int32_t* __restrict__ seq_lens,
    const float* __restrict__ k_scale, const float* __restrict__ v_scale, int Hkv, int G, int Nq, int M,
    PagedStrides st, PagedTable tb, float c_in, int causal, int chunk, int splits, int max_kv, int nk_add) {
    using L = PagedLayout<D>;
    constexpr int KSTEPS = D / 32;  // 32-d k-steps of K.Q^T
    constexpr int DB = D / 16;      // 16-d blocks of O
    __shared__ __attribute__((aligned(16))) char smem[L::LDS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, g = lane >> 4;
    const int hk = blockIdx.x % Hkv;
    const int split = (blockIdx.x / Hkv) % splits;
    const int b = blockIdx.x / (Hkv * splits);
    const int bh = b * Hkv + hk;
    const int Nk = paged_seq_len(seq_lens[b], nk_add, max_kv);
    const float c = c_in * fp8_scale_of(k_scale, hk);
    const float vsc = fp8_scale_of(v_scale, hk);

    const int m_row = l16;
    const bool row_ok = m_row < M;
    const int qi = row_ok ? m_row / G : 0, gi = row_ok ? m_row % G : 0;
    const int hq = hk * G + gi;
    i32x4 qf[KSTEPS];
    {
        const uint16_t* src = q + b * st.qb + hq * st.qh + (int64_t)qi * st.qn + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const i32x4 x = *reinterpret_cast<const i32x4*>(src + 32 * ks);
            qf[ks] = row_ok ? x : i32x4{0, 0, 0, 0};
        }
    }
    const int lim = causal ? Nk - Nq + qi : Nk - 1;

    const int c0 = split * chunk;
    const int per_wave = chunk / DEC_WAVES;
    const int w0 = c0 + wave * per_wave;
    const int w1 = min(w0 + per_wave, Nk);
    const int nsteps = w1 > w0 ? cdiv(w1 - w0, DEC_STEP) : 0;

    // row-major loads: lane loads the 16 codes of chunk rch of row i*RPI + rrow
    // of the step in instruction i
    constexpr int CPR = D / 16, RPI = 64 / CPR, NI = DEC_STEP / RPI;
    const int rrow = lane / CPR, rch = lane % CPR;
    const uint8_t* kp = k + 16 * rch;
    const uint8_t* vp = v + 16 * rch;
    i32x4 kc[NI], vc[NI];
    auto ld = [](const uint8_t* p) {
        return __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(p));
    };
    auto pages = [&](int key0, int& e0, int& e1) {
        e0 = table[paged_table_index(b, paged_block_pow2(key0, tb), tb)];
        e1 = table[paged_table_index(b, paged_block_pow2(key0 + 16, tb), tb)];
    };
    auto load_step = [&](int key0, int e0, int e1, i32x4 (&kr)[NI], i32x4 (&vr)[NI]) {
        const int blk0 = paged_block_pow2(key0, tb);
        const int p0 = paged_clamp_page(e0, tb), p1 = paged_clamp_page(e1, tb);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int key = min(key0 + i * RPI + rrow, Nk - 1);
            const int page = paged_block_pow2(key, tb) == blk0 ? p0 : p1;
            kr[i] = ld(kp + paged_offset_pow2(page, key, hk, tb, st.k));
            vr[i] = ld(vp + paged_offset_pow2(page, key, hk, tb, st.v));
        }
    };

    char* kt = smem + wave * L::WAVE_BYTES;
    char* vt = kt + L::KBYTES;
    const int vw = rrow * L::VS + rch * 32;                     // 16 T = 32 bytes per lane
    const int kw = rrow * L::KS + rch * 32;
    const int kr_off = l16 * L::KS + g * 16;                    // K fragment read
    const int qq = l16 >> 2, pp = lane & 3;
    const int vr_off = (4 * g + qq) * L::VS + 8 * pp;           // tr read: key 4g+qq, col 4pp

    f32x4 oacc[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d) oacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;

    int pn0 = 0, pn1 = 0;
    if (nsteps > 0) {
        int p0, p1;
        pages(w0, p0, p1);
        pages(w0 + DEC_STEP, pn0, pn1);
        load_step(w0, p0, p1, kc, vc);
    }
    for (int it = 0; it < nsteps; ++it) {
        const int key0 = w0 + it * DEC_STEP;
        i32x4 kn[NI], vn[NI];
        if (it + 1 < nsteps) {
            int f0, f1;
            pages(key0 + 2 * DEC_STEP, f0, f1);
            load_step(key0 + DEC_STEP, pn0, pn1, kn, vn);
            pn0 = f0, pn1 = f1;
        }

        // the conversion point: codes -> T, then the row-major padded image
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            i32x4 lo, hi;
            fp8_widen16<T>(vc[i], lo, hi);
            lds_write_b128(vt, vw + i * RPI * L::VS, lo);
            lds_write_b128(vt, vw + i * RPI * L::VS + 16, hi);
            fp8_widen16<T>(kc[i], lo, hi);
            lds_write_b128(kt, kw + i * RPI * L::KS, lo);
            lds_write_b128(kt, kw + i * RPI * L::KS + 16, hi);
        }
        asm volatile("" ::: "memory");

        f32x4 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            s[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) {
                const i32x4 kf = lds_read_b128(kt, kr_off + 16 * kb * L::KS + 64 * ks);
                s[kb] = mfma16x16x32<T>(kf, qf[ks], s[kb]);
            }
        }
        const int hi = min(w1 - 1, lim);
        if (key0 + DEC_STEP - 1 > hi) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (key0 + 16 * kb + 4 * g + r > hi) s[kb][r] = -INFINITY;
        }
        float mx = max3(s[0][0], s[0][1], s[0][2]);
        mx = max3(mx, s[0][3], s[1][0]);
        mx = max3(mx, s[1][1], s[1][2]);
        mx = fmaxf(mx, s[1][3]);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx * c);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[kb][r] = __builtin_amdgcn_exp2f(fmaf(s[kb][r], c, -m_new));
        const uint32_t p0 = pack2<T>(s[0][0], s[0][1]), p1 = pack2<T>(s[0][2], s[0][3]);
        const uint32_t p2 = pack2<T>(s[1][0], s[1][1]), p3 = pack2<T>(s[1][2], s[1][3]);
        const i32x4 pb = {(int)p0, (int)p1, (int)p2, (int)p3};
        l_run = fmaf(l_run, alpha, add_pair<T>(p0, add_pair<T>(p1, add_pair<T>(p2, add_pair<T>(p3, 0.f)))));

#pragma unroll
        for (int d = 0; d < DB; ++d) {
            const i32x2 lo = lds_read_tr16(vt, vr_off + 32 * d);
            const i32x2 hi2 = lds_read_tr16(vt, vr_off + 32 * d + 16 * L::VS);
            oacc[d] = mfma16x16x32<T>(i32x4{lo.x, lo.y, hi2.x, hi2.y}, pb, oacc[d] * alpha);
        }
        asm volatile("" ::: "memory");  // next step's writes stay below these reads
        if (it + 1 < nsteps) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                kc[i] = kn[i];
                vc[i] = vn[i];
            }
        }
    }
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);

    // ---- merge the 4 waves in LDS: [wave][row][D] O, then [wave][row] (m, l)
    __syncthreads();  // every wave is done with its tiles
    float* mo = reinterpret_cast<float*>(smem);
    float* mml = mo + DEC_WAVES * DEC_MAXM * D;
#pragma unroll
    for (int d = 0; d < DB; ++d)
        *reinterpret_cast<f32x4*>(mo + (wave * DEC_MAXM + l16) * D + 16 * d + 4 * g) = oacc[d];
    if (g == 0) {
        mml[(wave * DEC_MAXM + l16) * 2] = m_run;
        mml[(wave * DEC_MAXM + l16) * 2 + 1] = l_run;
    }
    __syncthreads();
    constexpr int CH = D / 4;  // float4 chunks per row
    for (int item = tid; item < M * CH; item += 256) {
        const int row = item / CH, cc = item % CH;
        float mw[DEC_WAVES], mt = -1e30f;
#pragma unroll
        for (int w = 0; w < DEC_WAVES; ++w) {
            mw[w] = mml[(w * DEC_MAXM + row) * 2];
            mt = fmaxf(mt, mw[w]);
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        float lt = 0.f;
#pragma unroll
        for (int w = 0; w < DEC_WAVES; ++w) {
            const float wgt = __builtin_amdgcn_exp2f(mw[w] - mt);
            lt = fmaf(mml[(w * DEC_MAXM + row) * 2 + 1], wgt, lt);
            acc += *reinterpret_cast<const f32x4*>(mo + (w * DEC_MAXM + row) * D + 4 * cc) * wgt;
        }
        if (splits == 1) {
            const float inv = lt > 0.f ? vsc / lt : 0.f;
            const int rqi = row / G, rgi = row % G;
            uint16_t* op = o + b * st.ob + (hk * G + rgi) * st.oh + (int64_t)rqi * st.on + 4 * cc;
            *reinterpret_cast<i32x2*>(op) =
                i32x2{(int)pack2<T>(acc[0] * inv, acc[1] * inv), (int)pack2<T>(acc[2] * inv, acc[3] * inv)};
        } else {
            const int64_t prow = ((int64_t)bh * splits + split) * M + row;
            *reinterpret_cast<f32x4*>(part_o + prow * D + 4 * cc) = acc;
            if (cc == 0) part_ml[prow] = float2{mt, lt / vsc};
        }
    }
}

// attn_decode_paged_generic over 1-byte pools: T is q / o's type, every code
// goes through fp8_e4m3_decode (fp8_codec.h).  Correctness path only.
template <typename T>
__global__ __launch_bounds__(64) void attn_decode_paged_generic_fp8(
    const T* __restrict__ q, const uint8_t* __restrict__ k, const uint8_t* __restrict__ v, T* __restrict__ o,
    const int32_t* __restrict__ table, const int32_t* __restrict__ seq_lens, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, int H, int G, int Nq, int D, PagedStrides st, PagedTable tb, float scale,
    int causal, int max_kv, int nk_add) {
    const int lane = threadIdx.x;
    const int qi = blockIdx.x % Nq;
    const int h = (blockIdx.x / Nq) % H;
    const int b = blockIdx.x / (Nq * H);
    const int hk = h / G;
    const int Nk = paged_seq_len(seq_lens[b], nk_add, max_kv);
    const int nvis = min(Nk, causal ? Nk - Nq + qi + 1 : Nk);
    const float sc = scale * fp8_scale_of(k_scale, hk);
    const T* qrow = q + b * st.qb + h * st.qh + (int64_t)qi * st.qn;
    float qv[GEN_DPL], acc[GEN_DPL];
#pragma unroll
    for (int i = 0; i < GEN_DPL; ++i) {
        const int d = lane + 64 * i;
        qv[i] = d < D ? elem<T>::to_f32(qrow[d]) : 0.f;
        acc[i] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int j = 0; j < nvis; ++j) {
        const uint8_t* krow = k + paged_key_offset(table, b, j, hk, tb, st.k);
        const uint8_t* vrow = v + paged_key_offset(table, b, j, hk, tb, st.v);
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < GEN_DPL; ++i) {
            const int d = lane + 64 * i;
            if (d < D) dot = fmaf(qv[i], fp8_e4m3_decode(krow[d]), dot);
        }
        const float s = wave_sum(dot) * sc;
        const float m_new = fmaxf(m, s);
        const float a = __expf(m - m_new), p = __expf(s - m_new);
        l = fmaf(l, a, p);
#pragma unroll
        for (int i = 0; i < GEN_DPL; ++i) {
            const int d = lane + 64 * i;
            if (d < D) acc[i] = fmaf(acc[i], a, p * fp8_e4m3_decode(vrow[d]));
        }
        m = m_new;
    }
    const float inv = l > 0.f ? fp8_scale_of(v_scale, hk) / l : 0.f;  // no visible key: O = 0
    T* orow = o + b * st.ob + h * st.oh + (int64_t)qi * st.on;
#pragma unroll
    for (int i = 0; i < GEN_DPL; ++i) {
        const int d = lane + 64 * i;
        if (d < D) orow[d] = elem<T>::from_f32(acc[i] * inv);
    }
}

// kv_append_paged_kernel that quantises: one thread per 8 elements of a row,
// read as 16 (bf16 / fp16) or 32 (fp32) bytes of the source and stored as one
// 8-byte chunk of codes, code = e4m3(clamp(x * (1 / scale[h]))) (fp8_kv.h).
// Source strides in bytes of the source, pool strides in bytes.
template <typename T>
__global__ __launch_bounds__(256) void kv_append_paged_fp8(
    const char* __restrict__ kn, const char* __restrict__ vn, char* __restrict__ kpool,
    char* __restrict__ vpool, const int32_t* __restrict__ table, const int32_t* __restrict__ seq_lens,
    const float* __restrict__ k_scale, const float* __restrict__ v_scale, int B, int Tn, int Hkv, int cpr,
    AppendStrides st, PagedTable tb) {
    const int64_t total = (int64_t)B * Tn * Hkv * cpr;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = idx % cpr;
    const int h = (idx / cpr) % Hkv;
    const int t = (idx / ((int64_t)cpr * Hkv)) % Tn;
    const int b = idx / ((int64_t)cpr * Hkv * Tn);
    const int64_t pos = (int64_t)seq_lens[b] + t;
    if (pos < 0 || pos >= (int64_t)tb.max_blocks_per_seq * tb.block_size) return;
    constexpr int SRC = 8 * elem<T>::bytes;
    const char* ks = kn + b * st.kb + h * st.kh + (int64_t)t * st.kn + SRC * ch;
    const char* vs = vn + b * st.vb + h * st.vh + (int64_t)t * st.vn + SRC * ch;
    char* kd = kpool + paged_key_offset(table, b, (int)pos, h, tb, st.k) + 8 * ch;
    char* vd = vpool + paged_key_offset(table, b, (int)pos, h, tb, st.v) + 8 * ch;
    *reinterpret_cast<i32x2*>(kd) = fp8_encode8<T>(ks, 1.0f / fp8_scale_of(k_scale, h));
    *reinterpret_cast<i32x2*>(vd) = fp8_encode8<T>(vs, 1.0f / fp8_scale_of(v_scale, h));
}

struct PagedCall {
    const void *q, *k, *v;
    void* o;
    const int32_t *table, *seq_lens;
    int B, H, Hkv, Nq, D, max_kv, causal, nk_add;
    PagedStrides st;
    PagedTable tb;
    float scale;
    hipStream_t stream;
};

template <typename T, int D>
int launch_paged(const PagedCall& a, const PagedPlan& p, float* ws) {
    const int64_t bh = (int64_t)a.B * a.Hkv;
    const int G = a.H / a.Hkv, M = a.Nq * G;
    const float c = a.scale * 1.4426950408889634f;
    float* part_o = ws;
    float2* part_ml = reinterpret_cast<float2*>(ws + bh * p.splits * M * D);
    hipLaunchKernelGGL((attn_decode_paged<T, D>), dim3((unsigned)(bh * p.splits)), dim3(256), 0, a.stream,
                       (const uint16_t*)a.q, (const uint16_t*)a.k, (const uint16_t*)a.v, (uint16_t*)a.o,
                       part_o, part_ml, a.table, a.seq_lens, a.Hkv, G, a.Nq, M, a.st, a.tb, c, a.causal,
                       p.chunk, p.splits, a.max_kv, a.nk_add);
    if (p.splits > 1)
        hipLaunchKernelGGL((attn_decode_paged_combine<T, D>), dim3((unsigned)(bh * M)), dim3(256), 0,
                           a.stream, part_o, part_ml, (uint16_t*)a.o, a.Hkv, G, M, a.st, p.splits);
    return launch_status(p.splits > 1 ? "attn_decode_paged+attn_decode_paged_combine" : "attn_decode_paged");
}

template <typename T>
int launch_paged_generic(const PagedCall& a) {
    const int64_t rows = (int64_t)a.B * a.H * a.Nq;
    hipLaunchKernelGGL((attn_decode_paged_generic<T>), dim3((unsigned)rows), dim3(64), 0, a.stream,
                       (const T*)a.q, (const T*)a.k, (const T*)a.v, (T*)a.o, a.table, a.seq_lens, a.H,
                       a.H / a.Hkv, a.Nq, a.D, a.st, a.tb, a.scale, a.causal, a.max_kv, a.nk_add);
    return launch_status("attn_decode_paged_generic");
}

template <typename T, int D>
int launch_paged_fp8(const PagedCall& a, const Fp8Scales& sc, const PagedPlan& p, float* ws) {
    const int64_t bh = (int64_t)a.B * a.Hkv;
    const int G = a.H / a.Hkv, M = a.Nq * G;
    const float c = a.scale * 1.4426950408889634f;
    float* part_o = ws;
    float2* part_ml = reinterpret_cast<float2*>(ws + bh * p.splits * M * D);
    hipLaunchKernelGGL((attn_decode_paged_fp8<T, D>), dim3((unsigned)(bh * p.splits)), dim3(256), 0, a.stream,
                       (const uint16_t*)a.q, (const uint8_t*)a.k, (const uint8_t*)a.v, (uint16_t*)a.o, part_o,
                       part_ml, a.table, a.seq_lens, sc.k, sc.v, a.Hkv, G, a.Nq, M, a.st, a.tb, c, a.causal,
                       p.chunk, p.splits, a.max_kv, a.nk_add);
    if (p.splits > 1)
        hipLaunchKernelGGL((attn_decode_paged_combine<T, D>), dim3((unsigned)(bh * M)), dim3(256), 0,
                           a.stream, part_o, part_ml, (uint16_t*)a.o, a.Hkv, G, M, a.st, p.splits);
    return launch_status(p.splits > 1 ? "attn_decode_paged_fp8+attn_decode_paged_combine" : "attn_decode_paged_fp8");
}

template <typename T>
int launch_paged_generic_fp8(const PagedCall& a, const Fp8Scales& sc) {
    const int64_t rows = (int64_t)a.B * a.H * a.Nq;
    hipLaunchKernelGGL((attn_decode_paged_generic_fp8<T>), dim3((unsigned)rows), dim3(64), 0, a.stream,
                       (const T*)a.q, (const uint8_t*)a.k, (const uint8_t*)a.v, (T*)a.o, a.table, a.seq_lens, sc.k,
                       sc.v, a.H, a.H / a.Hkv, a.Nq, a.D, a.st, a.tb, a.scale, a.causal, a.max_kv, a.nk_add);
    return launch_status("attn_decode_paged_generic_fp8");
}

template <typename T>
int launch_append_fp8(const char* kn, const char* vn, char* kpool, char* vpool, const int32_t* table,
                      const int32_t* seq_lens, const Fp8Scales& sc, int B, int Tn, int Hkv, int cpr,
                      const AppendStrides& st, const PagedTable& tb, hipStream_t stream) {
    const int64_t total = (int64_t)B * Tn * Hkv * cpr;
    hipLaunchKernelGGL(kv_append_paged_fp8<T>, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, stream, kn, vn,
                       kpool, vpool, table, seq_lens, sc.k, sc.v, B, Tn, Hkv, cpr, st, tb);
    return launch_status("kv_append_paged_fp8");
}

}  // namespace
}  // namespace pli

extern "C" size_t pli_attn_decode_paged_workspace_size(int batch, int heads, int kv_heads, int n_q,
                                                       int max_kv, int head_dim) {
    using namespace pli;
    if (batch <= 0 || heads <= 0 || kv_heads <= 0 || heads % kv_heads || n_q <= 0 || max_kv <= 0 ||
        head_dim <= 0)
        return 0;
    const int64_t M = (int64_t)n_q * (heads / kv_heads);
    if (M > DEC_MAXM || !(head_dim == 64 || head_dim == 128)) return 0;
    return (size_t)plan_paged(batch, kv_heads, max_kv, M, head_dim).workspace_bytes;
}

extern "C" int pli_attn_decode_paged(const void* q, const void* k_pool, const void* v_pool, void* o,
                                     const int32_t* block_table, const int32_t* seq_lens, int batch,
                                     int heads, int kv_heads, int n_q, int head_dim, int block_size,
                                     int num_blocks, int max_blocks_per_seq, int max_kv,
                                     const int64_t* strides, float scale, int causal, int n_kv_add,
                                     void* workspace, size_t workspace_bytes, int dtype,
                                     void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(batch >= 0 && heads > 0 && kv_heads > 0 && n_q >= 0 && head_dim > 0 &&
                    num_blocks >= 0 && max_blocks_per_seq >= 0 && max_kv >= 0,
                "pli_attn_decode_paged: bad shape B=%d H=%d Hkv=%d Nq=%d D=%d blocks=%d "
                "max_blocks_per_seq=%d max_kv=%d",
                batch, heads, kv_heads, n_q, head_dim, num_blocks, max_blocks_per_seq, max_kv);
    PLI_REQUIRE(heads % kv_heads == 0,
                "pli_attn_decode_paged: heads %d not a multiple of kv_heads %d", heads, kv_heads);
    PLI_REQUIRE(dtype == PLI_F32 || dtype == PLI_F16 || dtype == PLI_BF16,
                "pli_attn_decode_paged: bad dtype %d", dtype);
    PLI_REQUIRE(std::isfinite(scale), "pli_attn_decode_paged: non-finite scale");
    PLI_REQUIRE(block_size > 0, "pli_attn_decode_paged: block_size %d must be positive", block_size);
    PLI_REQUIRE((int64_t)max_kv <= (int64_t)max_blocks_per_seq * block_size,
                "pli_attn_decode_paged: max_kv %d past the table row (%d blocks of %d tokens)", max_kv,
                max_blocks_per_seq, block_size);
    PLI_REQUIRE((int64_t)max_blocks_per_seq * block_size < (1ll << 31),
                "pli_attn_decode_paged: a table row of %d blocks x %d tokens passes 2^31 keys",
                max_blocks_per_seq, block_size);
    // no output rows: the (possibly NULL, pli.h) operands are not read
    if (batch == 0 || n_q == 0) return PLI_OK;
    PLI_REQUIRE(q && o && k_pool && v_pool && block_table && seq_lens && strides,
                "pli_attn_decode_paged: null pointer");
    PLI_REQUIRE(num_blocks > 0 && max_blocks_per_seq > 0,
                "pli_attn_decode_paged: empty pool or table (blocks=%d max_blocks_per_seq=%d)",
                num_blocks, max_blocks_per_seq);
    PagedCall a;
    a.q = q, a.k = k_pool, a.v = v_pool, a.o = o, a.table = block_table, a.seq_lens = seq_lens;
    a.B = batch, a.H = heads, a.Hkv = kv_heads, a.Nq = n_q, a.D = head_dim, a.max_kv = max_kv;
    a.causal = causal != 0, a.nk_add = n_kv_add, a.scale = scale, a.stream = (hipStream_t)stream;
    // strides[12] = {q_b, q_h, q_n, k_page, k_token, k_head, v_page, v_token, v_head, o_b, o_h, o_n}
    a.st = PagedStrides{strides[0], strides[1], strides[2], strides[9], strides[10], strides[11],
                        PagedPool{strides[3], strides[4], strides[5]},
                        PagedPool{strides[6], strides[7], strides[8]}};
    a.tb = paged_table(block_size, num_blocks, max_blocks_per_seq);
    const int64_t M = (int64_t)n_q * (heads / kv_heads);
    const bool fast = paged_fast_path(dtype, head_dim, M, block_size, scale, strides,
                                      aligned16(q) && aligned16(k_pool) && aligned16(v_pool) && aligned16(o));
    if (!fast) {
        PLI_REQUIRE(head_dim <= GEN_MAXD, "pli_attn_decode_paged: head_dim %d > %d", head_dim, GEN_MAXD);
        PLI_REQUIRE((int64_t)batch * heads * n_q < (1ll << 31), "pli_attn_decode_paged: grid too large");
        if (dtype == PLI_F32) return launch_paged_generic<float>(a);
        return dtype == PLI_BF16 ? launch_paged_generic<bf16_t>(a) : launch_paged_generic<f16_t>(a);
    }
    const PagedPlan p = plan_paged(batch, kv_heads, max_kv, M, head_dim);
    const size_t need = (size_t)p.workspace_bytes;
    PLI_REQUIRE(workspace_bytes >= need && (need == 0 || workspace != nullptr),
                "pli_attn_decode_paged: workspace of %zu bytes needed, %zu given", need, workspace_bytes);
    PLI_REQUIRE(need == 0 || aligned16(workspace), "pli_attn_decode_paged: workspace must be 16-byte aligned");
    PLI_REQUIRE((int64_t)batch * kv_heads * p.splits < (1ll << 31), "pli_attn_decode_paged: grid too large");
    float* ws = (float*)workspace;
    if (dtype == PLI_BF16)
        return head_dim == 128 ? launch_paged<bf16_t, 128>(a, p, ws) : launch_paged<bf16_t, 64>(a, p, ws);
    return head_dim == 128 ? launch_paged<f16_t, 128>(a, p, ws) : launch_paged<f16_t, 64>(a, p, ws);
}

extern "C" int pli_kv_append_paged(const void* k_new, const void* v_new, void* k_pool, void* v_pool,
                                   const int32_t* block_table, const int32_t* seq_lens, int batch,
                                   int n_new, int kv_heads, int head_dim, int block_size,
                                   int num_blocks, int max_blocks_per_seq, const int64_t* strides,
                                   int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(batch >= 0 && n_new >= 0 && kv_heads > 0 && head_dim > 0 && num_blocks >= 0 &&
                    max_blocks_per_seq >= 0,
                "pli_kv_append_paged: bad shape B=%d T=%d Hkv=%d D=%d blocks=%d max_blocks_per_seq=%d",
                batch, n_new, kv_heads, head_dim, num_blocks, max_blocks_per_seq);
    PLI_REQUIRE(dtype == PLI_F32 || dtype == PLI_F16 || dtype == PLI_BF16,
                "pli_kv_append_paged: bad dtype %d", dtype);
    PLI_REQUIRE(block_size > 0, "pli_kv_append_paged: block_size %d must be positive", block_size);
    PLI_REQUIRE((int64_t)max_blocks_per_seq * block_size < (1ll << 31),
                "pli_kv_append_paged: a table row of %d blocks x %d tokens passes 2^31 keys",
                max_blocks_per_seq, block_size);
    // nothing to append: the (possibly NULL, pli.h) operands are not read
    if (batch == 0 || n_new == 0) return PLI_OK;
    PLI_REQUIRE(k_new && v_new && k_pool && v_pool && block_table && seq_lens && strides,
                "pli_kv_append_paged: null pointer");
    PLI_REQUIRE(num_blocks > 0 && max_blocks_per_seq > 0,
                "pli_kv_append_paged: empty pool or table (blocks=%d max_blocks_per_seq=%d)", num_blocks,
                max_blocks_per_seq);
    const int es = dtype == PLI_F32 ? 4 : 2, per16 = 16 / es;
    PLI_REQUIRE(head_dim % per16 == 0 && aligned16(k_new) && aligned16(v_new) && aligned16(k_pool) &&
                    aligned16(v_pool),
                "pli_kv_append_paged: 16-byte rows (head_dim %% %d) and 16-byte aligned operands required",
                per16);
    for (int i = 0; i < 12; ++i)
        PLI_REQUIRE(strides[i] % per16 == 0, "pli_kv_append_paged: stride %d not a multiple of %d", i, per16);
    const int cpr = head_dim / per16;
    const int64_t total = (int64_t)batch * n_new * kv_heads * cpr;
    PLI_REQUIRE(cdiv64(total, 256) < (1ll << 31), "pli_kv_append_paged: grid too large");
    // strides[12] = {kn_b, kn_h, kn_n, k_page, k_token, k_head, v_page, v_token, v_head, vn_b, vn_h, vn_n}
    const AppendStrides st{strides[0] * es, strides[1] * es, strides[2] * es,
                           strides[9] * es, strides[10] * es, strides[11] * es,
                           PagedPool{strides[3] * es, strides[4] * es, strides[5] * es},
                           PagedPool{strides[6] * es, strides[7] * es, strides[8] * es}};
    hipLaunchKernelGGL(kv_append_paged_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0,
                       (hipStream_t)stream, (const char*)k_new, (const char*)v_new, (char*)k_pool,
                       (char*)v_pool, block_table, seq_lens, batch, n_new, kv_heads, cpr, st,
                       paged_table(block_size, num_blocks, max_blocks_per_seq));
    return launch_status("kv_append_paged_kernel");
}

extern "C" int pli_attn_decode_paged_fp8(const void* q, const void* k_pool, const void* v_pool, void* o,
                                         const int32_t* block_table, const int32_t* seq_lens,
                                         const float* k_scale, const float* v_scale, int batch, int heads,
                                         int kv_heads, int n_q, int head_dim, int block_size, int num_blocks,
                                         int max_blocks_per_seq, int max_kv, const int64_t* strides,
                                         float scale, int causal, int n_kv_add, void* workspace,
                                         size_t workspace_bytes, int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(batch >= 0 && heads > 0 && kv_heads > 0 && n_q >= 0 && head_dim > 0 &&
                    num_blocks >= 0 && max_blocks_per_seq >= 0 && max_kv >= 0,
                "pli_attn_decode_paged_fp8: bad shape B=%d H=%d Hkv=%d Nq=%d D=%d blocks=%d "
                "max_blocks_per_seq=%d max_kv=%d",
                batch, heads, kv_heads, n_q, head_dim, num_blocks, max_blocks_per_seq, max_kv);
    PLI_REQUIRE(heads % kv_heads == 0,
                "pli_attn_decode_paged_fp8: heads %d not a multiple of kv_heads %d", heads, kv_heads);
    PLI_REQUIRE(dtype == PLI_F32 || dtype == PLI_F16 || dtype == PLI_BF16,
                "pli_attn_decode_paged_fp8: bad dtype %d", dtype);
    PLI_REQUIRE(std::isfinite(scale), "pli_attn_decode_paged_fp8: non-finite scale");
    PLI_REQUIRE(block_size > 0, "pli_attn_decode_paged_fp8: block_size %d must be positive", block_size);
    PLI_REQUIRE((int64_t)max_kv <= (int64_t)max_blocks_per_seq * block_size,
                "pli_attn_decode_paged_fp8: max_kv %d past the table row (%d blocks of %d tokens)", max_kv,
                max_blocks_per_seq, block_size);
    PLI_REQUIRE((int64_t)max_blocks_per_seq * block_size < (1ll << 31),
                "pli_attn_decode_paged_fp8: a table row of %d blocks x %d tokens passes 2^31 keys",
                max_blocks_per_seq, block_size);
    // no output rows: the (possibly NULL, pli.h) operands are not read
    if (batch == 0 || n_q == 0) return PLI_OK;
    PLI_REQUIRE(q && o && k_pool && v_pool && block_table && seq_lens && strides,
                "pli_attn_decode_paged_fp8: null pointer");
    PLI_REQUIRE(num_blocks > 0 && max_blocks_per_seq > 0,
                "pli_attn_decode_paged_fp8: empty pool or table (blocks=%d max_blocks_per_seq=%d)",
                num_blocks, max_blocks_per_seq);
    PagedCall a;
    a.q = q, a.k = k_pool, a.v = v_pool, a.o = o, a.table = block_table, a.seq_lens = seq_lens;
    a.B = batch, a.H = heads, a.Hkv = kv_heads, a.Nq = n_q, a.D = head_dim, a.max_kv = max_kv;
    a.causal = causal != 0, a.nk_add = n_kv_add, a.scale = scale, a.stream = (hipStream_t)stream;
    // strides[12] as for pli_attn_decode_paged; the pool strides count 1-byte elements
    a.st = PagedStrides{strides[0], strides[1], strides[2], strides[9], strides[10], strides[11],
                        PagedPool{strides[3], strides[4], strides[5]},
                        PagedPool{strides[6], strides[7], strides[8]}};
    a.tb = paged_table(block_size, num_blocks, max_blocks_per_seq);
    const Fp8Scales sc{k_scale, v_scale};
    const int64_t M = (int64_t)n_q * (heads / kv_heads);
    const bool fast = paged_fast_path_fp8(dtype, head_dim, M, block_size, scale, strides,
                                          aligned16(q) && aligned16(k_pool) && aligned16(v_pool) && aligned16(o));
    if (!fast) {
        PLI_REQUIRE(head_dim <= GEN_MAXD, "pli_attn_decode_paged_fp8: head_dim %d > %d", head_dim, GEN_MAXD);
        PLI_REQUIRE((int64_t)batch * heads * n_q < (1ll << 31), "pli_attn_decode_paged_fp8: grid too large");
        if (dtype == PLI_F32) return launch_paged_generic_fp8<float>(a, sc);
        return dtype == PLI_BF16 ? launch_paged_generic_fp8<bf16_t>(a, sc) : launch_paged_generic_fp8<f16_t>(a, sc);
    }
    const PagedPlan p = plan_paged(batch, kv_heads, max_kv, M, head_dim);
    const size_t need = (size_t)p.workspace_bytes;
    PLI_REQUIRE(workspace_bytes >= need && (need == 0 || workspace != nullptr),
                "pli_attn_decode_paged_fp8: workspace of %zu bytes needed, %zu given", need, workspace_bytes);
    PLI_REQUIRE(need == 0 || aligned16(workspace), "pli_attn_decode_paged_fp8: workspace must be 16-byte aligned");
    PLI_REQUIRE((int64_t)batch * kv_heads * p.splits < (1ll << 31), "pli_attn_decode_paged_fp8: grid too large");
    float* ws = (float*)workspace;
    if (dtype == PLI_BF16)
        return head_dim == 128 ? launch_paged_fp8<bf16_t, 128>(a, sc, p, ws) : launch_paged_fp8<bf16_t, 64>(a, sc, p, ws);
    return head_dim == 128 ? launch_paged_fp8<f16_t, 128>(a, sc, p, ws) : launch_paged_fp8<f16_t, 64>(a, sc, p, ws);
}

extern "C" int pli_kv_append_paged_fp8(const void* k_new, const void* v_new, void* k_pool, void* v_pool,
                                       const int32_t* block_table, const int32_t* seq_lens,
                                       const float* k_scale, const float* v_scale, int batch, int n_new,
                                       int kv_heads, int head_dim, int block_size, int num_blocks,
                                       int max_blocks_per_seq, const int64_t* strides, int dtype,
                                       void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(batch >= 0 && n_new >= 0 && kv_heads > 0 && head_dim > 0 && num_blocks >= 0 &&
                    max_blocks_per_seq >= 0,
                "pli_kv_append_paged_fp8: bad shape B=%d T=%d Hkv=%d D=%d blocks=%d max_blocks_per_seq=%d",
                batch, n_new, kv_heads, head_dim, num_blocks, max_blocks_per_seq);
    PLI_REQUIRE(dtype == PLI_F32 || dtype == PLI_F16 || dtype == PLI_BF16,
                "pli_kv_append_paged_fp8: bad dtype %d", dtype);
    PLI_REQUIRE(block_size > 0, "pli_kv_append_paged_fp8: block_size %d must be positive", block_size);
    PLI_REQUIRE((int64_t)max_blocks_per_seq * block_size < (1ll << 31),
                "pli_kv_append_paged_fp8: a table row of %d blocks x %d tokens passes 2^31 keys",
                max_blocks_per_seq, block_size);
    // nothing to append: the (possibly NULL, pli.h) operands are not read
    if (batch == 0 || n_new == 0) return PLI_OK;
    PLI_REQUIRE(k_new && v_new && k_pool && v_pool && block_table && seq_lens && strides,
                "pli_kv_append_paged_fp8: null pointer");
    PLI_REQUIRE(num_blocks > 0 && max_blocks_per_seq > 0,
                "pli_kv_append_paged_fp8: empty pool or table (blocks=%d max_blocks_per_seq=%d)", num_blocks,
                max_blocks_per_seq);
    PLI_REQUIRE(head_dim % 8 == 0 && aligned16(k_new) && aligned16(v_new) && aligned16(k_pool) && aligned16(v_pool),
                "pli_kv_append_paged_fp8: rows of whole 8-element chunks (head_dim %% 8) and 16-byte aligned "
                "operands required");
    for (int i = 0; i < 12; ++i)
        PLI_REQUIRE(strides[i] % 8 == 0, "pli_kv_append_paged_fp8: stride %d not a multiple of 8", i);
    const int es = dtype == PLI_F32 ? 4 : 2;
    const int cpr = head_dim / 8;
    const int64_t total = (int64_t)batch * n_new * kv_heads * cpr;
    PLI_REQUIRE(cdiv64(total, 256) < (1ll << 31), "pli_kv_append_paged_fp8: grid too large");
    // strides[12] as for pli_kv_append_paged: the source's in its elements, the pools' in bytes
    const AppendStrides st{strides[0] * es, strides[1] * es, strides[2] * es,
                           strides[9] * es, strides[10] * es, strides[11] * es,
                           PagedPool{strides[3], strides[4], strides[5]},
                           PagedPool{strides[6], strides[7], strides[8]}};
    const PagedTable tb = paged_table(block_size, num_blocks, max_blocks_per_seq);
    const Fp8Scales sc{k_scale, v_scale};
    const char *kn = (const char*)k_new, *vn = (const char*)v_new;
    char *kp = (char*)k_pool, *vp = (char*)v_pool;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PLI_F32)
        return launch_append_fp8<float>(kn, vn, kp, vp, block_table, seq_lens, sc, batch, n_new, kv_heads, cpr, st, tb, s);
    if (dtype == PLI_BF16)
        return launch_append_fp8<bf16_t>(kn, vn, kp, vp, block_table, seq_lens, sc, batch, n_new, kv_heads, cpr, st, tb, s);
    return launch_append_fp8<f16_t>(kn, vn, kp, vp, block_table, seq_lens, sc, batch, n_new, kv_heads, cpr, st, tb, s);
}
