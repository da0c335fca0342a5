// Decode attention over an MXFP4 paged KV pool, and the quantising appends
// that feed it, for gfx950.
//
// Format (pli.h): a code pool holds e2m1 codes, two per byte, head_dim / 2
// bytes per (token, kv head); a scale pool of its own holds one E8M0 byte per
// 32 elements, head_dim / 32 bytes per (token, kv head);
// value = decode_e2m1(code) * 2^(exp - 127).  68 bytes per row at head_dim 128
// against 128 for the fp8 pool and 256 for a 16-bit one.
//
// attn_decode_paged_mxfp4<T, D> keeps the decomposition and the arithmetic of
// attn_decode_paged<T, D> (paged_attn.hip): one workgroup = (batch, chunk, kv
// head), 4 waves of 32-key steps, wave-private LDS tiles, S^T = K . Q^T and
// O^T += V^T . P^T by v_mfma_f32_16x16x32, fp32 statistics, waves merged in
// LDS, fp32 partials and attn_decode_paged_combine (unchanged) when splits > 1.
// The steps, their order and the merge are the 16-bit kernel's, and the
// widening is exact, so the output is bitwise attn_decode_paged over a T pool
// of the dequantised values.  What is its own is the load stage:
//   * a lane's 16-byte non-temporal load is exactly one MX block: 32 codes
//     under one scale byte.  A 32-key step of D = 128 is 2 K + 2 V loads per
//     lane (D = 64: 1 + 1), a quarter of the 16-bit kernel's, and D / 32 lanes
//     own a row.
//   * the lane fetches its block's scale byte itself (global_load_ubyte at the
//     row's scale address + its block index), in the same stage as the codes.
//     The D / 32 lanes of a row hit one dword, so the bytes cost no extra
//     memory transaction, and nothing crosses lanes on the way to the
//     conversion.
//   * the loads run TWO steps ahead of their use (three register stages: the
//     step being converted, and two in flight), the table entries three steps
//     ahead.  A stage is 4 dwords of codes and 1 of scale per block, so three
//     of them are smaller than the 16-bit kernel's two; the occupancy is set by
//     LDS (two workgroups per CU) either way, and with a single step in flight
//     a CU would have only 32 KiB of K / V on the wire.
//   * between the load and the LDS write the lane widens its 32 codes with
//     sixteen v_cvt_scalef32_pk_{bf16,f16}_fp4, the block scale folded in as
//     the float 2^(s - 127) (exact inside the read contract), and writes 64
//     bytes of the row-major padded image the 16-bit MFMA loop reads.
//   * every load runs at a clamped address (key <= n_kv - 1, block index inside
//     the table row, page inside the pool, for the code and the scale pools
//     alike) and the scores are masked afterwards; no load sits behind a
//     runtime select.
//   * a 0xFF scale byte in a key's K or V block turns the first pair of the K
//     block into NaN and widens both blocks at scale 1: the key's score is NaN
//     for exactly the rows it is not masked for, and so is every element of
//     those rows; rows that do not see the key meet finite values at P = 0.
// attn_decode_paged_generic_mxfp4 covers every other case (fp32 q, any
// head_dim % 32 == 0 up to 256, any block size and group size) through
// fp4_codec.h: one wave per (batch, head, query row), a correctness path.
// kv_append_paged_mxfp4 / kv_append_varlen_paged_mxfp4 quantise on the way in:
// four lanes per block, each reads 8 source elements (16 or 32 bytes), the
// block's amax and NaN flag cross the four lanes by two exchanges, each lane
// stores one dword of eight codes and the first stores the scale byte.
#include <cmath>

#include "mxfp4_kv.h"
#include "paged_combine.h"
#include "paged_plan.h"
#include "pli_common.h"
#include "varlen_plan.h"

namespace pli {
namespace {

inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// q / o {batch, head, row} in elements; code pools and scale pools {page, token, head} in bytes
struct Kv4Strides {
    int64_t qb, qh, qn, ob, oh, on;
    PagedPool k, v, ke, ve;
};

// the LDS image of attn_decode_paged<T, D>
template <int D> struct Kv4Layout {
    static constexpr int KS = 2 * D + 16;             // K row stride in LDS (bytes)
    static constexpr int VS = 2 * D + 32;             // V row stride in LDS (bytes)
    static constexpr int KBYTES = DEC_STEP * KS;
    static constexpr int WAVE_BYTES = KBYTES + DEC_STEP * VS;  // per-wave K + V tile
    static constexpr int MERGE_BYTES = DEC_WAVES * (DEC_MAXM * D + 2 * DEC_MAXM) * 4;
    static constexpr int LDS = WAVE_BYTES * DEC_WAVES > MERGE_BYTES ? WAVE_BYTES * DEC_WAVES
                                                                     : MERGE_BYTES;
};

// one step of a lane in registers: NI blocks of K and of V with their scale bytes
template <int NI> struct Kv4Stage {
    i32x4 k[NI], v[NI];
    uint32_t ks[NI], vs[NI];
};

template <typename T, int D>
__global__ __launch_bounds__(256, 2) void attn_decode_paged_mxfp4(
    const uint16_t* __restrict__ q, const uint8_t* __restrict__ k, const uint8_t* __restrict__ v,
    const uint8_t* __restrict__ ke, const uint8_t* __restrict__ ve, uint16_t* __restrict__ o,
    float* __restrict__ part_o, float2* __restrict__ part_ml, const int32_t* __restrict__ table,
    const int32_t* __restrict__ seq_lens, int Hkv, int G, int Nq, int M, Kv4Strides st, PagedTable tb, float c,
    int causal, int chunk, int splits, int max_kv, int nk_add) {
    using L = Kv4Layout<D>;
    constexpr int KSTEPS = D / 32;  // 32-d k-steps of K.Q^T
    constexpr int DB = D / 16;      // 16-d blocks of O
    __shared__ __attribute__((aligned(16))) char smem[L::LDS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, g = lane >> 4;
    // block order: (b, split, hk), the kv head innermost (attn_decode_paged)
    const int hk = blockIdx.x % Hkv;
    const int split = (blockIdx.x / Hkv) % splits;
    const int b = blockIdx.x / (Hkv * splits);
    const int bh = b * Hkv + hk;
    const int Nk = paged_seq_len(seq_lens[b], nk_add, max_kv);

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

    // row-major loads: in instruction i the lane loads block rch (32 codes, 16
    // bytes) of row i*RPI + rrow of the step, and that block's scale byte
    constexpr int CPR = D / kKv4Block, RPI = 64 / CPR, NI = DEC_STEP / RPI;
    using Stage = Kv4Stage<NI>;
    const int rrow = lane / CPR, rch = lane % CPR;
    const uint8_t* kp = k + 16 * rch;
    const uint8_t* vp = v + 16 * rch;
    auto ld = [](const uint8_t* p) {
        return __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(p));
    };
    // the raw table entries of the two pages a step starting at key0 can touch
    auto pages = [&](int key0, int& e0, int& e1) {
        e0 = table[paged_table_index(b, paged_block_pow2(key0, tb), tb)];
        e1 = table[paged_table_index(b, paged_block_pow2(key0 + 16, tb), tb)];
    };
    auto load_step = [&](int key0, int e0, int e1, Stage& s) {
        const int blk0 = paged_block_pow2(key0, tb);
        const int p0 = paged_clamp_page(e0, tb), p1 = paged_clamp_page(e1, tb);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int key = min(key0 + i * RPI + rrow, Nk - 1);
            const int page = paged_block_pow2(key, tb) == blk0 ? p0 : p1;
            s.k[i] = ld(kp + paged_offset_pow2(page, key, hk, tb, st.k));
            s.v[i] = ld(vp + paged_offset_pow2(page, key, hk, tb, st.v));
            s.ks[i] = ke[paged_exp_offset_pow2(page, key, hk, rch, tb, st.ke)];
            s.vs[i] = ve[paged_exp_offset_pow2(page, key, hk, rch, tb, st.ve)];
        }
    };

    char* kt = smem + wave * L::WAVE_BYTES;
    char* vt = kt + L::KBYTES;
    const int vw = rrow * L::VS + rch * 64;                     // 32 T = 64 bytes per lane
    const int kw = rrow * L::KS + rch * 64;
    const int kr_off = l16 * L::KS + g * 16;                    // K fragment read
    const int qq = l16 >> 2, pp = lane & 3;
    const int vr_off = (4 * g + qq) * L::VS + 8 * pp;           // tr read: key 4g+qq, col 4pp

    f32x4 oacc[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d) oacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;

    // cur: the step being converted; nx: the step after it, in flight; pn0 /
    // pn1: the table entries of the step after that, whose loads go out next
    Stage cur{}, nx{};
    int pn0 = 0, pn1 = 0;
    if (nsteps > 0) {
        int a0, a1, b0, b1;
        pages(w0, a0, a1);
        pages(w0 + DEC_STEP, b0, b1);
        pages(w0 + 2 * DEC_STEP, pn0, pn1);
        load_step(w0, a0, a1, cur);
        if (nsteps > 1) load_step(w0 + DEC_STEP, b0, b1, nx);
    }
    for (int it = 0; it < nsteps; ++it) {
        const int key0 = w0 + it * DEC_STEP;
        Stage n2{};
        if (it + 2 < nsteps) {
            // step t+3's table entries first (consumed a whole step later),
            // then step t+2's blocks with the entries fetched a step ago
            int f0, f1;
            pages(key0 + 3 * DEC_STEP, f0, f1);
            load_step(key0 + 2 * DEC_STEP, pn0, pn1, n2);
            pn0 = f0, pn1 = f1;
        }

        // the conversion point: codes -> T at the block scale, then the row-major padded image
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const bool bad = cur.ks[i] == 0xffu || cur.vs[i] == 0xffu;
            i32x4 w[4];
            kv4_widen32<T>(cur.v[i], kv4_scale_f32(cur.vs[i], bad), w);
#pragma unroll
            for (int h = 0; h < 4; ++h) lds_write_b128(vt, vw + i * RPI * L::VS + 16 * h, w[h]);
            kv4_widen32<T>(cur.k[i], kv4_scale_f32(cur.ks[i], bad), w);
            w[0].x = kv4_nan_pair<T>(bad, w[0].x);
#pragma unroll
            for (int h = 0; h < 4; ++h) lds_write_b128(kt, kw + i * RPI * L::KS + 16 * h, w[h]);
        }
        // the tile is wave-private and a wave's LDS operations execute in
        // order; the fence only stops the compiler moving the transposed reads
        // above these writes
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
        cur = nx;
        nx = n2;
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
            // a row that saw no key has l = 0 and is written as 0; a NaN row
            // (l is NaN, the comparison false) stays NaN through acc * 0
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

// Any q type, head_dim % 32 == 0 up to 256, any block size, any group size: one
// wave per (batch, head, query row); lane l owns dims l, l + 64, ...; keys in
// order, fp32 online softmax; every code and scale byte goes through
// fp4_codec.h.  A 0xFF byte in a seen key's V row is carried into the key's
// score, as the fast kernel does, so the whole row is NaN.  Correctness path only.
constexpr int GEN4_MAXD = 256, GEN4_DPL = GEN4_MAXD / 64;
template <typename T>
__global__ __launch_bounds__(64) void attn_decode_paged_generic_mxfp4(
    const T* __restrict__ q, const uint8_t* __restrict__ k, const uint8_t* __restrict__ v,
    const uint8_t* __restrict__ ke, const uint8_t* __restrict__ ve, T* __restrict__ o,
    const int32_t* __restrict__ table, const int32_t* __restrict__ seq_lens, int H, int G, int Nq, int D,
    Kv4Strides st, PagedTable tb, float scale, int causal, int max_kv, int nk_add) {
    const int lane = threadIdx.x;
    const int qi = blockIdx.x % Nq;
    const int h = (blockIdx.x / Nq) % H;
    const int b = blockIdx.x / (Nq * H);
    const int hk = h / G;
    const int Nk = paged_seq_len(seq_lens[b], nk_add, max_kv);
    const int nvis = min(Nk, causal ? Nk - Nq + qi + 1 : Nk);
    const T* qrow = q + b * st.qb + h * st.qh + (int64_t)qi * st.qn;
    float qv[GEN4_DPL], acc[GEN4_DPL];
#pragma unroll
    for (int i = 0; i < GEN4_DPL; ++i) {
        const int d = lane + 64 * i;
        qv[i] = d < D ? elem<T>::to_f32(qrow[d]) : 0.f;
        acc[i] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int j = 0; j < nvis; ++j) {
        const uint8_t* krow = k + paged_key_offset(table, b, j, hk, tb, st.k);
        const uint8_t* vrow = v + paged_key_offset(table, b, j, hk, tb, st.v);
        const uint8_t* kexp = ke + paged_exp_key_offset(table, b, j, hk, 0, tb, st.ke);
        const uint8_t* vexp = ve + paged_exp_key_offset(table, b, j, hk, 0, tb, st.ve);
        float dot = 0.f, vv[GEN4_DPL];
#pragma unroll
        for (int i = 0; i < GEN4_DPL; ++i) {
            const int d = lane + 64 * i;
            vv[i] = 0.f;
            if (d < D) {
                dot = fmaf(qv[i], fp4_e2m1_decode(fp4_nibble(krow[d / 2], d)) * e8m0_decode(kexp[d / kKv4Block]), dot);
                vv[i] = fp4_e2m1_decode(fp4_nibble(vrow[d / 2], d)) * e8m0_decode(vexp[d / kKv4Block]);
                if (vv[i] != vv[i]) dot = vv[i];
            }
        }
        const float s = wave_sum(dot) * scale;
        const float m_new = fmaxf(m, s);
        const float a = __expf(m - m_new), p = __expf(s - m_new);
        l = fmaf(l, a, p);
#pragma unroll
        for (int i = 0; i < GEN4_DPL; ++i) acc[i] = fmaf(acc[i], a, p * vv[i]);
        m = m_new;
    }
    const float inv = l > 0.f ? 1.f / l : 0.f;  // no visible key: O = 0; a NaN row stays NaN
    T* orow = o + b * st.ob + h * st.oh + (int64_t)qi * st.on;
#pragma unroll
    for (int i = 0; i < GEN4_DPL; ++i) {
        const int d = lane + 64 * i;
        if (d < D) orow[d] = elem<T>::from_f32(acc[i] * inv);
    }
}

// ---- appends --------------------------------------------------------------------
// One thread per 8 elements of a (token, kv head) row of K and of V: chunk ch
// is quarter ch & 3 of block ch >> 2, and the four threads of a block are
// adjacent lanes that are live or not together (cpr % 4 == 0).  Source strides
// in bytes of the source, pool strides in bytes.
struct Kv4AppendStrides {
    int64_t kb, kh, kn, vb, vh, vn;  // the new tensors: batch (or packed token), head, token
    PagedPool k, v, ke, ve;
};
struct Kv4Pools {
    char *k, *v;
    uint8_t *ke, *ve;
};
template <typename T>
__device__ __forceinline__ void kv4_store_chunk(const char* ks, const char* vs, const Kv4Pools& pool,
                                                const int32_t* __restrict__ table, int b, int pos, int h, int ch,
                                                const Kv4AppendStrides& st, const PagedTable& tb) {
    float x[8];
    uint32_t byte;
    kv4_read8<T>(ks, x);
    const uint32_t kc = kv4_encode8(x, byte);
    *reinterpret_cast<uint32_t*>(pool.k + paged_key_offset(table, b, pos, h, tb, st.k) + 4 * ch) = kc;
    if ((ch & 3) == 0) pool.ke[paged_exp_key_offset(table, b, pos, h, ch >> 2, tb, st.ke)] = (uint8_t)byte;
    kv4_read8<T>(vs, x);
    const uint32_t vc = kv4_encode8(x, byte);
    *reinterpret_cast<uint32_t*>(pool.v + paged_key_offset(table, b, pos, h, tb, st.v) + 4 * ch) = vc;
    if ((ch & 3) == 0) pool.ve[paged_exp_key_offset(table, b, pos, h, ch >> 2, tb, st.ve)] = (uint8_t)byte;
}

// token t of sequence b -> logical position seq_lens[b] + t (kv_append_paged_kernel's rule)
template <typename T>
__global__ __launch_bounds__(256) void kv_append_paged_mxfp4(
    const char* __restrict__ kn, const char* __restrict__ vn, Kv4Pools pool, const int32_t* __restrict__ table,
    const int32_t* __restrict__ seq_lens, int B, int Tn, int Hkv, int cpr, Kv4AppendStrides st, PagedTable tb) {
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
    kv4_store_chunk<T>(kn + b * st.kb + h * st.kh + (int64_t)t * st.kn + SRC * ch,
                       vn + b * st.vb + h * st.vh + (int64_t)t * st.vn + SRC * ch, pool, table, b, (int)pos, h, ch, st,
                       tb);
}

// packed row cu[b] + i -> logical position seq_lens[b] - q_len(b) + i (varlen_plan.h); st.kb / st.vb are the
// packed-token strides
template <typename T>
__global__ __launch_bounds__(256) void kv_append_varlen_paged_mxfp4(
    const char* __restrict__ kn, const char* __restrict__ vn, Kv4Pools pool, const int32_t* __restrict__ cu,
    const int32_t* __restrict__ table, const int32_t* __restrict__ seq_lens, int batch, int max_tokens, int Hkv,
    int cpr, Kv4AppendStrides st, PagedTable tb) {
    const int64_t total = (int64_t)max_tokens * Hkv * cpr;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = idx % cpr;
    const int h = (idx / cpr) % Hkv;
    const int t = (int)(idx / ((int64_t)cpr * Hkv));
    if (t >= varlen_tokens_live(cu[batch], max_tokens)) return;
    const int b = varlen_owner(cu, batch, t);
    if (b < 0) return;
    const int64_t pos = varlen_append_pos(seq_lens[b], varlen_q_len(cu[b], cu[b + 1]), t - cu[b],
                                          (int64_t)tb.max_blocks_per_seq * tb.block_size);
    if (pos < 0) return;
    constexpr int SRC = 8 * elem<T>::bytes;
    kv4_store_chunk<T>(kn + (int64_t)t * st.kb + (int64_t)h * st.kh + SRC * ch,
                       vn + (int64_t)t * st.vb + (int64_t)h * st.vh + SRC * ch, pool, table, b, (int)pos, h, ch, st, tb);
}

struct Kv4Call {
    const void *q, *k, *v, *ke, *ve;
    void* o;
    const int32_t *table, *seq_lens;
    int B, H, Hkv, Nq, D, max_kv, causal, nk_add, dtype;
    Kv4Strides st;
    PagedTable tb;
    float scale;
    hipStream_t stream;
};

template <typename T, int D>
int launch_mxfp4(const Kv4Call& a, const PagedPlan& p, float* ws) {
    const int64_t bh = (int64_t)a.B * a.Hkv;
    const int G = a.H / a.Hkv, M = a.Nq * G;
    const float c = a.scale * 1.4426950408889634f;
    float* part_o = ws;
    float2* part_ml = reinterpret_cast<float2*>(ws + bh * p.splits * M * D);
    hipLaunchKernelGGL((attn_decode_paged_mxfp4<T, D>), dim3((unsigned)(bh * p.splits)), dim3(256), 0, a.stream,
                       (const uint16_t*)a.q, (const uint8_t*)a.k, (const uint8_t*)a.v, (const uint8_t*)a.ke,
                       (const uint8_t*)a.ve, (uint16_t*)a.o, part_o, part_ml, a.table, a.seq_lens, a.Hkv, G, a.Nq, M,
                       a.st, a.tb, c, a.causal, p.chunk, p.splits, a.max_kv, a.nk_add);
    if (p.splits > 1)
        launch_paged_combine(a.dtype, D, part_o, part_ml, a.o, a.B, a.Hkv, G, M, a.st.ob, a.st.oh, a.st.on, p.splits,
                             a.stream);
    return launch_status(p.splits > 1 ? "attn_decode_paged_mxfp4+attn_decode_paged_combine"
                                      : "attn_decode_paged_mxfp4");
}

template <typename T>
int launch_generic_mxfp4(const Kv4Call& a) {
    const int64_t rows = (int64_t)a.B * a.H * a.Nq;
    hipLaunchKernelGGL((attn_decode_paged_generic_mxfp4<T>), dim3((unsigned)rows), dim3(64), 0, a.stream,
                       (const T*)a.q, (const uint8_t*)a.k, (const uint8_t*)a.v, (const uint8_t*)a.ke,
                       (const uint8_t*)a.ve, (T*)a.o, a.table, a.seq_lens, a.H, a.H / a.Hkv, a.Nq, a.D, a.st, a.tb,
                       a.scale, a.causal, a.max_kv, a.nk_add);
    return launch_status("attn_decode_paged_generic_mxfp4");
}

// the checks the two appends share once their shapes are known good; `ns` strides of the call
int append_args(const char* fn, const void* k_new, const void* v_new, const void* k_pool, const void* v_pool,
                const void* k_exp_pool, const void* v_exp_pool, const void* ints, const int64_t* strides,
                const int64_t* exp_strides, int ns, int head_dim, int num_blocks, int max_blocks_per_seq) {
    PLI_REQUIRE(k_new && v_new && k_pool && v_pool && k_exp_pool && v_exp_pool && ints && strides && exp_strides,
                "%s: null pointer", fn);
    PLI_REQUIRE(num_blocks > 0 && max_blocks_per_seq > 0, "%s: empty pool or table (blocks=%d max_blocks_per_seq=%d)",
                fn, num_blocks, max_blocks_per_seq);
    PLI_REQUIRE(aligned16(k_new) && aligned16(v_new) && aligned16(k_pool) && aligned16(v_pool),
                "%s: 16-byte aligned sources and code pools required", fn);
    // the source's strides: whole 8-element chunks; the code pools': whole dwords of eight codes
    for (int i = 0; i < ns; ++i) {
        const bool pool = i >= ns / 2 - 3 && i < ns / 2 + 3;
        PLI_REQUIRE(strides[i] % (pool ? 4 : 8) == 0, "%s: stride %d not a multiple of %d", fn, i, pool ? 4 : 8);
    }
    PLI_REQUIRE(paged_exp_strides_ok(exp_strides, head_dim), "%s: a scale-pool stride is below head_dim / 32 = %d", fn,
                head_dim / kKv4Block);
    return PLI_OK;
}

}  // namespace
}  // namespace pli

extern "C" int pli_attn_decode_paged_mxfp4(const void* q, const void* k_pool, const void* v_pool, void* o,
                                           const int32_t* block_table, const int32_t* seq_lens,
                                           const void* k_exp_pool, const void* v_exp_pool, int batch, int heads,
                                           int kv_heads, int n_q, int head_dim, int block_size, int num_blocks,
                                           int max_blocks_per_seq, int max_kv, const int64_t* strides,
                                           const int64_t* exp_strides, float scale, int causal, int n_kv_add,
                                           void* workspace, size_t workspace_bytes, int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(batch >= 0 && heads > 0 && kv_heads > 0 && n_q >= 0 && head_dim > 0 && num_blocks >= 0 &&
                    max_blocks_per_seq >= 0 && max_kv >= 0,
                "pli_attn_decode_paged_mxfp4: bad shape B=%d H=%d Hkv=%d Nq=%d D=%d blocks=%d "
                "max_blocks_per_seq=%d max_kv=%d",
                batch, heads, kv_heads, n_q, head_dim, num_blocks, max_blocks_per_seq, max_kv);
    PLI_REQUIRE(heads % kv_heads == 0, "pli_attn_decode_paged_mxfp4: heads %d not a multiple of kv_heads %d", heads,
                kv_heads);
    PLI_REQUIRE(dtype == PLI_F32 || dtype == PLI_F16 || dtype == PLI_BF16, "pli_attn_decode_paged_mxfp4: bad dtype %d",
                dtype);
    PLI_REQUIRE(head_dim % kKv4Block == 0, "pli_attn_decode_paged_mxfp4: head_dim %d is not a multiple of the MX block of 32",
                head_dim);
    PLI_REQUIRE(std::isfinite(scale), "pli_attn_decode_paged_mxfp4: non-finite scale");
    PLI_REQUIRE(block_size > 0, "pli_attn_decode_paged_mxfp4: block_size %d must be positive", block_size);
    PLI_REQUIRE((int64_t)max_kv <= (int64_t)max_blocks_per_seq * block_size,
                "pli_attn_decode_paged_mxfp4: max_kv %d past the table row (%d blocks of %d tokens)", max_kv,
                max_blocks_per_seq, block_size);
    PLI_REQUIRE((int64_t)max_blocks_per_seq * block_size < (1ll << 31),
                "pli_attn_decode_paged_mxfp4: a table row of %d blocks x %d tokens passes 2^31 keys",
                max_blocks_per_seq, block_size);
    // no output rows: the (possibly NULL, pli.h) operands are not read
    if (batch == 0 || n_q == 0) return PLI_OK;
    PLI_REQUIRE(q && o && k_pool && v_pool && k_exp_pool && v_exp_pool && block_table && seq_lens && strides &&
                    exp_strides,
                "pli_attn_decode_paged_mxfp4: null pointer");
    PLI_REQUIRE(num_blocks > 0 && max_blocks_per_seq > 0,
                "pli_attn_decode_paged_mxfp4: empty pool or table (blocks=%d max_blocks_per_seq=%d)", num_blocks,
                max_blocks_per_seq);
    PLI_REQUIRE(paged_exp_strides_ok(exp_strides, head_dim),
                "pli_attn_decode_paged_mxfp4: a scale-pool stride is below head_dim / 32 = %d", head_dim / kKv4Block);
    Kv4Call a;
    a.q = q, a.k = k_pool, a.v = v_pool, a.ke = k_exp_pool, a.ve = v_exp_pool, a.o = o;
    a.table = block_table, a.seq_lens = seq_lens;
    a.B = batch, a.H = heads, a.Hkv = kv_heads, a.Nq = n_q, a.D = head_dim, a.max_kv = max_kv, a.dtype = dtype;
    a.causal = causal != 0, a.nk_add = n_kv_add, a.scale = scale, a.stream = (hipStream_t)stream;
    // strides[12] as for pli_attn_decode_paged, the code pools' in bytes; exp_strides[6] the scale pools', in bytes
    a.st = Kv4Strides{strides[0], strides[1], strides[2], strides[9], strides[10], strides[11],
                      PagedPool{strides[3], strides[4], strides[5]}, PagedPool{strides[6], strides[7], strides[8]},
                      PagedPool{exp_strides[0], exp_strides[1], exp_strides[2]},
                      PagedPool{exp_strides[3], exp_strides[4], exp_strides[5]}};
    a.tb = paged_table(block_size, num_blocks, max_blocks_per_seq);
    const int64_t M = (int64_t)n_q * (heads / kv_heads);
    const bool fast = paged_fast_path_mxfp4(dtype, head_dim, M, block_size, scale, strides,
                                            aligned16(q) && aligned16(k_pool) && aligned16(v_pool) && aligned16(o));
    if (!fast) {
        PLI_REQUIRE(head_dim <= GEN4_MAXD, "pli_attn_decode_paged_mxfp4: head_dim %d > %d", head_dim, GEN4_MAXD);
        PLI_REQUIRE((int64_t)batch * heads * n_q < (1ll << 31), "pli_attn_decode_paged_mxfp4: grid too large");
        if (dtype == PLI_F32) return launch_generic_mxfp4<float>(a);
        return dtype == PLI_BF16 ? launch_generic_mxfp4<bf16_t>(a) : launch_generic_mxfp4<f16_t>(a);
    }
    const PagedPlan p = plan_paged(batch, kv_heads, max_kv, M, head_dim);
    const size_t need = (size_t)p.workspace_bytes;
    PLI_REQUIRE(workspace_bytes >= need && (need == 0 || workspace != nullptr),
                "pli_attn_decode_paged_mxfp4: workspace of %zu bytes needed, %zu given", need, workspace_bytes);
    PLI_REQUIRE(need == 0 || aligned16(workspace), "pli_attn_decode_paged_mxfp4: workspace must be 16-byte aligned");
    PLI_REQUIRE((int64_t)batch * kv_heads * p.splits < (1ll << 31), "pli_attn_decode_paged_mxfp4: grid too large");
    float* ws = (float*)workspace;
    if (dtype == PLI_BF16)
        return head_dim == 128 ? launch_mxfp4<bf16_t, 128>(a, p, ws) : launch_mxfp4<bf16_t, 64>(a, p, ws);
    return head_dim == 128 ? launch_mxfp4<f16_t, 128>(a, p, ws) : launch_mxfp4<f16_t, 64>(a, p, ws);
}

extern "C" int pli_kv_append_paged_mxfp4(const void* k_new, const void* v_new, void* k_pool, void* v_pool,
                                         void* k_exp_pool, void* v_exp_pool, const int32_t* block_table,
                                         const int32_t* seq_lens, int batch, int n_new, int kv_heads, int head_dim,
                                         int block_size, int num_blocks, int max_blocks_per_seq,
                                         const int64_t* strides, const int64_t* exp_strides, int dtype, void* stream) {
    using namespace pli;
    clear_error();
    const char* fn = "pli_kv_append_paged_mxfp4";
    PLI_REQUIRE(batch >= 0 && n_new >= 0 && kv_heads > 0 && head_dim > 0 && num_blocks >= 0 && max_blocks_per_seq >= 0,
                "%s: bad shape B=%d T=%d Hkv=%d D=%d blocks=%d max_blocks_per_seq=%d", fn, batch, n_new, kv_heads,
                head_dim, num_blocks, max_blocks_per_seq);
    PLI_REQUIRE(dtype == PLI_F32 || dtype == PLI_F16 || dtype == PLI_BF16, "%s: bad dtype %d", fn, dtype);
    PLI_REQUIRE(head_dim % kKv4Block == 0, "%s: head_dim %d is not a multiple of the MX block of 32", fn, head_dim);
    PLI_REQUIRE(block_size > 0, "%s: block_size %d must be positive", fn, block_size);
    PLI_REQUIRE((int64_t)max_blocks_per_seq * block_size < (1ll << 31),
                "%s: a table row of %d blocks x %d tokens passes 2^31 keys", fn, max_blocks_per_seq, block_size);
    // nothing to append: the (possibly NULL, pli.h) operands are not read
    if (batch == 0 || n_new == 0) return PLI_OK;
    const void* ints = block_table && seq_lens ? block_table : nullptr;
    if (int rc = append_args(fn, k_new, v_new, k_pool, v_pool, k_exp_pool, v_exp_pool, ints, strides, exp_strides, 12,
                             head_dim, num_blocks, max_blocks_per_seq))
        return rc;
    const int es = dtype == PLI_F32 ? 4 : 2;
    const int cpr = head_dim / 8;
    const int64_t total = (int64_t)batch * n_new * kv_heads * cpr;
    PLI_REQUIRE(cdiv64(total, 256) < (1ll << 31), "%s: grid too large", fn);
    // strides[12] as for pli_kv_append_paged: the source's in its elements, the code pools' in bytes
    const Kv4AppendStrides st{strides[0] * es, strides[1] * es, strides[2] * es, strides[9] * es, strides[10] * es,
                              strides[11] * es, PagedPool{strides[3], strides[4], strides[5]},
                              PagedPool{strides[6], strides[7], strides[8]},
                              PagedPool{exp_strides[0], exp_strides[1], exp_strides[2]},
                              PagedPool{exp_strides[3], exp_strides[4], exp_strides[5]}};
    const PagedTable tb = paged_table(block_size, num_blocks, max_blocks_per_seq);
    const Kv4Pools pool{(char*)k_pool, (char*)v_pool, (uint8_t*)k_exp_pool, (uint8_t*)v_exp_pool};
    const dim3 grid((unsigned)cdiv64(total, 256));
#define PLI_KV4_APPEND(T)                                                                                          \
    hipLaunchKernelGGL(kv_append_paged_mxfp4<T>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)k_new,      \
                       (const char*)v_new, pool, block_table, seq_lens, batch, n_new, kv_heads, cpr, st, tb)
    if (dtype == PLI_F32) PLI_KV4_APPEND(float);
    else if (dtype == PLI_BF16) PLI_KV4_APPEND(bf16_t);
    else PLI_KV4_APPEND(f16_t);
#undef PLI_KV4_APPEND
    return launch_status("kv_append_paged_mxfp4");
}

extern "C" int pli_kv_append_varlen_paged_mxfp4(const void* k_new, const void* v_new, void* k_pool, void* v_pool,
                                                void* k_exp_pool, void* v_exp_pool, const int32_t* cu_seqlens_q,
                                                const int32_t* block_table, const int32_t* seq_lens, int batch,
                                                int max_tokens, int kv_heads, int head_dim, int block_size,
                                                int num_blocks, int max_blocks_per_seq, const int64_t* strides,
                                                const int64_t* exp_strides, int dtype, void* stream) {
    using namespace pli;
    clear_error();
    const char* fn = "pli_kv_append_varlen_paged_mxfp4";
    PLI_REQUIRE(batch >= 0 && max_tokens >= 0 && kv_heads > 0 && head_dim > 0 && num_blocks >= 0 &&
                    max_blocks_per_seq >= 0,
                "%s: bad shape B=%d tokens=%d Hkv=%d D=%d blocks=%d max_blocks_per_seq=%d", fn, batch, max_tokens,
                kv_heads, head_dim, num_blocks, max_blocks_per_seq);
    PLI_REQUIRE(dtype == PLI_F32 || dtype == PLI_F16 || dtype == PLI_BF16, "%s: bad dtype %d", fn, dtype);
    PLI_REQUIRE(head_dim % kKv4Block == 0, "%s: head_dim %d is not a multiple of the MX block of 32", fn, head_dim);
    PLI_REQUIRE(block_size > 0, "%s: block_size %d must be positive", fn, block_size);
    PLI_REQUIRE((int64_t)max_blocks_per_seq * block_size < (1ll << 31),
                "%s: a table row of %d blocks x %d tokens passes 2^31 keys", fn, max_blocks_per_seq, block_size);
    // nothing to append: the (possibly NULL, pli.h) operands are not read
    if (batch == 0 || max_tokens == 0) return PLI_OK;
    const void* ints = cu_seqlens_q && block_table && seq_lens ? block_table : nullptr;
    if (int rc = append_args(fn, k_new, v_new, k_pool, v_pool, k_exp_pool, v_exp_pool, ints, strides, exp_strides, 10,
                             head_dim, num_blocks, max_blocks_per_seq))
        return rc;
    const int es = dtype == PLI_F32 ? 4 : 2;
    const int cpr = head_dim / 8;
    const int64_t total = (int64_t)max_tokens * kv_heads * cpr;
    PLI_REQUIRE(cdiv64(total, 256) < (1ll << 31), "%s: grid too large", fn);
    // strides[10] as for pli_kv_append_varlen_paged: the source's in its elements, the code pools' in bytes
    const Kv4AppendStrides st{strides[0] * es, strides[1] * es, 0, strides[8] * es, strides[9] * es, 0,
                              PagedPool{strides[2], strides[3], strides[4]},
                              PagedPool{strides[5], strides[6], strides[7]},
                              PagedPool{exp_strides[0], exp_strides[1], exp_strides[2]},
                              PagedPool{exp_strides[3], exp_strides[4], exp_strides[5]}};
    const PagedTable tb = paged_table(block_size, num_blocks, max_blocks_per_seq);
    const Kv4Pools pool{(char*)k_pool, (char*)v_pool, (uint8_t*)k_exp_pool, (uint8_t*)v_exp_pool};
    const dim3 grid((unsigned)cdiv64(total, 256));
#define PLI_KV4_APPEND(T)                                                                                              \
    hipLaunchKernelGGL(kv_append_varlen_paged_mxfp4<T>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)k_new,  \
                       (const char*)v_new, pool, cu_seqlens_q, block_table, seq_lens, batch, max_tokens, kv_heads, cpr, \
                       st, tb)
    if (dtype == PLI_F32) PLI_KV4_APPEND(float);
    else if (dtype == PLI_BF16) PLI_KV4_APPEND(bf16_t);
    else PLI_KV4_APPEND(f16_t);
#undef PLI_KV4_APPEND
    return launch_status("kv_append_varlen_paged_mxfp4");
}
