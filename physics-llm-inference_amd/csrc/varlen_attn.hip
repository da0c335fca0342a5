// Packed variable-length causal attention over the paged KV pool, and the
// packed append that feeds it, for gfx950: one launch for a step in which
// every sequence brings its own number of new tokens (prompt chunks, decode
// rows and sequences that sit the step out, mixed).
//
// attn_varlen_paged<T, D> keeps the MFMA dataflow of attn_decode_paged
// (paged_attn.hip): S^T = K . Q^T and O^T += V^T . P^T by
// v_mfma_f32_16x16x32, fp32 statistics, 16 query rows per wave.  The roles of
// the waves change:
//   * a workgroup is one tile of VAR_BM = 64 rows of one kv head; row r of a
//     sequence is (token r / G, head hk*G + r % G), so a decode row group reads
//     its keys once per kv head and a prompt chunk fills the tile with 64 / G
//     tokens.  Workgroup w finds its (sequence, tile) from cu_seqlens_q with
//     the rule of varlen_plan.h (one load round per 256 sequences: each lane
//     sums a slice of 4 sequences, the wave prefix-sums the slices) or finds
//     nothing and exits.  The grid depends on (batch, max_tokens, heads,
//     kv_heads) only.
//   * the 4 waves hold the tile's four 16-row groups and share one K/V LDS image
//     per 32-key step.  All 256 threads load the step through the block table
//     (whole-row 16-byte loads, registers, then LDS); the image is
//     double-buffered and the loads run two steps ahead of the MFMAs (two
//     register stages), with one barrier per step.  Each wave keeps its own
//     running max / sum / O: there is no merge at the end.
//   * a 16-key group of a step lies in one page (power-of-two block size >=
//     16), and the lanes of a wave load rows of one group per pass, so the table
//     entry is wave-uniform; the entries of step t + 3 are fetched while step t
//     computes, a step ahead of the loads that use them.
//   * a tile walks keys [0, key_end), key_end one past its last row's causal
//     limit; only steps that cross a row's limit apply the mask.  A wave none
//     of whose rows exist (a decode tile) loads and synchronises but skips the
//     MFMAs.
//   * every address is clamped (token into [0, max_tokens - 1], key to the
//     sequence's last key, block into the table row, page into the pool) and the
//     masks are applied afterwards; stores are predicated.
// attn_varlen_paged_generic covers every other case (fp32, other head dims,
// any block size, any group size): one wave per packed (token, head) row,
// modelled on attn_decode_paged_generic -- a correctness path, not tuned.
// kv_append_varlen_paged_kernel: one thread per 16-byte chunk of a packed
// token's K and V row.
// attn_varlen_paged_fp8 / attn_varlen_paged_generic_fp8 /
// kv_append_varlen_paged_fp8 are the same three over 1-byte pools of fp8 e4m3
// codes (below, "1-byte pools"); the 16-bit kernels are not touched by them.
// attn_varlen_paged_split / attn_varlen_paged_split_fp8 /
// attn_varlen_paged_combine are split-K over a caller workspace
// (pli_attn_varlen_paged_ws): copies again, one workgroup per chunk of a tile's
// key range, merged by the combine kernel; the kernels above are not touched.
#include <cmath>

#include "fp8_kv.h"
#include "pli_common.h"
#include "varlen_plan.h"

namespace pli {
namespace {

inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// element strides: q / o {token, head}; pools {page, token, head}
struct VarStrides {
    int64_t qt, qh, ot, oh;
    PagedPool k, v;
};

template <int D> struct VarLayout {
    static constexpr int KS = 2 * D + 16;  // K row stride in LDS (bytes)
    static constexpr int VS = 2 * D + 32;  // V row stride in LDS (bytes)
    static constexpr int KBYTES = VAR_STEP * KS;
    static constexpr int IMAGE = KBYTES + VAR_STEP * VS;  // one step's K + V
    static constexpr int LDS = 2 * IMAGE;
};

// workgroup w -> (sequence, tile), every lane of the calling wave gets the
// same answer: varlen_find_tile of varlen_plan.h spread over the 64 lanes
__device__ __forceinline__ VarTile find_tile_wave(const int32_t* __restrict__ cu, int batch, int tpt,
                                                  int64_t cap, int64_t w, int lane) {
    int64_t before = 0;
    for (int base = 0; base < batch; base += VAR_SLICE * VAR_LANES) {
        const int first = base + VAR_SLICE * lane;
        const int64_t n = varlen_slice_tiles(cu, batch, first, tpt, cap);
        int64_t incl = n;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        const int64_t lo = before + incl - n;
        const bool hit = w >= lo && w < lo + n;
        const unsigned long long votes = __ballot(hit);
        if (votes) {
            const int src = __ffsll((long long)votes) - 1;
            const int64_t lo_src = __shfl(lo, src, 64);
            return varlen_find_in_slice(cu, batch, base + VAR_SLICE * src, tpt, cap, w - lo_src);
        }
        before += __shfl(incl, 63, 64);
    }
    return VarTile{-1, 0};
}

template <typename T, int D>
__global__ __launch_bounds__(256, 2) void attn_varlen_paged(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
    uint16_t* __restrict__ o, const int32_t* __restrict__ cu, const int32_t* __restrict__ table,
    const int32_t* __restrict__ seq_lens, int batch, int max_tokens, int Hkv, int G, VarStrides st,
    PagedTable tb, float c, int causal, int max_kv, int tiles_upper) {
    using L = VarLayout<D>;
    constexpr int KSTEPS = D / 32;  // 32-d k-steps of K.Q^T
    constexpr int DB = D / 16;      // 16-d blocks of O
    __shared__ __attribute__((aligned(16))) char smem[L::LDS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, g = lane >> 4;
    // block order: (tile, hk) with the kv head innermost, so co-resident
    // workgroups sweep the same pages of all heads
    const int hk = blockIdx.x % Hkv;
    const int w = blockIdx.x / Hkv;
    const int tpt = VAR_BM / G;
    const VarTile found = find_tile_wave(cu, batch, tpt, tiles_upper, w, lane);
    const int b = __builtin_amdgcn_readfirstlane(found.b);
    if (b < 0) return;  // every wave finds the same answer: the whole workgroup leaves
    const int tile = __builtin_amdgcn_readfirstlane(found.tile);
    const int cu_b = cu[b];
    const int q_len = varlen_q_len(cu_b, cu[b + 1]);
    const int live = varlen_tokens_live(cu[batch], max_tokens);
    const int Nk = varlen_n_kv(seq_lens[b], max_kv);
    const int key_end = varlen_key_end(Nk, q_len, tile, tpt, causal);
    const int nsteps = cdiv(key_end, VAR_STEP);

    // this lane's query row: MFMA column l16 of the wave's 16-row group
    const int r = wave * VAR_ROWS + l16;
    const int64_t qi = (int64_t)tile * tpt + r / G;
    const int hq = hk * G + r % G;
    const bool row_ok = qi < q_len;
    // a wave with no row at all (rows are dense from 0) skips the MFMAs
    const bool wave_on = __builtin_amdgcn_readfirstlane((int64_t)tile * tpt + (wave * VAR_ROWS) / G < q_len ? 1 : 0) != 0;
    const int tok = varlen_token(cu_b, qi, max_tokens);
    i32x4 qf[KSTEPS];
    {
        const uint16_t* src = q + (int64_t)tok * st.qt + (int64_t)hq * st.qh + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const i32x4 x = *reinterpret_cast<const i32x4*>(src + 32 * ks);
            qf[ks] = row_ok ? x : i32x4{0, 0, 0, 0};
        }
    }
    // last key this row sees (bottom-right causal per sequence); < 0: none
    const int hi = row_ok ? varlen_row_limit(Nk, q_len, (int)qi, causal) : -1;

    // cooperative row-major loads: thread loads 16-byte chunk rch of step row
    // i*RPP + rrow in pass i; the rows of a wave in a pass lie in one 16-key group
    constexpr int CPR = D / 8, RPP = 256 / CPR, PASSES = VAR_STEP / RPP;
    const int rrow = tid / CPR, rch = tid % CPR;
    const uint16_t* kp = k + 8 * rch;
    const uint16_t* vp = v + 8 * rch;
    // plain loads: the other tiles of the sequence re-read these rows from L2
    auto ld = [](const uint16_t* p) { return *reinterpret_cast<const i32x4*>(p); };
    // raw table entries of the wave's group of each pass: clamping here would
    // wait for the load at once
    auto pages = [&](int key0, int (&e)[PASSES]) {
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
            const int grp = (i * RPP + wave * (64 / CPR)) / 16;
            e[i] = table[paged_table_index(b, varlen_group_block(key0, grp, Nk, tb), tb)];
        }
    };
    auto load_step = [&](int key0, const int (&e)[PASSES], i32x4 (&kr)[PASSES], i32x4 (&vr)[PASSES]) {
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
            const int key = varlen_load_key(key0, i * RPP + rrow, Nk);
            kr[i] = ld(kp + varlen_kv_offset(e[i], key, hk, tb, st.k));
            vr[i] = ld(vp + varlen_kv_offset(e[i], key, hk, tb, st.v));
        }
    };
    const int kw = rrow * L::KS + rch * 16;                     // K row-major write
    const int vw = rrow * L::VS + rch * 16;
    auto store_step = [&](char* img, const i32x4 (&kr)[PASSES], const i32x4 (&vr)[PASSES]) {
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
            lds_write_b128(img + L::KBYTES, vw + i * RPP * L::VS, vr[i]);
            lds_write_b128(img, kw + i * RPP * L::KS, kr[i]);
        }
    };
    const int kr_off = l16 * L::KS + g * 16;                    // K fragment read
    const int qq = l16 >> 2, pp = lane & 3;
    const int vr_off = (4 * g + qq) * L::VS + 8 * pp;           // tr read: key 4g+qq, col 4pp

    f32x4 oacc[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d) oacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;

    // one 32-key step of this wave's 16 rows on the image at `img`
    auto compute = [&](const char* img, int key0) {
        const char* kt = img;
        const char* vt = img + L::KBYTES;
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
        // mask only where the step crosses this row's limit (or n_kv)
        if (key0 + VAR_STEP - 1 > hi) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
                    if (key0 + 16 * kb + 4 * g + rr > hi) s[kb][rr] = -INFINITY;
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
            for (int rr = 0; rr < 4; ++rr) s[kb][rr] = __builtin_amdgcn_exp2f(fmaf(s[kb][rr], c, -m_new));
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
    };

    // Pipeline.  Iteration t: issue step t+2's loads into the free register
    // stage (entries fetched an iteration ago), fetch step t+3's entries,
    // compute step t from image t & 1, write step t+1's registers into the other
    // image, barrier.  The barrier at the end of iteration t-1 is what makes the
    // other image free to overwrite and this one complete to read.
    // The loads and the LDS writes of steps past the last one are NOT skipped:
    // their addresses are clamped like any other (they re-read the sequence's
    // last key) and nobody reads what they write.  Behind a condition, the
    // compiler's wait-count pass sees a path on which a register stage is still
    // in flight when its registers are reused, and waits for every outstanding
    // load before it issues the next step's -- which puts the whole memory
    // latency back into each step.
    i32x4 ka[PASSES], va[PASSES], kb2[PASSES], vb2[PASSES];
    int pn[PASSES];
    auto body = [&](int t, int cur, i32x4 (&kfree)[PASSES], i32x4 (&vfree)[PASSES], i32x4 (&knext)[PASSES],
                    i32x4 (&vnext)[PASSES]) {
        int pf[PASSES];
        pages((t + 3) * VAR_STEP, pf);
        load_step((t + 2) * VAR_STEP, pn, kfree, vfree);
#pragma unroll
        for (int i = 0; i < PASSES; ++i) pn[i] = pf[i];
        if (wave_on && t < nsteps) compute(smem + cur * L::IMAGE, t * VAR_STEP);
        store_step(smem + (cur ^ 1) * L::IMAGE, knext, vnext);
        __syncthreads();
    };
    if (nsteps > 0) {
        int p0[PASSES], p1[PASSES];
        pages(0, p0);
        pages(VAR_STEP, p1);
        pages(2 * VAR_STEP, pn);
        load_step(0, p0, ka, va);
        load_step(VAR_STEP, p1, kb2, vb2);
        store_step(smem, ka, va);
        __syncthreads();
    }
    // two steps per trip (the register stages swap roles).  With an odd step
    // count the last trip's second half loads, writes and synchronises but does
    // not compute: the loop has one exit, so no path re-enters the first half
    // with its register stage in flight (see above).
    for (int t = 0; t < nsteps; t += 2) {
        body(t, 0, ka, va, kb2, vb2);
        body(t + 1, 1, kb2, vb2, ka, va);
    }

    // row sum over the 4 lane groups holding the row
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    if (!varlen_row_stored(cu_b, qi, q_len, live)) return;
    // a row that saw no key (n_kv < q_len rows, an empty sequence) has l = 0: written as 0
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
    // O^T block d: this lane holds dims 16d + 4g .. + 3 of row l16
    uint16_t* op = o + (int64_t)tok * st.ot + (int64_t)hq * st.oh + 4 * g;
#pragma unroll
    for (int d = 0; d < DB; ++d)
        *reinterpret_cast<i32x2*>(op + 16 * d) = i32x2{(int)pack2<T>(oacc[d][0] * inv, oacc[d][1] * inv),
                                                        (int)pack2<T>(oacc[d][2] * inv, oacc[d][3] * inv)};
}

// Any dtype, head_dim <= 256, any block size, any group size: one wave per
// packed (token, head) row; lane l owns dims l, l + 64, ...; keys in order,
// fp32 online softmax.  Correctness path only.
constexpr int VGEN_MAXD = 256, VGEN_DPL = VGEN_MAXD / 64;
template <typename T>
__global__ __launch_bounds__(64) void attn_varlen_paged_generic(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ o,
    const int32_t* __restrict__ cu, const int32_t* __restrict__ table, const int32_t* __restrict__ seq_lens,
    int batch, int max_tokens, int H, int G, int D, VarStrides st, PagedTable tb, float scale, int causal,
    int max_kv) {
    const int lane = threadIdx.x;
    const int h = blockIdx.x % H;
    const int t = blockIdx.x / H;
    if (t >= varlen_tokens_live(cu[batch], max_tokens)) return;
    const int b = varlen_owner(cu, batch, t);
    if (b < 0) return;
    const int hk = h / G;
    const int q_len = varlen_q_len(cu[b], cu[b + 1]);
    const int Nk = varlen_n_kv(seq_lens[b], max_kv);
    const int nvis = varlen_row_limit(Nk, q_len, t - cu[b], causal) + 1;
    const T* qrow = q + (int64_t)t * st.qt + (int64_t)h * st.qh;
    float qv[VGEN_DPL], acc[VGEN_DPL];
#pragma unroll
    for (int i = 0; i < VGEN_DPL; ++i) {
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
        for (int i = 0; i < VGEN_DPL; ++i) {
            const int d = lane + 64 * i;
            if (d < D) dot = fmaf(qv[i], elem<T>::to_f32(krow[d]), dot);
        }
        const float s = wave_sum(dot) * scale;
        const float m_new = fmaxf(m, s);
        const float a = __expf(m - m_new), p = __expf(s - m_new);
        l = fmaf(l, a, p);
#pragma unroll
        for (int i = 0; i < VGEN_DPL; ++i) {
            const int d = lane + 64 * i;
            if (d < D) acc[i] = fmaf(acc[i], a, p * elem<T>::to_f32(vrow[d]));
        }
        m = m_new;
    }
    const float inv = l > 0.f ? 1.f / l : 0.f;  // no visible key: O = 0
    T* orow = o + (int64_t)t * st.ot + (int64_t)h * st.oh;
#pragma unroll
    for (int i = 0; i < VGEN_DPL; ++i) {
        const int d = lane + 64 * i;
        if (d < D) orow[d] = elem<T>::from_f32(acc[i] * inv);
    }
}

// Packed append: one thread per 16-byte chunk of packed token t's K and V row
// of one head; the token's owner comes from cu_seqlens_q, its position from
// varlen_append_pos.  Every stride here is in bytes.
struct VarAppendStrides {
    int64_t kt, kh, vt, vh;  // the new tensors: token, head
    PagedPool k, v;
};
__global__ __launch_bounds__(256) void kv_append_varlen_paged_kernel(
    const char* __restrict__ kn, const char* __restrict__ vn, char* __restrict__ kpool,
    char* __restrict__ vpool, const int32_t* __restrict__ cu, const int32_t* __restrict__ table,
    const int32_t* __restrict__ seq_lens, int batch, int max_tokens, int Hkv, int cpr, VarAppendStrides st,
    PagedTable tb) {
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
    const char* ks = kn + (int64_t)t * st.kt + (int64_t)h * st.kh + 16 * ch;
    const char* vs = vn + (int64_t)t * st.vt + (int64_t)h * st.vh + 16 * ch;
    char* kd = kpool + paged_key_offset(table, b, (int)pos, h, tb, st.k) + 16 * ch;
    char* vd = vpool + paged_key_offset(table, b, (int)pos, h, tb, st.v) + 16 * ch;
    *reinterpret_cast<i32x4*>(kd) = *reinterpret_cast<const i32x4*>(ks);
    *reinterpret_cast<i32x4*>(vd) = *reinterpret_cast<const i32x4*>(vs);
}

// ---- 1-byte pools: OCP fp8 e4m3fn codes, value = code * scale[kv head] --------
// attn_varlen_paged_fp8<T, D> is attn_varlen_paged<T, D> with the pools read as
// bytes.  A thread loads D/8 codes (16 bytes for D 128, 8 for D 64) of one row,
// so the 256 threads cover a 32-key step of K and of V in ONE pass each (the
// 16-bit kernel takes two at D 128): 8 threads per row, wave w the rows 8w ..
// 8w + 7, which lie in 16-key group w / 2.  The codes are widened (exactly, by
// v_cvt_scalef32_pk_*_fp8) to T between the register stage and the LDS write;
// the image, the MFMA loop and the softmax are those of the 16-bit kernel.
// k_scale[hk] is folded into the softmax constant, v_scale[hk] into the final
// 1/l.  Pool strides are in bytes; the scales are read on the device.
template <typename T, int D>
__global__ __launch_bounds__(256, 2) void attn_varlen_paged_fp8(
    const uint16_t* __restrict__ q, const uint8_t* __restrict__ k, const uint8_t* __restrict__ v,
    uint16_t* __restrict__ o, const int32_t* __restrict__ cu, const int32_t* __restrict__ table,
    const int32_t* __restrict__ seq_lens, const float* __restrict__ k_scale, const float* __restrict__ v_scale,
    int batch, int max_tokens, int Hkv, int G, VarStrides st, PagedTable tb, float c_in, int causal, int max_kv,
    int tiles_upper) {
    using L = VarLayout<D>;
    using Stage = typename std::conditional<D == 128, i32x4, i32x2>::type;  // D/8 codes
    constexpr int KSTEPS = D / 32;  // 32-d k-steps of K.Q^T
    constexpr int DB = D / 16;      // 16-d blocks of O
    __shared__ __attribute__((aligned(16))) char smem[L::LDS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, g = lane >> 4;
    const int hk = blockIdx.x % Hkv;
    const int w = blockIdx.x / Hkv;
    const int tpt = VAR_BM / G;
    const VarTile found = find_tile_wave(cu, batch, tpt, tiles_upper, w, lane);
    const int b = __builtin_amdgcn_readfirstlane(found.b);
    if (b < 0) return;  // every wave finds the same answer: the whole workgroup leaves
    const int tile = __builtin_amdgcn_readfirstlane(found.tile);
    const int cu_b = cu[b];
    const int q_len = varlen_q_len(cu_b, cu[b + 1]);
    const int live = varlen_tokens_live(cu[batch], max_tokens);
    const int Nk = varlen_n_kv(seq_lens[b], max_kv);
    const int key_end = varlen_key_end(Nk, q_len, tile, tpt, causal);
    const int nsteps = cdiv(key_end, VAR_STEP);
    const float c = c_in * fp8_scale_of(k_scale, hk);
    const float vsc = fp8_scale_of(v_scale, hk);

    const int r = wave * VAR_ROWS + l16;
    const int64_t qi = (int64_t)tile * tpt + r / G;
    const int hq = hk * G + r % G;
    const bool row_ok = qi < q_len;
    const bool wave_on = __builtin_amdgcn_readfirstlane((int64_t)tile * tpt + (wave * VAR_ROWS) / G < q_len ? 1 : 0) != 0;
    const int tok = varlen_token(cu_b, qi, max_tokens);
    i32x4 qf[KSTEPS];
    {
        const uint16_t* src = q + (int64_t)tok * st.qt + (int64_t)hq * st.qh + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const i32x4 x = *reinterpret_cast<const i32x4*>(src + 32 * ks);
            qf[ks] = row_ok ? x : i32x4{0, 0, 0, 0};
        }
    }
    const int hi = row_ok ? varlen_row_limit(Nk, q_len, (int)qi, causal) : -1;

    // cooperative row-major loads: thread loads chunk rch (D/8 codes) of step row rrow
    constexpr int CPR = 8, LB = D / 8;
    static_assert(256 / CPR == VAR_STEP, "one pass covers a step");
    const int rrow = tid / CPR, rch = tid % CPR;
    const uint8_t* kp = k + LB * rch;
    const uint8_t* vp = v + LB * rch;
    auto ld = [](const uint8_t* p) { return *reinterpret_cast<const Stage*>(p); };
    // raw table entry of the wave's 16-key group: clamping here would wait for the load at once
    auto page = [&](int key0) {
        return table[paged_table_index(b, varlen_group_block(key0, (wave * (64 / CPR)) / 16, Nk, tb), tb)];
    };
    auto load_step = [&](int key0, int e, Stage& kr, Stage& vr) {
        const int key = varlen_load_key(key0, rrow, Nk);
        kr = ld(kp + varlen_kv_offset(e, key, hk, tb, st.k));
        vr = ld(vp + varlen_kv_offset(e, key, hk, tb, st.v));
    };
    const int kw = rrow * L::KS + rch * 2 * LB;                 // D/8 T = 2 LB bytes per thread
    const int vw = rrow * L::VS + rch * 2 * LB;
    // the conversion point: codes -> T, then the row-major padded image
    auto store_step = [&](char* img, const Stage& kr, const Stage& vr) {
        if constexpr (D == 128) {
            i32x4 lo, hi4;
            fp8_widen16<T>(vr, lo, hi4);
            lds_write_b128(img + L::KBYTES, vw, lo);
            lds_write_b128(img + L::KBYTES, vw + 16, hi4);
            fp8_widen16<T>(kr, lo, hi4);
            lds_write_b128(img, kw, lo);
            lds_write_b128(img, kw + 16, hi4);
        } else {
            lds_write_b128(img + L::KBYTES, vw, fp8_widen8<T>(vr));
            lds_write_b128(img, kw, fp8_widen8<T>(kr));
        }
    };
    const int kr_off = l16 * L::KS + g * 16;                    // K fragment read
    const int qq = l16 >> 2, pp = lane & 3;
    const int vr_off = (4 * g + qq) * L::VS + 8 * pp;           // tr read: key 4g+qq, col 4pp

    f32x4 oacc[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d) oacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;

    auto compute = [&](const char* img, int key0) {
        const char* kt = img;
        const char* vt = img + L::KBYTES;
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
        if (key0 + VAR_STEP - 1 > hi) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
                    if (key0 + 16 * kb + 4 * g + rr > hi) s[kb][rr] = -INFINITY;
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
            for (int rr = 0; rr < 4; ++rr) s[kb][rr] = __builtin_amdgcn_exp2f(fmaf(s[kb][rr], c, -m_new));
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
    };

    // the pipeline of attn_varlen_paged: loads two steps ahead in two register
    // stages, entries three steps ahead, one barrier per step; the loads and LDS
    // writes of steps past the last one are not skipped (their addresses are
    // clamped like any other), see the comment there
    Stage ka, va, kb2, vb2;
    int pn = 0;
    auto body = [&](int t, int cur, Stage& kfree, Stage& vfree, Stage& knext, Stage& vnext) {
        const int pf = page((t + 3) * VAR_STEP);
        load_step((t + 2) * VAR_STEP, pn, kfree, vfree);
        pn = pf;
        if (wave_on && t < nsteps) compute(smem + cur * L::IMAGE, t * VAR_STEP);
        store_step(smem + (cur ^ 1) * L::IMAGE, knext, vnext);
        __syncthreads();
    };
    if (nsteps > 0) {
        const int p0 = page(0), p1 = page(VAR_STEP);
        pn = page(2 * VAR_STEP);
        load_step(0, p0, ka, va);
        load_step(VAR_STEP, p1, kb2, vb2);
        store_step(smem, ka, va);
        __syncthreads();
    }
    for (int t = 0; t < nsteps; t += 2) {
        body(t, 0, ka, va, kb2, vb2);
        body(t + 1, 1, kb2, vb2, ka, va);
    }

    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    if (!varlen_row_stored(cu_b, qi, q_len, live)) return;
    const float inv = l_run > 0.f ? vsc / l_run : 0.f;
    uint16_t* op = o + (int64_t)tok * st.ot + (int64_t)hq * st.oh + 4 * g;
#pragma unroll
    for (int d = 0; d < DB; ++d)
        *reinterpret_cast<i32x2*>(op + 16 * d) = i32x2{(int)pack2<T>(oacc[d][0] * inv, oacc[d][1] * inv),
                                                        (int)pack2<T>(oacc[d][2] * inv, oacc[d][3] * inv)};
}

// attn_varlen_paged_generic over 1-byte pools: T is q / o's type, every code
// goes through fp8_e4m3_decode (fp8_codec.h).  Correctness path only.
template <typename T>
__global__ __launch_bounds__(64) void attn_varlen_paged_generic_fp8(
    const T* __restrict__ q, const uint8_t* __restrict__ k, const uint8_t* __restrict__ v, T* __restrict__ o,
    const int32_t* __restrict__ cu, const int32_t* __restrict__ table, const int32_t* __restrict__ seq_lens,
    const float* __restrict__ k_scale, const float* __restrict__ v_scale, int batch, int max_tokens, int H, int G,
    int D, VarStrides st, PagedTable tb, float scale, int causal, int max_kv) {
    const int lane = threadIdx.x;
    const int h = blockIdx.x % H;
    const int t = blockIdx.x / H;
    if (t >= varlen_tokens_live(cu[batch], max_tokens)) return;
    const int b = varlen_owner(cu, batch, t);
    if (b < 0) return;
    const int hk = h / G;
    const int q_len = varlen_q_len(cu[b], cu[b + 1]);
    const int Nk = varlen_n_kv(seq_lens[b], max_kv);
    const int nvis = varlen_row_limit(Nk, q_len, t - cu[b], causal) + 1;
    const float sc = scale * fp8_scale_of(k_scale, hk);
    const T* qrow = q + (int64_t)t * st.qt + (int64_t)h * st.qh;
    float qv[VGEN_DPL], acc[VGEN_DPL];
#pragma unroll
    for (int i = 0; i < VGEN_DPL; ++i) {
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
        for (int i = 0; i < VGEN_DPL; ++i) {
            const int d = lane + 64 * i;
            if (d < D) dot = fmaf(qv[i], fp8_e4m3_decode(krow[d]), dot);
        }
        const float s = wave_sum(dot) * sc;
        const float m_new = fmaxf(m, s);
        const float a = __expf(m - m_new), p = __expf(s - m_new);
        l = fmaf(l, a, p);
#pragma unroll
        for (int i = 0; i < VGEN_DPL; ++i) {
            const int d = lane + 64 * i;
            if (d < D) acc[i] = fmaf(acc[i], a, p * fp8_e4m3_decode(vrow[d]));
        }
        m = m_new;
    }
    const float inv = l > 0.f ? fp8_scale_of(v_scale, hk) / l : 0.f;  // no visible key: O = 0
    T* orow = o + (int64_t)t * st.ot + (int64_t)h * st.oh;
#pragma unroll
    for (int i = 0; i < VGEN_DPL; ++i) {
        const int d = lane + 64 * i;
        if (d < D) orow[d] = elem<T>::from_f32(acc[i] * inv);
    }
}

// kv_append_varlen_paged_kernel that quantises: one thread per 8 elements of a
// packed token's row, read as 16 (bf16 / fp16) or 32 (fp32) bytes of the source
// and stored as one 8-byte chunk of codes (fp8_kv.h).  Source strides in bytes
// of the source, pool strides in bytes.
template <typename T>
__global__ __launch_bounds__(256) void kv_append_varlen_paged_fp8(
    const char* __restrict__ kn, const char* __restrict__ vn, char* __restrict__ kpool,
    char* __restrict__ vpool, const int32_t* __restrict__ cu, const int32_t* __restrict__ table,
    const int32_t* __restrict__ seq_lens, const float* __restrict__ k_scale, const float* __restrict__ v_scale,
    int batch, int max_tokens, int Hkv, int cpr, VarAppendStrides st, PagedTable tb) {
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
    const char* ks = kn + (int64_t)t * st.kt + (int64_t)h * st.kh + SRC * ch;
    const char* vs = vn + (int64_t)t * st.vt + (int64_t)h * st.vh + SRC * ch;
    char* kd = kpool + paged_key_offset(table, b, (int)pos, h, tb, st.k) + 8 * ch;
    char* vd = vpool + paged_key_offset(table, b, (int)pos, h, tb, st.v) + 8 * ch;
    *reinterpret_cast<i32x2*>(kd) = fp8_encode8<T>(ks, 1.0f / fp8_scale_of(k_scale, h));
    *reinterpret_cast<i32x2*>(vd) = fp8_encode8<T>(vs, 1.0f / fp8_scale_of(v_scale, h));
}

// ---- split-K: a tile's key range cut into chunks (varlen_plan.h) ----------------
// attn_varlen_paged_split<T, D> is attn_varlen_paged<T, D> (a copy, so that
// kernel's registers and schedule stay what they are) whose workgroup is one
// CHUNK of a tile: block order (tile, chunk, kv head), the kv head innermost.
// It walks the chunk's steps only -- the chunk starts on an even step, so the
// prologue, the two-steps-per-trip loop and its unconditional clamped tail loads
// are those of the whole-range walk shifted to step t0.  A workgroup without a
// tile or whose chunk number is past the tile's chunks leaves before any K / V
// load.  A tile with one chunk normalises and stores O as attn_varlen_paged
// does (bitwise the same rows); otherwise every stored row writes its
// unnormalised fp32 O and (m, l), m in the log2 domain, to the workspace row of
// (chunk, packed token, head), and attn_varlen_paged_combine merges them.  A row
// that sees no key of its chunk writes (-1e30, 0, 0): its scores are all -inf.
struct VarSplit {
    float* part_o;     // [splits][max_tokens][heads][D]
    float2* part_ml;   // [splits][max_tokens][heads]
    int span, splits;
};

template <typename T, int D>
__global__ __launch_bounds__(256, 2) void attn_varlen_paged_split(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
    uint16_t* __restrict__ o, const int32_t* __restrict__ cu, const int32_t* __restrict__ table,
    const int32_t* __restrict__ seq_lens, int batch, int max_tokens, int Hkv, int G, VarStrides st,
    PagedTable tb, float c, int causal, int max_kv, int tiles_upper, VarSplit sp) {
    using L = VarLayout<D>;
    constexpr int KSTEPS = D / 32;  // 32-d k-steps of K.Q^T
    constexpr int DB = D / 16;      // 16-d blocks of O
    __shared__ __attribute__((aligned(16))) char smem[L::LDS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, g = lane >> 4;
    const int hk = blockIdx.x % Hkv;
    const int split = (blockIdx.x / Hkv) % sp.splits;
    const int w = blockIdx.x / Hkv / sp.splits;
    const int tpt = VAR_BM / G;
    const VarTile found = find_tile_wave(cu, batch, tpt, tiles_upper, w, lane);
    const int b = __builtin_amdgcn_readfirstlane(found.b);
    if (b < 0) return;  // every wave finds the same answer: the whole workgroup leaves
    const int tile = __builtin_amdgcn_readfirstlane(found.tile);
    const int cu_b = cu[b], cu_b1 = cu[b + 1], len_b = seq_lens[b];
    const int chunks = __builtin_amdgcn_readfirstlane(
        varlen_tile_chunks(cu_b, cu_b1, len_b, max_kv, tile, tpt, causal, sp.span, sp.splits));
    if (split >= chunks) return;  // uniform too
    const int q_len = varlen_q_len(cu_b, cu_b1);
    const int live = varlen_tokens_live(cu[batch], max_tokens);
    const int Nk = varlen_n_kv(len_b, max_kv);
    const int key_end = varlen_key_end(Nk, q_len, tile, tpt, causal);
    // this chunk's steps [t0, nsteps) of the tile's walk, t0 even
    const int t0 = varlen_chunk_begin(split, sp.span) / VAR_STEP;
    const int nsteps = cdiv(varlen_chunk_end(split, sp.span, key_end), VAR_STEP);

    const int r = wave * VAR_ROWS + l16;
    const int64_t qi = (int64_t)tile * tpt + r / G;
    const int hq = hk * G + r % G;
    const bool row_ok = qi < q_len;
    const bool wave_on = __builtin_amdgcn_readfirstlane((int64_t)tile * tpt + (wave * VAR_ROWS) / G < q_len ? 1 : 0) != 0;
    const int tok = varlen_token(cu_b, qi, max_tokens);
    i32x4 qf[KSTEPS];
    {
        const uint16_t* src = q + (int64_t)tok * st.qt + (int64_t)hq * st.qh + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const i32x4 x = *reinterpret_cast<const i32x4*>(src + 32 * ks);
            qf[ks] = row_ok ? x : i32x4{0, 0, 0, 0};
        }
    }
    const int hi = row_ok ? varlen_row_limit(Nk, q_len, (int)qi, causal) : -1;

    constexpr int CPR = D / 8, RPP = 256 / CPR, PASSES = VAR_STEP / RPP;
    const int rrow = tid / CPR, rch = tid % CPR;
    const uint16_t* kp = k + 8 * rch;
    const uint16_t* vp = v + 8 * rch;
    auto ld = [](const uint16_t* p) { return *reinterpret_cast<const i32x4*>(p); };
    auto pages = [&](int key0, int (&e)[PASSES]) {
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
            const int grp = (i * RPP + wave * (64 / CPR)) / 16;
            e[i] = table[paged_table_index(b, varlen_group_block(key0, grp, Nk, tb), tb)];
        }
    };
    auto load_step = [&](int key0, const int (&e)[PASSES], i32x4 (&kr)[PASSES], i32x4 (&vr)[PASSES]) {
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
            const int key = varlen_load_key(key0, i * RPP + rrow, Nk);
            kr[i] = ld(kp + varlen_kv_offset(e[i], key, hk, tb, st.k));
            vr[i] = ld(vp + varlen_kv_offset(e[i], key, hk, tb, st.v));
        }
    };
    const int kw = rrow * L::KS + rch * 16;
    const int vw = rrow * L::VS + rch * 16;
    auto store_step = [&](char* img, const i32x4 (&kr)[PASSES], const i32x4 (&vr)[PASSES]) {
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
            lds_write_b128(img + L::KBYTES, vw + i * RPP * L::VS, vr[i]);
            lds_write_b128(img, kw + i * RPP * L::KS, kr[i]);
        }
    };
    const int kr_off = l16 * L::KS + g * 16;
    const int qq = l16 >> 2, pp = lane & 3;
    const int vr_off = (4 * g + qq) * L::VS + 8 * pp;

    f32x4 oacc[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d) oacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;

    auto compute = [&](const char* img, int key0) {
        const char* kt = img;
        const char* vt = img + L::KBYTES;
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
        if (key0 + VAR_STEP - 1 > hi) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
                    if (key0 + 16 * kb + 4 * g + rr > hi) s[kb][rr] = -INFINITY;
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
            for (int rr = 0; rr < 4; ++rr) s[kb][rr] = __builtin_amdgcn_exp2f(fmaf(s[kb][rr], c, -m_new));
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
    };

    // the pipeline of attn_varlen_paged from step t0: see the comment there on
    // why the loads and LDS writes past the last step are not skipped (here
    // they read the next chunk's keys, or re-read the sequence's last key)
    i32x4 ka[PASSES], va[PASSES], kb2[PASSES], vb2[PASSES];
    int pn[PASSES];
    auto body = [&](int t, int cur, i32x4 (&kfree)[PASSES], i32x4 (&vfree)[PASSES], i32x4 (&knext)[PASSES],
                    i32x4 (&vnext)[PASSES]) {
        int pf[PASSES];
        pages((t + 3) * VAR_STEP, pf);
        load_step((t + 2) * VAR_STEP, pn, kfree, vfree);
#pragma unroll
        for (int i = 0; i < PASSES; ++i) pn[i] = pf[i];
        if (wave_on && t < nsteps) compute(smem + cur * L::IMAGE, t * VAR_STEP);
        store_step(smem + (cur ^ 1) * L::IMAGE, knext, vnext);
        __syncthreads();
    };
    if (t0 < nsteps) {
        int p0[PASSES], p1[PASSES];
        pages(t0 * VAR_STEP, p0);
        pages((t0 + 1) * VAR_STEP, p1);
        pages((t0 + 2) * VAR_STEP, pn);
        load_step(t0 * VAR_STEP, p0, ka, va);
        load_step((t0 + 1) * VAR_STEP, p1, kb2, vb2);
        store_step(smem, ka, va);
        __syncthreads();
    }
    for (int t = t0; t < nsteps; t += 2) {
        body(t, 0, ka, va, kb2, vb2);
        body(t + 1, 1, kb2, vb2, ka, va);
    }

    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    if (!varlen_row_stored(cu_b, qi, q_len, live)) return;
    if (chunks == 1) {
        const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
        uint16_t* op = o + (int64_t)tok * st.ot + (int64_t)hq * st.oh + 4 * g;
#pragma unroll
        for (int d = 0; d < DB; ++d)
            *reinterpret_cast<i32x2*>(op + 16 * d) = i32x2{(int)pack2<T>(oacc[d][0] * inv, oacc[d][1] * inv),
                                                            (int)pack2<T>(oacc[d][2] * inv, oacc[d][3] * inv)};
        return;
    }
    // a stored row's token is its own (not a clamped one): the partial row is inside the workspace
    const int64_t pr = varlen_partial_row(split, tok, hq, max_tokens, Hkv * G);
    float* po = sp.part_o + pr * D + 4 * g;
#pragma unroll
    for (int d = 0; d < DB; ++d) *reinterpret_cast<f32x4*>(po + 16 * d) = oacc[d];
    if (g == 0) sp.part_ml[pr] = float2{m_run, l_run};
}

// attn_varlen_paged_fp8<T, D> cut the same way (a copy of that kernel with the
// changes of attn_varlen_paged_split).  k_scale is folded into c; a partial
// stores l / v_scale, so that the combine's O / l carries v_scale and one
// combine kernel serves both pools.
template <typename T, int D>
__global__ __launch_bounds__(256, 2) void attn_varlen_paged_split_fp8(
    const uint16_t* __restrict__ q, const uint8_t* __restrict__ k, const uint8_t* __restrict__ v,
    uint16_t* __restrict__ o, const int32_t* __restrict__ cu, const int32_t* __restrict__ table,
    const int32_t* __restrict__ seq_lens, const float* __restrict__ k_scale, const float* __restrict__ v_scale,
    int batch, int max_tokens, int Hkv, int G, VarStrides st, PagedTable tb, float c_in, int causal, int max_kv,
    int tiles_upper, VarSplit sp) {
    using L = VarLayout<D>;
    using Stage = typename std::conditional<D == 128, i32x4, i32x2>::type;  // D/8 codes
    constexpr int KSTEPS = D / 32;
    constexpr int DB = D / 16;
    __shared__ __attribute__((aligned(16))) char smem[L::LDS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, g = lane >> 4;
    const int hk = blockIdx.x % Hkv;
    const int split = (blockIdx.x / Hkv) % sp.splits;
    const int w = blockIdx.x / Hkv / sp.splits;
    const int tpt = VAR_BM / G;
    const VarTile found = find_tile_wave(cu, batch, tpt, tiles_upper, w, lane);
    const int b = __builtin_amdgcn_readfirstlane(found.b);
    if (b < 0) return;
    const int tile = __builtin_amdgcn_readfirstlane(found.tile);
    const int cu_b = cu[b], cu_b1 = cu[b + 1], len_b = seq_lens[b];
    const int chunks = __builtin_amdgcn_readfirstlane(
        varlen_tile_chunks(cu_b, cu_b1, len_b, max_kv, tile, tpt, causal, sp.span, sp.splits));
    if (split >= chunks) return;
    const int q_len = varlen_q_len(cu_b, cu_b1);
    const int live = varlen_tokens_live(cu[batch], max_tokens);
    const int Nk = varlen_n_kv(len_b, max_kv);
    const int key_end = varlen_key_end(Nk, q_len, tile, tpt, causal);
    const int t0 = varlen_chunk_begin(split, sp.span) / VAR_STEP;
    const int nsteps = cdiv(varlen_chunk_end(split, sp.span, key_end), VAR_STEP);
    const float c = c_in * fp8_scale_of(k_scale, hk);
    const float vsc = fp8_scale_of(v_scale, hk);

    const int r = wave * VAR_ROWS + l16;
    const int64_t qi = (int64_t)tile * tpt + r / G;
    const int hq = hk * G + r % G;
    const bool row_ok = qi < q_len;
    const bool wave_on = __builtin_amdgcn_readfirstlane((int64_t)tile * tpt + (wave * VAR_ROWS) / G < q_len ? 1 : 0) != 0;
    const int tok = varlen_token(cu_b, qi, max_tokens);
    i32x4 qf[KSTEPS];
    {
        const uint16_t* src = q + (int64_t)tok * st.qt + (int64_t)hq * st.qh + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const i32x4 x = *reinterpret_cast<const i32x4*>(src + 32 * ks);
            qf[ks] = row_ok ? x : i32x4{0, 0, 0, 0};
        }
    }
    const int hi = row_ok ? varlen_row_limit(Nk, q_len, (int)qi, causal) : -1;

    constexpr int CPR = 8, LB = D / 8;
    static_assert(256 / CPR == VAR_STEP, "one pass covers a step");
    const int rrow = tid / CPR, rch = tid % CPR;
    const uint8_t* kp = k + LB * rch;
    const uint8_t* vp = v + LB * rch;
    auto ld = [](const uint8_t* p) { return *reinterpret_cast<const Stage*>(p); };
    auto page = [&](int key0) {
        return table[paged_table_index(b, varlen_group_block(key0, (wave * (64 / CPR)) / 16, Nk, tb), tb)];
    };
    auto load_step = [&](int key0, int e, Stage& kr, Stage& vr) {
        const int key = varlen_load_key(key0, rrow, Nk);
        kr = ld(kp + varlen_kv_offset(e, key, hk, tb, st.k));
        vr = ld(vp + varlen_kv_offset(e, key, hk, tb, st.v));
    };
    const int kw = rrow * L::KS + rch * 2 * LB;
    const int vw = rrow * L::VS + rch * 2 * LB;
    auto store_step = [&](char* img, const Stage& kr, const Stage& vr) {
        if constexpr (D == 128) {
            i32x4 lo, hi4;
            fp8_widen16<T>(vr, lo, hi4);
            lds_write_b128(img + L::KBYTES, vw, lo);
            lds_write_b128(img + L::KBYTES, vw + 16, hi4);
            fp8_widen16<T>(kr, lo, hi4);
            lds_write_b128(img, kw, lo);
            lds_write_b128(img, kw + 16, hi4);
        } else {
            lds_write_b128(img + L::KBYTES, vw, fp8_widen8<T>(vr));
            lds_write_b128(img, kw, fp8_widen8<T>(kr));
        }
    };
    const int kr_off = l16 * L::KS + g * 16;
    const int qq = l16 >> 2, pp = lane & 3;
    const int vr_off = (4 * g + qq) * L::VS + 8 * pp;

    f32x4 oacc[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d) oacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;

    auto compute = [&](const char* img, int key0) {
        const char* kt = img;
        const char* vt = img + L::KBYTES;
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
        if (key0 + VAR_STEP - 1 > hi) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
                    if (key0 + 16 * kb + 4 * g + rr > hi) s[kb][rr] = -INFINITY;
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
            for (int rr = 0; rr < 4; ++rr) s[kb][rr] = __builtin_amdgcn_exp2f(fmaf(s[kb][rr], c, -m_new));
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
    };

    // the pipeline of attn_varlen_paged_fp8 from step t0
    Stage ka, va, kb2, vb2;
    int pn = 0;
    auto body = [&](int t, int cur, Stage& kfree, Stage& vfree, Stage& knext, Stage& vnext) {
        const int pf = page((t + 3) * VAR_STEP);
        load_step((t + 2) * VAR_STEP, pn, kfree, vfree);
        pn = pf;
        if (wave_on && t < nsteps) compute(smem + cur * L::IMAGE, t * VAR_STEP);
        store_step(smem + (cur ^ 1) * L::IMAGE, knext, vnext);
        __syncthreads();
    };
    if (t0 < nsteps) {
        const int p0 = page(t0 * VAR_STEP), p1 = page((t0 + 1) * VAR_STEP);
        pn = page((t0 + 2) * VAR_STEP);
        load_step(t0 * VAR_STEP, p0, ka, va);
        load_step((t0 + 1) * VAR_STEP, p1, kb2, vb2);
        store_step(smem, ka, va);
        __syncthreads();
    }
    for (int t = t0; t < nsteps; t += 2) {
        body(t, 0, ka, va, kb2, vb2);
        body(t + 1, 1, kb2, vb2, ka, va);
    }

    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    if (!varlen_row_stored(cu_b, qi, q_len, live)) return;
    if (chunks == 1) {
        const float inv = l_run > 0.f ? vsc / l_run : 0.f;
        uint16_t* op = o + (int64_t)tok * st.ot + (int64_t)hq * st.oh + 4 * g;
#pragma unroll
        for (int d = 0; d < DB; ++d)
            *reinterpret_cast<i32x2*>(op + 16 * d) = i32x2{(int)pack2<T>(oacc[d][0] * inv, oacc[d][1] * inv),
                                                            (int)pack2<T>(oacc[d][2] * inv, oacc[d][3] * inv)};
        return;
    }
    const int64_t pr = varlen_partial_row(split, tok, hq, max_tokens, Hkv * G);
    float* po = sp.part_o + pr * D + 4 * g;
#pragma unroll
    for (int d = 0; d < DB; ++d) *reinterpret_cast<f32x4*>(po + 16 * d) = oacc[d];
    if (g == 0) sp.part_ml[pr] = float2{m_run, l_run / vsc};
}

// Merge the chunks of a packed (token, head) row: thread = (row, 16-byte chunk
// of the row), so a wave holds 64 / (D / 4) rows.  The row's owner, tile and
// chunk count come from the device tensors by the functions the split kernel
// uses (varlen_owner, varlen_tile_chunks); a row of a one-chunk tile was
// stored by the split kernel and is left alone, a row nobody stores is left
// alone, and only partials of chunks 0 .. chunks - 1 -- exactly those this
// call's split kernel wrote for the row -- are read, in that order, with the
// arithmetic of attn_decode_paged_combine (paged_attn.hip).
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_varlen_paged_combine(
    const float* __restrict__ part_o, const float2* __restrict__ part_ml, uint16_t* __restrict__ o,
    const int32_t* __restrict__ cu, const int32_t* __restrict__ seq_lens, int batch, int max_tokens, int H, int G,
    int64_t ot, int64_t oh, int causal, int max_kv, int span, int splits) {
    constexpr int CH = D / 4;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int cc = (int)(idx % CH);
    const int64_t row = idx / CH;
    if (row >= (int64_t)max_tokens * H) return;
    const int h = (int)(row % H), t = (int)(row / H);
    const int live = varlen_tokens_live(cu[batch], max_tokens);
    if (t >= live) return;
    const int b = varlen_owner(cu, batch, t);
    if (b < 0) return;
    const int cu_b = cu[b], cu_b1 = cu[b + 1];
    const int64_t i = (int64_t)t - cu_b;
    const int tpt = VAR_BM / G;
    if (!varlen_row_stored(cu_b, i, varlen_q_len(cu_b, cu_b1), live)) return;
    const int chunks = varlen_tile_chunks(cu_b, cu_b1, seq_lens[b], max_kv, varlen_row_tile(i, tpt), tpt, causal, span, splits);
    if (chunks <= 1) return;
    float mt = -1e30f, lt = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int s = 0; s < chunks; ++s) {
        const int64_t pr = varlen_partial_row(s, t, h, max_tokens, H);
        const float2 ml = part_ml[pr];
        const f32x4 po = *reinterpret_cast<const f32x4*>(part_o + pr * D + 4 * cc);
        const float mn = fmaxf(mt, ml.x);
        const float wa = __builtin_amdgcn_exp2f(mt - mn), wb = __builtin_amdgcn_exp2f(ml.x - mn);
        acc = acc * wa + po * wb;
        lt = lt * wa + ml.y * wb;
        mt = mn;
    }
    const float inv = lt > 0.f ? 1.f / lt : 0.f;  // no chunk saw a key: written as 0
    uint16_t* op = o + (int64_t)t * ot + (int64_t)h * oh + 4 * cc;
    *reinterpret_cast<i32x2*>(op) =
        i32x2{(int)pack2<T>(acc[0] * inv, acc[1] * inv), (int)pack2<T>(acc[2] * inv, acc[3] * inv)};
}

struct VarCall {
    const void *q, *k, *v;
    void* o;
    const int32_t *cu, *table, *seq_lens;
    int B, T, H, Hkv, D, max_kv, causal;
    VarStrides st;
    PagedTable tb;
    float scale;
    hipStream_t stream;
};

template <typename T, int D>
int launch_varlen(const VarCall& a, int64_t tiles_upper) {
    const float c = a.scale * 1.4426950408889634f;
    hipLaunchKernelGGL((attn_varlen_paged<T, D>), dim3((unsigned)(tiles_upper * a.Hkv)), dim3(256), 0, a.stream,
                       (const uint16_t*)a.q, (const uint16_t*)a.k, (const uint16_t*)a.v, (uint16_t*)a.o, a.cu,
                       a.table, a.seq_lens, a.B, a.T, a.Hkv, a.H / a.Hkv, a.st, a.tb, c, a.causal, a.max_kv,
                       (int)tiles_upper);
    return launch_status("attn_varlen_paged");
}

template <typename T>
int launch_varlen_generic(const VarCall& a) {
    hipLaunchKernelGGL((attn_varlen_paged_generic<T>), dim3((unsigned)((int64_t)a.T * a.H)), dim3(64), 0, a.stream,
                       (const T*)a.q, (const T*)a.k, (const T*)a.v, (T*)a.o, a.cu, a.table, a.seq_lens, a.B, a.T,
                       a.H, a.H / a.Hkv, a.D, a.st, a.tb, a.scale, a.causal, a.max_kv);
    return launch_status("attn_varlen_paged_generic");
}

template <typename T, int D>
int launch_varlen_fp8(const VarCall& a, const Fp8Scales& sc, int64_t tiles_upper) {
    const float c = a.scale * 1.4426950408889634f;
    hipLaunchKernelGGL((attn_varlen_paged_fp8<T, D>), dim3((unsigned)(tiles_upper * a.Hkv)), dim3(256), 0, a.stream,
                       (const uint16_t*)a.q, (const uint8_t*)a.k, (const uint8_t*)a.v, (uint16_t*)a.o, a.cu, a.table,
                       a.seq_lens, sc.k, sc.v, a.B, a.T, a.Hkv, a.H / a.Hkv, a.st, a.tb, c, a.causal, a.max_kv,
                       (int)tiles_upper);
    return launch_status("attn_varlen_paged_fp8");
}

template <typename T>
int launch_varlen_generic_fp8(const VarCall& a, const Fp8Scales& sc) {
    hipLaunchKernelGGL((attn_varlen_paged_generic_fp8<T>), dim3((unsigned)((int64_t)a.T * a.H)), dim3(64), 0,
                       a.stream, (const T*)a.q, (const uint8_t*)a.k, (const uint8_t*)a.v, (T*)a.o, a.cu, a.table,
                       a.seq_lens, sc.k, sc.v, a.B, a.T, a.H, a.H / a.Hkv, a.D, a.st, a.tb, a.scale, a.causal,
                       a.max_kv);
    return launch_status("attn_varlen_paged_generic_fp8");
}

// split + combine: grids tiles_upper x splits_max x kv_heads and ceil(rows * D/4 / 256), both from host arguments
template <typename T, int D>
int launch_varlen_split(const VarCall& a, const Fp8Scales* sc, int64_t tiles_upper, const VarSplitPlan& p, void* ws) {
    const float c = a.scale * 1.4426950408889634f;
    const int64_t rows = (int64_t)p.splits_max * a.T * a.H;
    VarSplit sp;
    sp.part_o = (float*)ws;
    sp.part_ml = reinterpret_cast<float2*>((float*)ws + rows * D);
    sp.span = p.span, sp.splits = p.splits_max;
    const dim3 grid((unsigned)(tiles_upper * p.splits_max * a.Hkv));
    if (sc)
        hipLaunchKernelGGL((attn_varlen_paged_split_fp8<T, D>), grid, dim3(256), 0, a.stream, (const uint16_t*)a.q,
                           (const uint8_t*)a.k, (const uint8_t*)a.v, (uint16_t*)a.o, a.cu, a.table, a.seq_lens, sc->k,
                           sc->v, a.B, a.T, a.Hkv, a.H / a.Hkv, a.st, a.tb, c, a.causal, a.max_kv, (int)tiles_upper, sp);
    else
        hipLaunchKernelGGL((attn_varlen_paged_split<T, D>), grid, dim3(256), 0, a.stream, (const uint16_t*)a.q,
                           (const uint16_t*)a.k, (const uint16_t*)a.v, (uint16_t*)a.o, a.cu, a.table, a.seq_lens, a.B,
                           a.T, a.Hkv, a.H / a.Hkv, a.st, a.tb, c, a.causal, a.max_kv, (int)tiles_upper, sp);
    hipLaunchKernelGGL((attn_varlen_paged_combine<T, D>), dim3((unsigned)cdiv64((int64_t)a.T * a.H * (D / 4), 256)),
                       dim3(256), 0, a.stream, sp.part_o, sp.part_ml, (uint16_t*)a.o, a.cu, a.seq_lens, a.B, a.T, a.H,
                       a.H / a.Hkv, a.st.ot, a.st.oh, a.causal, a.max_kv, p.span, p.splits_max);
    return launch_status(sc ? "attn_varlen_paged_split_fp8+attn_varlen_paged_combine"
                            : "attn_varlen_paged_split+attn_varlen_paged_combine");
}

template <typename T>
int launch_varlen_append_fp8(const char* kn, const char* vn, char* kpool, char* vpool, const int32_t* cu,
                             const int32_t* table, const int32_t* seq_lens, const Fp8Scales& sc, int batch,
                             int max_tokens, int Hkv, int cpr, const VarAppendStrides& st, const PagedTable& tb,
                             hipStream_t stream) {
    const int64_t total = (int64_t)max_tokens * Hkv * cpr;
    hipLaunchKernelGGL(kv_append_varlen_paged_fp8<T>, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, stream, kn,
                       vn, kpool, vpool, cu, table, seq_lens, sc.k, sc.v, batch, max_tokens, Hkv, cpr, st, tb);
    return launch_status("kv_append_varlen_paged_fp8");
}

}  // namespace
}  // namespace pli

extern "C" int pli_attn_varlen_paged(const void* q, const void* k_pool, const void* v_pool, void* o,
                                     const int32_t* cu_seqlens_q, const int32_t* block_table,
                                     const int32_t* seq_lens, int batch, int max_tokens, int heads,
                                     int kv_heads, int head_dim, int block_size, int num_blocks,
                                     int max_blocks_per_seq, int max_kv, const int64_t* strides, float scale,
                                     int causal, int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(batch >= 0 && max_tokens >= 0 && heads > 0 && kv_heads > 0 && head_dim > 0 && num_blocks >= 0 &&
                    max_blocks_per_seq >= 0 && max_kv >= 0,
                "pli_attn_varlen_paged: bad shape B=%d tokens=%d H=%d Hkv=%d D=%d blocks=%d "
                "max_blocks_per_seq=%d max_kv=%d",
                batch, max_tokens, heads, kv_heads, head_dim, num_blocks, max_blocks_per_seq, max_kv);
    PLI_REQUIRE(heads % kv_heads == 0, "pli_attn_varlen_paged: heads %d not a multiple of kv_heads %d", heads,
                kv_heads);
    PLI_REQUIRE(dtype == PLI_F32 || dtype == PLI_F16 || dtype == PLI_BF16, "pli_attn_varlen_paged: bad dtype %d",
                dtype);
    PLI_REQUIRE(std::isfinite(scale), "pli_attn_varlen_paged: non-finite scale");
    PLI_REQUIRE(block_size > 0, "pli_attn_varlen_paged: block_size %d must be positive", block_size);
    PLI_REQUIRE((int64_t)max_kv <= (int64_t)max_blocks_per_seq * block_size,
                "pli_attn_varlen_paged: max_kv %d past the table row (%d blocks of %d tokens)", max_kv,
                max_blocks_per_seq, block_size);
    PLI_REQUIRE((int64_t)max_blocks_per_seq * block_size < (1ll << 31),
                "pli_attn_varlen_paged: a table row of %d blocks x %d tokens passes 2^31 keys", max_blocks_per_seq,
                block_size);
    // no output rows: the (possibly NULL, pli.h) operands are not read
    if (batch == 0 || max_tokens == 0) return PLI_OK;
    PLI_REQUIRE(q && o && k_pool && v_pool && cu_seqlens_q && block_table && seq_lens && strides,
                "pli_attn_varlen_paged: null pointer");
    PLI_REQUIRE(num_blocks > 0 && max_blocks_per_seq > 0,
                "pli_attn_varlen_paged: empty pool or table (blocks=%d max_blocks_per_seq=%d)", num_blocks,
                max_blocks_per_seq);
    VarCall a;
    a.q = q, a.k = k_pool, a.v = v_pool, a.o = o, a.cu = cu_seqlens_q, a.table = block_table, a.seq_lens = seq_lens;
    a.B = batch, a.T = max_tokens, a.H = heads, a.Hkv = kv_heads, a.D = head_dim, a.max_kv = max_kv;
    a.causal = causal != 0, a.scale = scale, a.stream = (hipStream_t)stream;
    // strides[10] = {q_t, q_h, k_page, k_token, k_head, v_page, v_token, v_head, o_t, o_h}
    a.st = VarStrides{strides[0], strides[1], strides[8], strides[9], PagedPool{strides[2], strides[3], strides[4]},
                      PagedPool{strides[5], strides[6], strides[7]}};
    a.tb = paged_table(block_size, num_blocks, max_blocks_per_seq);
    const bool fast = varlen_fast_path(dtype, head_dim, heads, kv_heads, block_size, scale, strides,
                                       aligned16(q) && aligned16(k_pool) && aligned16(v_pool) && aligned16(o));
    if (!fast) {
        PLI_REQUIRE(head_dim <= VGEN_MAXD, "pli_attn_varlen_paged: head_dim %d > %d", head_dim, VGEN_MAXD);
        PLI_REQUIRE((int64_t)max_tokens * heads < (1ll << 31), "pli_attn_varlen_paged: grid too large");
        if (dtype == PLI_F32) return launch_varlen_generic<float>(a);
        return dtype == PLI_BF16 ? launch_varlen_generic<bf16_t>(a) : launch_varlen_generic<f16_t>(a);
    }
    const int64_t tiles_upper = varlen_tiles_upper(max_tokens, heads / kv_heads, batch);
    PLI_REQUIRE(tiles_upper * kv_heads < (1ll << 31), "pli_attn_varlen_paged: grid too large");
    if (dtype == PLI_BF16)
        return head_dim == 128 ? launch_varlen<bf16_t, 128>(a, tiles_upper) : launch_varlen<bf16_t, 64>(a, tiles_upper);
    return head_dim == 128 ? launch_varlen<f16_t, 128>(a, tiles_upper) : launch_varlen<f16_t, 64>(a, tiles_upper);
}

extern "C" int pli_kv_append_varlen_paged(const void* k_new, const void* v_new, void* k_pool, void* v_pool,
                                          const int32_t* cu_seqlens_q, const int32_t* block_table,
                                          const int32_t* seq_lens, int batch, int max_tokens, int kv_heads,
                                          int head_dim, int block_size, int num_blocks, int max_blocks_per_seq,
                                          const int64_t* strides, int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(batch >= 0 && max_tokens >= 0 && kv_heads > 0 && head_dim > 0 && num_blocks >= 0 &&
                    max_blocks_per_seq >= 0,
                "pli_kv_append_varlen_paged: bad shape B=%d tokens=%d Hkv=%d D=%d blocks=%d max_blocks_per_seq=%d",
                batch, max_tokens, kv_heads, head_dim, num_blocks, max_blocks_per_seq);
    PLI_REQUIRE(dtype == PLI_F32 || dtype == PLI_F16 || dtype == PLI_BF16,
                "pli_kv_append_varlen_paged: bad dtype %d", dtype);
    PLI_REQUIRE(block_size > 0, "pli_kv_append_varlen_paged: block_size %d must be positive", block_size);
    PLI_REQUIRE((int64_t)max_blocks_per_seq * block_size < (1ll << 31),
                "pli_kv_append_varlen_paged: a table row of %d blocks x %d tokens passes 2^31 keys",
                max_blocks_per_seq, block_size);
    // nothing to append: the (possibly NULL, pli.h) operands are not read
    if (batch == 0 || max_tokens == 0) return PLI_OK;
    PLI_REQUIRE(k_new && v_new && k_pool && v_pool && cu_seqlens_q && block_table && seq_lens && strides,
                "pli_kv_append_varlen_paged: null pointer");
    PLI_REQUIRE(num_blocks > 0 && max_blocks_per_seq > 0,
                "pli_kv_append_varlen_paged: empty pool or table (blocks=%d max_blocks_per_seq=%d)", num_blocks,
                max_blocks_per_seq);
    const int es = dtype == PLI_F32 ? 4 : 2, per16 = 16 / es;
    PLI_REQUIRE(head_dim % per16 == 0 && aligned16(k_new) && aligned16(v_new) && aligned16(k_pool) &&
                    aligned16(v_pool),
                "pli_kv_append_varlen_paged: 16-byte rows (head_dim %% %d) and 16-byte aligned operands required",
                per16);
    for (int i = 0; i < 10; ++i)
        PLI_REQUIRE(strides[i] % per16 == 0, "pli_kv_append_varlen_paged: stride %d not a multiple of %d", i,
                    per16);
    const int cpr = head_dim / per16;
    const int64_t total = (int64_t)max_tokens * kv_heads * cpr;
    PLI_REQUIRE(cdiv64(total, 256) < (1ll << 31), "pli_kv_append_varlen_paged: grid too large");
    // strides[10] = {kn_t, kn_h, k_page, k_token, k_head, v_page, v_token, v_head, vn_t, vn_h}
    const VarAppendStrides st{strides[0] * es, strides[1] * es, strides[8] * es, strides[9] * es,
                              PagedPool{strides[2] * es, strides[3] * es, strides[4] * es},
                              PagedPool{strides[5] * es, strides[6] * es, strides[7] * es}};
    hipLaunchKernelGGL(kv_append_varlen_paged_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0,
                       (hipStream_t)stream, (const char*)k_new, (const char*)v_new, (char*)k_pool, (char*)v_pool,
                       cu_seqlens_q, block_table, seq_lens, batch, max_tokens, kv_heads, cpr, st,
                       paged_table(block_size, num_blocks, max_blocks_per_seq));
    return launch_status("kv_append_varlen_paged");
}

extern "C" int pli_attn_varlen_paged_fp8(const void* q, const void* k_pool, const void* v_pool, void* o,
                                         const int32_t* cu_seqlens_q, const int32_t* block_table,
                                         const int32_t* seq_lens, const float* k_scale, const float* v_scale,
                                         int batch, int max_tokens, int heads, int kv_heads, int head_dim,
                                         int block_size, int num_blocks, int max_blocks_per_seq, int max_kv,
                                         const int64_t* strides, float scale, int causal, int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(batch >= 0 && max_tokens >= 0 && heads > 0 && kv_heads > 0 && head_dim > 0 && num_blocks >= 0 &&
                    max_blocks_per_seq >= 0 && max_kv >= 0,
                "pli_attn_varlen_paged_fp8: bad shape B=%d tokens=%d H=%d Hkv=%d D=%d blocks=%d "
                "max_blocks_per_seq=%d max_kv=%d",
                batch, max_tokens, heads, kv_heads, head_dim, num_blocks, max_blocks_per_seq, max_kv);
    PLI_REQUIRE(heads % kv_heads == 0, "pli_attn_varlen_paged_fp8: heads %d not a multiple of kv_heads %d", heads,
                kv_heads);
    PLI_REQUIRE(dtype == PLI_F32 || dtype == PLI_F16 || dtype == PLI_BF16,
                "pli_attn_varlen_paged_fp8: bad dtype %d", dtype);
    PLI_REQUIRE(std::isfinite(scale), "pli_attn_varlen_paged_fp8: non-finite scale");
    PLI_REQUIRE(block_size > 0, "pli_attn_varlen_paged_fp8: block_size %d must be positive", block_size);
    PLI_REQUIRE((int64_t)max_kv <= (int64_t)max_blocks_per_seq * block_size,
                "pli_attn_varlen_paged_fp8: max_kv %d past the table row (%d blocks of %d tokens)", max_kv,
                max_blocks_per_seq, block_size);
    PLI_REQUIRE((int64_t)max_blocks_per_seq * block_size < (1ll << 31),
                "pli_attn_varlen_paged_fp8: a table row of %d blocks x %d tokens passes 2^31 keys",
                max_blocks_per_seq, block_size);
    // no output rows: the (possibly NULL, pli.h) operands are not read
    if (batch == 0 || max_tokens == 0) return PLI_OK;
    PLI_REQUIRE(q && o && k_pool && v_pool && cu_seqlens_q && block_table && seq_lens && strides,
                "pli_attn_varlen_paged_fp8: null pointer");
    PLI_REQUIRE(num_blocks > 0 && max_blocks_per_seq > 0,
                "pli_attn_varlen_paged_fp8: empty pool or table (blocks=%d max_blocks_per_seq=%d)", num_blocks,
                max_blocks_per_seq);
    VarCall a;
    a.q = q, a.k = k_pool, a.v = v_pool, a.o = o, a.cu = cu_seqlens_q, a.table = block_table, a.seq_lens = seq_lens;
    a.B = batch, a.T = max_tokens, a.H = heads, a.Hkv = kv_heads, a.D = head_dim, a.max_kv = max_kv;
    a.causal = causal != 0, a.scale = scale, a.stream = (hipStream_t)stream;
    // strides[10] as for pli_attn_varlen_paged; the pool strides count 1-byte elements
    a.st = VarStrides{strides[0], strides[1], strides[8], strides[9], PagedPool{strides[2], strides[3], strides[4]},
                      PagedPool{strides[5], strides[6], strides[7]}};
    a.tb = paged_table(block_size, num_blocks, max_blocks_per_seq);
    const Fp8Scales sc{k_scale, v_scale};
    const bool fast = varlen_fast_path_fp8(dtype, head_dim, heads, kv_heads, block_size, scale, strides,
                                           aligned16(q) && aligned16(k_pool) && aligned16(v_pool) && aligned16(o));
    if (!fast) {
        PLI_REQUIRE(head_dim <= VGEN_MAXD, "pli_attn_varlen_paged_fp8: head_dim %d > %d", head_dim, VGEN_MAXD);
        PLI_REQUIRE((int64_t)max_tokens * heads < (1ll << 31), "pli_attn_varlen_paged_fp8: grid too large");
        if (dtype == PLI_F32) return launch_varlen_generic_fp8<float>(a, sc);
        return dtype == PLI_BF16 ? launch_varlen_generic_fp8<bf16_t>(a, sc) : launch_varlen_generic_fp8<f16_t>(a, sc);
    }
    const int64_t tiles_upper = varlen_tiles_upper(max_tokens, heads / kv_heads, batch);
    PLI_REQUIRE(tiles_upper * kv_heads < (1ll << 31), "pli_attn_varlen_paged_fp8: grid too large");
    if (dtype == PLI_BF16)
        return head_dim == 128 ? launch_varlen_fp8<bf16_t, 128>(a, sc, tiles_upper)
                               : launch_varlen_fp8<bf16_t, 64>(a, sc, tiles_upper);
    return head_dim == 128 ? launch_varlen_fp8<f16_t, 128>(a, sc, tiles_upper)
                           : launch_varlen_fp8<f16_t, 64>(a, sc, tiles_upper);
}

extern "C" int pli_kv_append_varlen_paged_fp8(const void* k_new, const void* v_new, void* k_pool, void* v_pool,
                                              const int32_t* cu_seqlens_q, const int32_t* block_table,
                                              const int32_t* seq_lens, const float* k_scale, const float* v_scale,
                                              int batch, int max_tokens, int kv_heads, int head_dim, int block_size,
                                              int num_blocks, int max_blocks_per_seq, const int64_t* strides,
                                              int dtype, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(batch >= 0 && max_tokens >= 0 && kv_heads > 0 && head_dim > 0 && num_blocks >= 0 &&
                    max_blocks_per_seq >= 0,
                "pli_kv_append_varlen_paged_fp8: bad shape B=%d tokens=%d Hkv=%d D=%d blocks=%d "
                "max_blocks_per_seq=%d",
                batch, max_tokens, kv_heads, head_dim, num_blocks, max_blocks_per_seq);
    PLI_REQUIRE(dtype == PLI_F32 || dtype == PLI_F16 || dtype == PLI_BF16,
                "pli_kv_append_varlen_paged_fp8: bad dtype %d", dtype);
    PLI_REQUIRE(block_size > 0, "pli_kv_append_varlen_paged_fp8: block_size %d must be positive", block_size);
    PLI_REQUIRE((int64_t)max_blocks_per_seq * block_size < (1ll << 31),
                "pli_kv_append_varlen_paged_fp8: a table row of %d blocks x %d tokens passes 2^31 keys",
                max_blocks_per_seq, block_size);
    // nothing to append: the (possibly NULL, pli.h) operands are not read
    if (batch == 0 || max_tokens == 0) return PLI_OK;
    PLI_REQUIRE(k_new && v_new && k_pool && v_pool && cu_seqlens_q && block_table && seq_lens && strides,
                "pli_kv_append_varlen_paged_fp8: null pointer");
    PLI_REQUIRE(num_blocks > 0 && max_blocks_per_seq > 0,
                "pli_kv_append_varlen_paged_fp8: empty pool or table (blocks=%d max_blocks_per_seq=%d)", num_blocks,
                max_blocks_per_seq);
    PLI_REQUIRE(head_dim % 8 == 0 && aligned16(k_new) && aligned16(v_new) && aligned16(k_pool) && aligned16(v_pool),
                "pli_kv_append_varlen_paged_fp8: rows of whole 8-element chunks (head_dim %% 8) and 16-byte "
                "aligned operands required");
    for (int i = 0; i < 10; ++i)
        PLI_REQUIRE(strides[i] % 8 == 0, "pli_kv_append_varlen_paged_fp8: stride %d not a multiple of 8", i);
    const int es = dtype == PLI_F32 ? 4 : 2;
    const int cpr = head_dim / 8;
    const int64_t total = (int64_t)max_tokens * kv_heads * cpr;
    PLI_REQUIRE(cdiv64(total, 256) < (1ll << 31), "pli_kv_append_varlen_paged_fp8: grid too large");
    // strides[10] as for pli_kv_append_varlen_paged: the source's in its elements, the pools' in bytes
    const VarAppendStrides st{strides[0] * es, strides[1] * es, strides[8] * es, strides[9] * es,
                              PagedPool{strides[2], strides[3], strides[4]},
                              PagedPool{strides[5], strides[6], strides[7]}};
    const PagedTable tb = paged_table(block_size, num_blocks, max_blocks_per_seq);
    const Fp8Scales sc{k_scale, v_scale};
    const char *kn = (const char*)k_new, *vn = (const char*)v_new;
    char *kp = (char*)k_pool, *vp = (char*)v_pool;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PLI_F32)
        return launch_varlen_append_fp8<float>(kn, vn, kp, vp, cu_seqlens_q, block_table, seq_lens, sc, batch,
                                               max_tokens, kv_heads, cpr, st, tb, s);
    if (dtype == PLI_BF16)
        return launch_varlen_append_fp8<bf16_t>(kn, vn, kp, vp, cu_seqlens_q, block_table, seq_lens, sc, batch,
                                                max_tokens, kv_heads, cpr, st, tb, s);
    return launch_varlen_append_fp8<f16_t>(kn, vn, kp, vp, cu_seqlens_q, block_table, seq_lens, sc, batch,
                                           max_tokens, kv_heads, cpr, st, tb, s);
}

// ---- split-K entry points: the calls above with a caller workspace ----------------
namespace pli {
namespace {

// checks shared by the plan call and the two _ws calls
int varlen_split_args(const char* fn, int batch, int max_tokens, int heads, int kv_heads, int max_kv, int head_dim,
                      int split_keys) {
    PLI_REQUIRE(batch >= 0 && max_tokens >= 0 && heads > 0 && kv_heads > 0 && head_dim > 0 && max_kv >= 0,
                "%s: bad shape B=%d tokens=%d H=%d Hkv=%d D=%d max_kv=%d", fn, batch, max_tokens, heads, kv_heads,
                head_dim, max_kv);
    PLI_REQUIRE(heads % kv_heads == 0, "%s: heads %d not a multiple of kv_heads %d", fn, heads, kv_heads);
    PLI_REQUIRE(split_keys >= 0 && split_keys % VAR_SPAN_UNIT == 0,
                "%s: split_keys %d must be 0 (the plan's choice) or a positive multiple of %d", fn, split_keys,
                VAR_SPAN_UNIT);
    return PLI_OK;
}

int varlen_ws_call(const char* fn, bool fp8, const void* q, const void* k_pool, const void* v_pool, void* o,
                   const int32_t* cu_seqlens_q, const int32_t* block_table, const int32_t* seq_lens,
                   const float* k_scale, const float* v_scale, int batch, int max_tokens, int heads, int kv_heads,
                   int head_dim, int block_size, int num_blocks, int max_blocks_per_seq, int max_kv,
                   const int64_t* strides, float scale, int causal, int dtype, int split_keys, void* workspace,
                   size_t workspace_bytes, void* stream) {
    clear_error();
    PLI_REQUIRE(num_blocks >= 0 && max_blocks_per_seq >= 0, "%s: bad shape blocks=%d max_blocks_per_seq=%d", fn,
                num_blocks, max_blocks_per_seq);
    if (const int rc = varlen_split_args(fn, batch, max_tokens, heads, kv_heads, max_kv, head_dim, split_keys)) return rc;
    PLI_REQUIRE(dtype == PLI_F32 || dtype == PLI_F16 || dtype == PLI_BF16, "%s: bad dtype %d", fn, dtype);
    PLI_REQUIRE(std::isfinite(scale), "%s: non-finite scale", fn);
    PLI_REQUIRE(block_size > 0, "%s: block_size %d must be positive", fn, block_size);
    PLI_REQUIRE((int64_t)max_kv <= (int64_t)max_blocks_per_seq * block_size,
                "%s: max_kv %d past the table row (%d blocks of %d tokens)", fn, max_kv, max_blocks_per_seq,
                block_size);
    PLI_REQUIRE((int64_t)max_blocks_per_seq * block_size < (1ll << 31),
                "%s: a table row of %d blocks x %d tokens passes 2^31 keys", fn, max_blocks_per_seq, block_size);
    // no output rows: the (possibly NULL, pli.h) operands and the workspace are not read
    if (batch == 0 || max_tokens == 0) return PLI_OK;
    PLI_REQUIRE(q && o && k_pool && v_pool && cu_seqlens_q && block_table && seq_lens && strides,
                "%s: null pointer", fn);
    PLI_REQUIRE(num_blocks > 0 && max_blocks_per_seq > 0,
                "%s: empty pool or table (blocks=%d max_blocks_per_seq=%d)", fn, num_blocks, max_blocks_per_seq);
    const bool al = aligned16(q) && aligned16(k_pool) && aligned16(v_pool) && aligned16(o);
    const bool fast = fp8 ? varlen_fast_path_fp8(dtype, head_dim, heads, kv_heads, block_size, scale, strides, al)
                          : varlen_fast_path(dtype, head_dim, heads, kv_heads, block_size, scale, strides, al);
    const VarSplitPlan p = varlen_split_plan(max_tokens, heads, kv_heads, max_kv, head_dim, split_keys);
    // the generic kernels and the one-chunk plan are the existing calls, untouched: the workspace is not used
    if (!fast || p.splits_max == 1)
        return fp8 ? pli_attn_varlen_paged_fp8(q, k_pool, v_pool, o, cu_seqlens_q, block_table, seq_lens, k_scale,
                                               v_scale, batch, max_tokens, heads, kv_heads, head_dim, block_size,
                                               num_blocks, max_blocks_per_seq, max_kv, strides, scale, causal, dtype,
                                               stream)
                   : pli_attn_varlen_paged(q, k_pool, v_pool, o, cu_seqlens_q, block_table, seq_lens, batch,
                                           max_tokens, heads, kv_heads, head_dim, block_size, num_blocks,
                                           max_blocks_per_seq, max_kv, strides, scale, causal, dtype, stream);
    // tiles_upper < 2^32; the second factor is checked first, so the product does not overflow.  The combine's
    // grid is a fraction of max_tokens * heads, bounded as the generic kernel's is.
    const int64_t tiles_upper = varlen_tiles_upper(max_tokens, heads / kv_heads, batch);
    const int64_t per_tile = (int64_t)p.splits_max * kv_heads;
    PLI_REQUIRE(per_tile < (1ll << 31) && tiles_upper * per_tile < (1ll << 31) &&
                    (int64_t)max_tokens * heads < (1ll << 31),
                "%s: grid too large", fn);
    const size_t need = (size_t)p.workspace_bytes;
    PLI_REQUIRE(workspace != nullptr && workspace_bytes >= need, "%s: workspace of %zu bytes needed, %zu given", fn,
                need, workspace ? workspace_bytes : (size_t)0);
    PLI_REQUIRE(aligned16(workspace), "%s: workspace must be 16-byte aligned", fn);
    VarCall a;
    a.q = q, a.k = k_pool, a.v = v_pool, a.o = o, a.cu = cu_seqlens_q, a.table = block_table, a.seq_lens = seq_lens;
    a.B = batch, a.T = max_tokens, a.H = heads, a.Hkv = kv_heads, a.D = head_dim, a.max_kv = max_kv;
    a.causal = causal != 0, a.scale = scale, a.stream = (hipStream_t)stream;
    a.st = VarStrides{strides[0], strides[1], strides[8], strides[9], PagedPool{strides[2], strides[3], strides[4]},
                      PagedPool{strides[5], strides[6], strides[7]}};
    a.tb = paged_table(block_size, num_blocks, max_blocks_per_seq);
    const Fp8Scales scales{k_scale, v_scale};
    const Fp8Scales* sc = fp8 ? &scales : nullptr;
    if (dtype == PLI_BF16)
        return head_dim == 128 ? launch_varlen_split<bf16_t, 128>(a, sc, tiles_upper, p, workspace)
                               : launch_varlen_split<bf16_t, 64>(a, sc, tiles_upper, p, workspace);
    return head_dim == 128 ? launch_varlen_split<f16_t, 128>(a, sc, tiles_upper, p, workspace)
                           : launch_varlen_split<f16_t, 64>(a, sc, tiles_upper, p, workspace);
}

}  // namespace
}  // namespace pli

extern "C" int pli_attn_varlen_paged_split_plan(int batch, int max_tokens, int heads, int kv_heads, int max_kv,
                                                int head_dim, int split_keys, int* span, int* splits_max) {
    using namespace pli;
    clear_error();
    if (const int rc = varlen_split_args("pli_attn_varlen_paged_split_plan", batch, max_tokens, heads, kv_heads,
                                         max_kv, head_dim, split_keys))
        return rc;
    const VarSplitPlan p = varlen_split_plan(max_tokens, heads, kv_heads, max_kv, head_dim, split_keys);
    if (span) *span = p.span;
    if (splits_max) *splits_max = p.splits_max;
    return PLI_OK;
}

extern "C" size_t pli_attn_varlen_paged_workspace_size(int batch, int max_tokens, int heads, int kv_heads,
                                                       int max_kv, int head_dim, int split_keys) {
    using namespace pli;
    if (batch <= 0 || max_tokens <= 0 || heads <= 0 || kv_heads <= 0 || heads % kv_heads || max_kv <= 0 ||
        head_dim <= 0 || split_keys < 0 || split_keys % VAR_SPAN_UNIT)
        return 0;
    return (size_t)varlen_split_plan(max_tokens, heads, kv_heads, max_kv, head_dim, split_keys).workspace_bytes;
}

extern "C" int pli_attn_varlen_paged_ws(const void* q, const void* k_pool, const void* v_pool, void* o,
                                        const int32_t* cu_seqlens_q, const int32_t* block_table,
                                        const int32_t* seq_lens, int batch, int max_tokens, int heads, int kv_heads,
                                        int head_dim, int block_size, int num_blocks, int max_blocks_per_seq,
                                        int max_kv, const int64_t* strides, float scale, int causal, int dtype,
                                        int split_keys, void* workspace, size_t workspace_bytes, void* stream) {
    return pli::varlen_ws_call("pli_attn_varlen_paged_ws", false, q, k_pool, v_pool, o, cu_seqlens_q, block_table,
                               seq_lens, nullptr, nullptr, batch, max_tokens, heads, kv_heads, head_dim, block_size,
                               num_blocks, max_blocks_per_seq, max_kv, strides, scale, causal, dtype, split_keys,
                               workspace, workspace_bytes, stream);
}

extern "C" int pli_attn_varlen_paged_fp8_ws(const void* q, const void* k_pool, const void* v_pool, void* o,
                                            const int32_t* cu_seqlens_q, const int32_t* block_table,
                                            const int32_t* seq_lens, const float* k_scale, const float* v_scale,
                                            int batch, int max_tokens, int heads, int kv_heads, int head_dim,
                                            int block_size, int num_blocks, int max_blocks_per_seq, int max_kv,
                                            const int64_t* strides, float scale, int causal, int dtype,
                                            int split_keys, void* workspace, size_t workspace_bytes, void* stream) {
    return pli::varlen_ws_call("pli_attn_varlen_paged_fp8_ws", true, q, k_pool, v_pool, o, cu_seqlens_q, block_table,
                               seq_lens, k_scale, v_scale, batch, max_tokens, heads, kv_heads, head_dim, block_size,
                               num_blocks, max_blocks_per_seq, max_kv, strides, scale, causal, dtype, split_keys,
                               workspace, workspace_bytes, stream);
}
