// Packed variable-length attention over the paged KV pool as pure C++17 (no
// HIP headers): the tile map, the key range and mask of a tile, the append
// position rule, the address clamps and the fast/generic rule that the
// kernels of varlen_attn.hip use.  Every function carries PLI_HD
// (paged_plan.h), so the same text runs in the kernels and in
// tests/host/varlen_plan_check.cpp (tests/test_varlen_plan.py).  The split-K
// section (chunks of a tile's key range, the workspace rows) is replayed by
// tests/host/varlen_split_check.cpp (tests/test_varlen_split_plan.py).
//
// Operands: q / o packed [max_tokens, heads, head_dim]; cu_seqlens_q int32
// [batch + 1], sequence b owns packed tokens cu[b] .. cu[b+1] - 1; seq_lens[b]
// the kv length AFTER this step's tokens are in the pool; the pools and the
// block table exactly as in paged_plan.h.
#pragma once

#include <cstdint>

#include "paged_plan.h"

namespace pli {

constexpr int VAR_WAVES = 4;                     // waves of a workgroup
constexpr int VAR_ROWS = 16;                     // query rows per wave (one MFMA column block)
constexpr int VAR_BM = VAR_WAVES * VAR_ROWS;     // rows of a tile, all of one kv head
constexpr int VAR_STEP = 32;                     // keys per step (one shared K/V LDS image)
constexpr int VAR_SLICE = 4;                     // sequences per lane in the tile lookup
constexpr int VAR_LANES = 64;

// q_len(b) = max(0, cu[b+1] - cu[b]); a non-monotone cu gives 0, never a
// negative count.
PLI_HD inline int varlen_q_len(int cu0, int cu1) {
    const int64_t d = (int64_t)cu1 - cu0;
    return d < 0 ? 0 : (d > 0x7fffffff ? 0x7fffffff : (int)d);
}
// n_kv(b) = clamp(seq_lens[b], 0, max_kv)
PLI_HD inline int varlen_n_kv(int seq_len, int max_kv) { return paged_seq_len(seq_len, 0, max_kv); }

// ---- tile map ---------------------------------------------------------------
// Row r of a sequence is (token r / G, head hk*G + r % G), G = heads/kv_heads
// dividing 16, so a tile of VAR_BM rows holds tpt = VAR_BM / G whole tokens and
// sequence b owns ceil(q_len(b) / tpt) tiles.  Tiles are numbered sequence by
// sequence; the grid has tiles_upper = ceil(max_tokens*G / VAR_BM) + batch
// workgroups per kv head (each sequence rounds up by less than one tile), and
// a workgroup whose number is past the last tile finds nothing.  A sequence's
// count is capped at tiles_upper: a malformed cu cannot make the running sum
// overflow, and no workgroup below tiles_upper is mapped differently.
PLI_HD inline int64_t varlen_tiles_upper(int max_tokens, int G, int batch) {
    return ((int64_t)max_tokens * G + VAR_BM - 1) / VAR_BM + batch;
}
PLI_HD inline int64_t varlen_seq_tiles(int q_len, int tpt, int64_t cap) {
    const int64_t n = ((int64_t)q_len + tpt - 1) / tpt;
    return n > cap ? cap : n;
}
// The lookup works on slices of VAR_SLICE consecutive sequences: on the device
// lane l of a wave owns slice l of a 256-sequence chunk, the slice totals are
// prefix-summed across the wave, and the one slice that holds workgroup w is
// then walked.  varlen_find_tile below composes the same two functions
// serially.
PLI_HD inline int64_t varlen_slice_tiles(const int32_t* cu, int batch, int first, int tpt, int64_t cap) {
    int64_t n = 0;
    for (int k = 0; k < VAR_SLICE; ++k) {
        const int b = first + k;
        if (b >= 0 && b < batch) n += varlen_seq_tiles(varlen_q_len(cu[b], cu[b + 1]), tpt, cap);
    }
    return n;
}
struct VarTile {
    int b;     // sequence, -1: this workgroup has no tile
    int tile;  // tile of the sequence: its rows start at token tile * tpt
};
PLI_HD inline VarTile varlen_find_in_slice(const int32_t* cu, int batch, int first, int tpt, int64_t cap,
                                           int64_t w_rel) {
    for (int k = 0; k < VAR_SLICE; ++k) {
        const int b = first + k;
        if (b < 0 || b >= batch) break;
        const int64_t n = varlen_seq_tiles(varlen_q_len(cu[b], cu[b + 1]), tpt, cap);
        if (w_rel < n) return VarTile{b, (int)w_rel};
        w_rel -= n;
    }
    return VarTile{-1, 0};
}
PLI_HD inline VarTile varlen_find_tile(const int32_t* cu, int batch, int tpt, int64_t cap, int64_t w) {
    if (w < 0 || w >= cap) return VarTile{-1, 0};
    int64_t before = 0;
    for (int first = 0; first < batch; first += VAR_SLICE) {
        const int64_t n = varlen_slice_tiles(cu, batch, first, tpt, cap);
        if (w < before + n) return varlen_find_in_slice(cu, batch, first, tpt, cap, w - before);
        before += n;
    }
    return VarTile{-1, 0};
}

// Owner of packed token t, for the one-row / one-chunk kernels (generic
// attention, append): the last b with cu[b] <= t by bisection, accepted only
// if cu[b] <= t < cu[b+1]; -1 otherwise (a token no sequence owns, or a
// non-monotone cu the bisection went astray in).  <= 32 steps.
PLI_HD inline int varlen_owner(const int32_t* cu, int batch, int t) {
    int lo = 0, hi = batch;  // first b in [0, batch] with cu[b] > t
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (cu[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    const int b = lo - 1;
    if (b < 0 || b >= batch) return -1;
    return (cu[b] <= t && t < cu[b + 1]) ? b : -1;
}
// rows written: packed tokens [0, min(cu[batch], max_tokens))
PLI_HD inline int varlen_tokens_live(int cu_total, int max_tokens) {
    const int n = cu_total < max_tokens ? cu_total : max_tokens;
    return n < 0 ? 0 : n;
}

// ---- key range and mask -------------------------------------------------------
// Bottom-right causal: token i of a sequence sees keys j <= n_kv - q_len + i
// (and j < n_kv).  varlen_row_limit is the last visible key (-1 or less: none).
PLI_HD inline int varlen_row_limit(int n_kv, int q_len, int i, int causal) {
    const int64_t lim = causal ? (int64_t)n_kv - q_len + i : (int64_t)n_kv - 1;
    const int64_t hi = lim < n_kv - 1 ? lim : (int64_t)n_kv - 1;
    return hi < -1 ? -1 : (int)hi;
}
// A tile walks keys [0, key_end): one past the limit of its last token
// i_last = min(q_len, (tile + 1) * tpt) - 1.
PLI_HD inline int varlen_key_end(int n_kv, int q_len, int tile, int tpt, int causal) {
    const int64_t end = (int64_t)(tile + 1) * tpt;
    const int i_last = (int)(end < q_len ? end : q_len) - 1;
    if (i_last < 0) return 0;
    return varlen_row_limit(n_kv, q_len, i_last, causal) + 1;
}

// ---- split-K ------------------------------------------------------------------
// A tile's key range [0, key_end) is cut into chunks of `span` keys (a multiple
// of 64, so a chunk starts on an even 32-key step): chunk s covers
// [s * span, min((s + 1) * span, key_end)), and a tile has
// chunks = max(1, ceil(key_end / span)) of them -- a tile that sees no key keeps
// one (empty) chunk, whose workgroup writes its rows as 0.  The grid holds
// splits_max = max(1, ceil(max_kv / span)) workgroups per tile and kv head;
// those with s >= chunks leave before any K / V load.  span and splits_max
// depend on host arguments only.
constexpr int VAR_SPAN_UNIT = 2 * VAR_STEP;      // 64: spans are multiples of it
// split_keys == 0: no chunk shorter than VAR_SPAN_MIN keys and no more than VAR_SPLITS_CAP chunks per tile.
// Measured: spans of 2048 - 4096 keys are the best on the long-context shapes, and a
// step whose tiles already fill the device loses to the plain call whenever it is cut at all.
constexpr int VAR_SPAN_MIN = 2048;
constexpr int VAR_SPLITS_CAP = 16;
struct VarSplitPlan {
    int span;                 // keys per chunk
    int splits_max;           // chunks the grid provides per tile; 1: no split, no workspace
    int64_t workspace_bytes;  // splits_max * max_tokens * heads * (head_dim + 2) * 4, or 0
};
// split_keys > 0: the caller's span (the caller checks % 64); 0: the plan's.
// A shape only the generic kernel takes (head_dim, group size) is never split.
inline VarSplitPlan varlen_split_plan(int max_tokens, int heads, int kv_heads, int max_kv, int head_dim,
                                      int split_keys) {
    int64_t span = split_keys;
    if (span <= 0) {
        const int64_t per = ((int64_t)max_kv + VAR_SPLITS_CAP - 1) / VAR_SPLITS_CAP;
        span = (per + VAR_SPAN_UNIT - 1) / VAR_SPAN_UNIT * VAR_SPAN_UNIT;
        if (span < VAR_SPAN_MIN) span = VAR_SPAN_MIN;
    }
    int64_t splits = ((int64_t)max_kv + span - 1) / span;
    const int G = kv_heads > 0 && heads % kv_heads == 0 ? heads / kv_heads : 0;
    const bool mfma_shape = (head_dim == 64 || head_dim == 128) && (G == 1 || G == 2 || G == 4 || G == 8 || G == 16);
    if (splits < 1 || !mfma_shape || max_tokens <= 0) splits = 1;
    VarSplitPlan p;
    p.span = (int)(span > 0x7fffffc0 ? 0x7fffffc0 : span);
    p.splits_max = (int)splits;
    p.workspace_bytes = 0;
    if (splits > 1) {
        // splits <= 2^25, max_tokens and heads < 2^31 each: take the factors one at a time and saturate (no
        // such workspace exists, and the call rejects the grid before it looks at the workspace)
        const int64_t row = ((int64_t)head_dim + 2) * 4, top = INT64_MAX / row;
        int64_t rows = splits * max_tokens;  // < 2^56
        rows = rows > top / heads ? top : rows * heads;
        p.workspace_bytes = rows >= top ? INT64_MAX / 16 * 16 : rows * row;
    }
    return p;
}
PLI_HD inline int varlen_chunks(int key_end, int span) {
    const int64_t n = ((int64_t)key_end + span - 1) / span;
    return n < 1 ? 1 : (int)n;
}
// chunks of tile `tile` of a sequence, from the device tensors' entries: the
// one function the split kernel (per tile) and the combine kernel (per row,
// tile = i / tpt) both call.  key_end <= n_kv <= max_kv, so the count never
// passes splits_max; the clamp only states it.
PLI_HD inline int varlen_tile_chunks(int cu_b, int cu_b1, int seq_len, int max_kv, int tile, int tpt, int causal,
                                     int span, int splits_max) {
    const int n = varlen_chunks(
        varlen_key_end(varlen_n_kv(seq_len, max_kv), varlen_q_len(cu_b, cu_b1), tile, tpt, causal), span);
    return n > splits_max ? splits_max : n;
}
// tile of token i (0 <= i < q_len) of a sequence; tpt >= 4, so it fits an int
PLI_HD inline int varlen_row_tile(int64_t i, int tpt) {
    const int64_t t = i < 0 ? 0 : i / tpt;
    return t > 0x7fffffff ? 0x7fffffff : (int)t;
}
// chunk s of a tile: keys [begin, end), begin a multiple of 64
PLI_HD inline int varlen_chunk_begin(int s, int span) {
    const int64_t k = (int64_t)s * span;
    return k > 0x7fffffc0 ? 0x7fffffc0 : (int)k;
}
PLI_HD inline int varlen_chunk_end(int s, int span, int key_end) {
    const int64_t k = ((int64_t)s + 1) * span;
    return k < key_end ? (int)k : key_end;
}
// fp32 partial row of (chunk s, packed token, head) in the workspace, in rows:
// partial O holds head_dim floats per row, the (m, l) pairs follow all of O.
// The token is a clamped one (varlen_token), s < splits_max.
PLI_HD inline int64_t varlen_partial_row(int s, int tok, int h, int max_tokens, int heads) {
    return ((int64_t)s * max_tokens + tok) * heads + h;
}

// ---- append -------------------------------------------------------------------
// Token i of sequence b goes to logical position seq_lens[b] - q_len(b) + i;
// -1: dropped (negative, or past the table row's cap = max_blocks * block_size).
PLI_HD inline int64_t varlen_append_pos(int seq_len, int q_len, int i, int64_t cap) {
    const int64_t pos = (int64_t)seq_len - q_len + i;
    return (pos < 0 || pos >= cap) ? -1 : pos;
}

// ---- addresses ------------------------------------------------------------------
// Packed token of (sequence start cu_b, token i), clamped into the operand: the
// load address of a row that is masked or never stored is still inside q.
PLI_HD inline int varlen_token(int cu_b, int64_t i, int max_tokens) {
    const int64_t t = (int64_t)cu_b + i;
    return t < 0 ? 0 : (t > max_tokens - 1 ? max_tokens - 1 : (int)t);
}
// A row is stored only if it is a token of the sequence and a live packed row.
PLI_HD inline bool varlen_row_stored(int cu_b, int64_t i, int q_len, int live) {
    const int64_t t = (int64_t)cu_b + i;
    return i >= 0 && i < q_len && t >= 0 && t < live;
}
// Key a load of step row `row` (key0 + row) uses: clamped to the sequence's last
// key, so it is a key the sequence owns; the score is masked afterwards.
PLI_HD inline int varlen_load_key(int key0, int row, int n_kv) {
    const int64_t k = (int64_t)key0 + row;
    const int64_t c = k < n_kv - 1 ? k : (int64_t)n_kv - 1;
    return c < 0 ? 0 : (int)c;
}
// Logical block of 16-key group `grp` of the step at key0 (a multiple of 32):
// with a power-of-two block size >= 16 all 16 keys, clamped as above, lie in
// it, so the table entry is uniform over the lanes that load the group.
PLI_HD inline int varlen_group_block(int key0, int grp, int n_kv, const PagedTable& t) {
    return paged_block_pow2(varlen_load_key(key0, 16 * grp, n_kv), t);
}
// Offset of a K / V row from a raw table entry (clamped into the pool here).
PLI_HD inline int64_t varlen_kv_offset(int entry, int key, int hk, const PagedTable& t, const PagedPool& p) {
    return paged_offset_pow2(paged_clamp_page(entry, t), key, hk, t, p);
}

// ---- fast path or generic ---------------------------------------------------------
// attn_varlen_paged (MFMA) takes bf16 / fp16, head_dim 64 / 128, G in {1, 2, 4,
// 8, 16}, a power-of-two block size >= 16, a positive scale and 16-byte rows:
// every stride a multiple of 8 elements, operands 16-byte aligned.  Everything
// else runs attn_varlen_paged_generic.  strides10 = {q_t, q_h, k_page, k_token,
// k_head, v_page, v_token, v_head, o_t, o_h}.
inline bool varlen_fast_path(int dtype, int head_dim, int heads, int kv_heads, int block_size, float scale,
                             const int64_t* strides10, bool aligned16_operands) {
    if (!(dtype == 1 || dtype == 2)) return false;
    if (!(head_dim == 64 || head_dim == 128)) return false;
    if (kv_heads <= 0 || heads % kv_heads != 0) return false;
    const int G = heads / kv_heads;
    if (!(G == 1 || G == 2 || G == 4 || G == 8 || G == 16)) return false;
    if (block_size < 16 || paged_log2(block_size) < 0) return false;
    if (!(scale > 0.f)) return false;
    for (int i = 0; i < 10; ++i)
        if (strides10[i] % 8 != 0) return false;
    return aligned16_operands;
}
// The same rule for a 1-byte (fp8 e4m3) pool, attn_varlen_paged_fp8: dtype is
// q / o's, whose strides stay multiples of 8 elements; the pool strides
// (strides10[2..7], in elements = bytes) are multiples of 16.
inline bool varlen_fast_path_fp8(int dtype, int head_dim, int heads, int kv_heads, int block_size, float scale,
                                 const int64_t* strides10, bool aligned16_operands) {
    int64_t qo[10];
    for (int i = 0; i < 10; ++i) qo[i] = (i >= 2 && i < 8) ? 0 : strides10[i];
    if (!varlen_fast_path(dtype, head_dim, heads, kv_heads, block_size, scale, qo, aligned16_operands)) return false;
    for (int i = 2; i < 8; ++i)
        if (strides10[i] % 16 != 0) return false;
    return true;
}

}  // namespace pli
