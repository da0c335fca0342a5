// Paged KV-cache decode attention as pure C++17 (no HIP headers): the split-K
// plan of a paged call, the rule that picks the MFMA kernel or the generic
// one, and the address arithmetic the kernels of paged_attn.hip use -- logical
// key j of sequence b -> element offset of its K (or V) row in the pool,
// through the block table.  The functions carry PLI_HD, which is
// __host__ __device__ under hipcc and empty in a host build, so the same text
// runs in the kernels and in tests/host/paged_plan_check.cpp
// (tests/test_paged_plan.py).
//
// Pool layout (ch07/paged_memory.py:38-48): k_cache / v_cache
// [num_blocks, num_layers, block_size, num_heads, head_dim]; a layer view
// k_cache[:, layer] is {page, token, head} strides = {L*bs*H*D, H*D, D}.
#pragma once

#include <cstdint>

#include "decode_plan.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define PLI_HD __host__ __device__
#else
#define PLI_HD
#endif

namespace pli {

// One pool (K or V) as the address function sees it; strides in elements
// (or bytes: the arithmetic does not care, pli_kv_append_paged uses bytes).
struct PagedPool {
    int64_t page_stride, token_stride, head_stride;
};
// The table: block_table int32 [batch, max_blocks_per_seq] of page indices.
struct PagedTable {
    int block_size;
    int log2_bs;  // log2(block_size), -1 when block_size is not a power of two
    int num_blocks;
    int max_blocks_per_seq;
};

PLI_HD inline int paged_log2(int block_size) {
    if (block_size <= 0 || (block_size & (block_size - 1)) != 0) return -1;
    int l = 0;
    while ((1 << l) < block_size) ++l;
    return l;
}

PLI_HD inline PagedTable paged_table(int block_size, int num_blocks, int max_blocks_per_seq) {
    return PagedTable{block_size, paged_log2(block_size), num_blocks, max_blocks_per_seq};
}

// logical block / slot in the block of key j (j >= 0)
PLI_HD inline int paged_block_of(int j, const PagedTable& t) {
    return t.log2_bs >= 0 ? j >> t.log2_bs : j / t.block_size;
}
PLI_HD inline int paged_slot_of(int j, const PagedTable& t) {
    return t.log2_bs >= 0 ? j & (t.block_size - 1) : j % t.block_size;
}

// A table entry as the kernels use it: clamped into [0, num_blocks - 1], so a
// stale or corrupt entry reads the wrong page of the pool, never outside it.
PLI_HD inline int paged_clamp_page(int p, const PagedTable& t) {
    return p < 0 ? 0 : (p > t.num_blocks - 1 ? t.num_blocks - 1 : p);
}

// Where the table holds logical block `block` of sequence b.  The block index
// is clamped into the table row (a prefetch one step past a sequence's last
// block stays inside the table).  The kernels that fetch entries ahead of time
// load table[paged_table_index(..)] raw and clamp the value where they use it.
PLI_HD inline int64_t paged_table_index(int b, int block, const PagedTable& t) {
    const int blk = block < 0 ? 0 : (block > t.max_blocks_per_seq - 1 ? t.max_blocks_per_seq - 1 : block);
    return (int64_t)b * t.max_blocks_per_seq + blk;
}
// Page of logical block `block` of sequence b.
PLI_HD inline int paged_page_of(const int32_t* table, int b, int block, const PagedTable& t) {
    return paged_clamp_page(table[paged_table_index(b, block, t)], t);
}

// Offset of row (page, slot j & (bs - 1), head hk), 64-bit.
PLI_HD inline int64_t paged_offset(int page, int j, int hk, const PagedTable& t, const PagedPool& p) {
    return (int64_t)page * p.page_stride + (int64_t)paged_slot_of(j, t) * p.token_stride +
           (int64_t)hk * p.head_stride;
}

// The same for a power-of-two block size (log2_bs >= 0), shift and mask only:
// what attn_decode_paged computes per row, the page fetched a step ahead.
PLI_HD inline int paged_block_pow2(int j, const PagedTable& t) { return j >> t.log2_bs; }
PLI_HD inline int64_t paged_offset_pow2(int page, int j, int hk, const PagedTable& t, const PagedPool& p) {
    return (int64_t)page * p.page_stride + (int64_t)(j & (t.block_size - 1)) * p.token_stride +
           (int64_t)hk * p.head_stride;
}

// The whole address function: logical key j of sequence b, kv head hk.
PLI_HD inline int64_t paged_key_offset(const int32_t* table, int b, int j, int hk, const PagedTable& t,
                                       const PagedPool& p) {
    return paged_offset(paged_page_of(table, b, paged_block_of(j, t), t), j, hk, t, p);
}

// valid keys of a sequence: clamp(seq_lens[b] + n_kv_add, 0, max_kv)
PLI_HD inline int paged_seq_len(int seq_len, int n_kv_add, int max_kv) {
    const int64_t n = (int64_t)seq_len + n_kv_add;
    return n < 0 ? 0 : (n > max_kv ? max_kv : (int)n);
}

// ---- fast path or generic -------------------------------------------------
// attn_decode_paged (MFMA, paged_attn.hip) takes bf16 / fp16, head_dim 64 /
// 128, at most DEC_MAXM query rows per kv head, a power-of-two block size >=
// 16 (a 32-key step then touches at most two pages), a positive scale (its
// running max is of the raw scores) and 16-byte rows: every stride a multiple
// of 8 elements, operands 16-byte aligned.  Everything else runs
// attn_decode_paged_generic.  dtype: PLI_F32 0, PLI_F16 1, PLI_BF16 2 (pli.h).
inline bool paged_fast_path(int dtype, int head_dim, int64_t rows_per_kv_head, int block_size, float scale,
                            const int64_t* strides12, bool aligned16_operands) {
    if (!(dtype == 1 || dtype == 2)) return false;
    if (!(head_dim == 64 || head_dim == 128)) return false;
    if (rows_per_kv_head < 1 || rows_per_kv_head > DEC_MAXM) return false;
    if (block_size < 16 || paged_log2(block_size) < 0) return false;
    if (!(scale > 0.f)) return false;
    for (int i = 0; i < 12; ++i)
        if (strides12[i] % 8 != 0) return false;
    return aligned16_operands;
}
// The same rule for a 1-byte (fp8 e4m3) pool, attn_decode_paged_fp8: dtype is
// q / o's, whose strides stay multiples of 8 elements; a pool row is loaded
// in 16-byte chunks of 16 codes, so the pool strides (in elements = bytes) are
// multiples of 16.
inline bool paged_fast_path_fp8(int dtype, int head_dim, int64_t rows_per_kv_head, int block_size, float scale,
                                const int64_t* strides12, bool aligned16_operands) {
    int64_t qo[12];
    for (int i = 0; i < 12; ++i) qo[i] = (i >= 3 && i < 9) ? 0 : strides12[i];
    if (!paged_fast_path(dtype, head_dim, rows_per_kv_head, block_size, scale, qo, aligned16_operands)) return false;
    for (int i = 3; i < 9; ++i)
        if (strides12[i] % 16 != 0) return false;
    return true;
}

// ---- split-K plan -----------------------------------------------------------
// The grid and the workspace are sized for max_kv, a host upper bound on every
// sequence's length, by plan_decode (decode_plan.h) -- the rule of the
// contiguous kernel.  workspace: fp32 partial O [bh, splits, rows, D] then
// (m, l) [bh, splits, rows], only when splits > 1.
struct PagedPlan {
    int chunk, splits;
    int64_t workspace_bytes;
};
inline PagedPlan plan_paged(int64_t batch, int64_t kv_heads, int max_kv, int64_t rows_per_kv_head, int head_dim) {
    // no key anywhere: one chunk that runs no step and writes O = 0
    if (max_kv <= 0) return {DEC_QUANT, 1, 0};
    const int64_t bh = batch * kv_heads;
    const DecPlan p = plan_decode(bh, max_kv);
    const int64_t ws = p.splits > 1 ? bh * p.splits * rows_per_kv_head * ((int64_t)head_dim + 2) * 4 : 0;
    return {p.chunk, p.splits, ws};
}

}  // namespace pli
