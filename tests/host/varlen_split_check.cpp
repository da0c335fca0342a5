// CPU driver for the split-K part of csrc/varlen_plan.h
// (tests/test_varlen_split_plan.py builds and runs it; no HIP).  One command
// per input line, one JSON line out:
//   cu B c0 .. cB                      -> set cu_seqlens_q
//   lens B l0 .. l(B-1)                -> set seq_lens
//   table bs num_blocks max_blocks B e0 e1 ..   (B * max_blocks entries)
//   pool page_stride token_stride head_stride
//   plan max_tokens heads kv_heads max_kv head_dim split_keys
//                                      -> span, splits_max, workspace bytes and the two
//                                         tuning constants
//   split max_tokens heads kv_heads D max_kv causal span splits_max
//                                      -> replays attn_varlen_paged_split workgroup by
//                                         workgroup and attn_varlen_paged_combine row by
//                                         row for the state above: every tile's chunks,
//                                         the partial rows written and read, the rows
//                                         stored directly, and every address as a range
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "varlen_plan.h"

namespace {
struct Range {
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    void add(int64_t x) { lo = std::min(lo, x), hi = std::max(hi, x); }
};
void print_range(const char* name, const Range& r, const char* tail) {
    std::printf("\"%s\": [%" PRId64 ", %" PRId64 "]%s", name, r.lo, r.hi, tail);
}
}  // namespace

int main() {
    using namespace pli;
    std::vector<int32_t> cu, lens, table;
    PagedTable tb{};
    PagedPool pool{};
    int B = 0, TB = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "cu") {
            in >> B;
            if (!in || B < 0) return 2;
            cu.assign((size_t)B + 1, 0);
            for (auto& x : cu) in >> x;
            if (!in) return 2;
            std::printf("{}\n");
        } else if (cmd == "lens") {
            int n = 0;
            in >> n;
            if (!in || n < 0) return 2;
            lens.assign((size_t)n, 0);
            for (auto& x : lens) in >> x;
            if (!in) return 2;
            std::printf("{}\n");
        } else if (cmd == "table") {
            int bs = 0, nb = 0, mb = 0;
            in >> bs >> nb >> mb >> TB;
            if (!in || bs <= 0 || nb <= 0 || mb <= 0 || TB <= 0) return 2;
            tb = paged_table(bs, nb, mb);
            table.assign((size_t)TB * mb, 0);
            for (auto& e : table) in >> e;
            if (!in) return 2;
            std::printf("{}\n");
        } else if (cmd == "pool") {
            in >> pool.page_stride >> pool.token_stride >> pool.head_stride;
            if (!in) return 2;
            std::printf("{}\n");
        } else if (cmd == "plan") {
            int max_tokens = 0, heads = 0, kv_heads = 0, max_kv = 0, D = 0, split_keys = 0;
            in >> max_tokens >> heads >> kv_heads >> max_kv >> D >> split_keys;
            if (!in || split_keys < 0 || split_keys % VAR_SPAN_UNIT) return 2;
            const VarSplitPlan p = varlen_split_plan(max_tokens, heads, kv_heads, max_kv, D, split_keys);
            std::printf("{\"span\": %d, \"splits_max\": %d, \"bytes\": %" PRId64 ", \"span_min\": %d, \"splits_cap\": %d}\n",
                        p.span, p.splits_max, p.workspace_bytes, VAR_SPAN_MIN, VAR_SPLITS_CAP);
        } else if (cmd == "split") {
            int max_tokens = 0, heads = 0, kv_heads = 0, D = 0, max_kv = 0, causal = 0, span = 0, splits = 0;
            in >> max_tokens >> heads >> kv_heads >> D >> max_kv >> causal >> span >> splits;
            if (!in || cu.empty() || (int)lens.size() != B || TB != B || tb.log2_bs < 4 || max_tokens <= 0 ||
                kv_heads <= 0 || heads % kv_heads || VAR_BM % (heads / kv_heads) || !(D == 64 || D == 128) ||
                span <= 0 || span % VAR_SPAN_UNIT || splits < 1)
                return 2;
            // the kernels' own arithmetic (varlen_attn.hip)
            const int G = heads / kv_heads, tpt = VAR_BM / G;
            const int CPR = D / 8, RPP = 256 / CPR, PASSES = VAR_STEP / RPP;
            const int64_t upper = varlen_tiles_upper(max_tokens, G, B);
            const int live = varlen_tokens_live(cu[(size_t)B], max_tokens);
            const int64_t partial_rows = (int64_t)splits * max_tokens * heads;
            Range pw, prd, tr, kr;
            std::set<int64_t> written, read, direct, merged;
            int64_t dup = 0, bad_step = 0;
            std::printf("{\"tiles\": [");
            bool first = true;
            // attn_varlen_paged_split: workgroup (w, split, hk)
            for (int64_t w = 0; w < upper; ++w) {
                const VarTile f = varlen_find_tile(cu.data(), B, tpt, upper, w);
                if (f.b < 0) continue;
                const int b = f.b, cu_b = cu[(size_t)b], cu_b1 = cu[(size_t)b + 1], len_b = lens[(size_t)b];
                const int q_len = varlen_q_len(cu_b, cu_b1);
                const int Nk = varlen_n_kv(len_b, max_kv);
                const int key_end = varlen_key_end(Nk, q_len, f.tile, tpt, causal);
                const int chunks = varlen_tile_chunks(cu_b, cu_b1, len_b, max_kv, f.tile, tpt, causal, span, splits);
                std::printf("%s{\"b\": %d, \"tile\": %d, \"key_end\": %d, \"chunks\": %d, \"ranges\": [", first ? "" : ", ",
                            b, f.tile, key_end, chunks);
                first = false;
                for (int s = 0; s < splits; ++s) {
                    if (s >= chunks) continue;  // the workgroup leaves
                    const int k0 = varlen_chunk_begin(s, span), k1 = varlen_chunk_end(s, span, key_end);
                    std::printf("%s[%d, %d]", s ? ", " : "", k0, k1);
                    const int t0 = k0 / VAR_STEP, nsteps = (k1 + VAR_STEP - 1) / VAR_STEP;
                    if (k0 % VAR_SPAN_UNIT || t0 % 2) ++bad_step;
                    for (int hk = 0; hk < kv_heads; ++hk) {
                        for (int r = 0; r < VAR_BM; ++r) {
                            const int64_t qi = (int64_t)f.tile * tpt + r / G;
                            const int hq = hk * G + r % G;
                            const int tok = varlen_token(cu_b, qi, max_tokens);
                            if (!varlen_row_stored(cu_b, qi, q_len, live)) continue;
                            const int64_t orow = (int64_t)tok * heads + hq;
                            if (chunks == 1) {
                                if (!direct.insert(orow).second) ++dup;
                                continue;
                            }
                            const int64_t pr = varlen_partial_row(s, tok, hq, max_tokens, heads);
                            pw.add(pr);
                            if (!written.insert(pr).second) ++dup;
                        }
                        // rows are loaded up to step nsteps + 2, entries fetched up to step nsteps + 3
                        for (int t = t0; t < (t0 < nsteps ? nsteps + 4 : t0); ++t) {
                            for (int tid = 0; tid < 256; ++tid) {
                                const int wave = tid / 64, rrow = tid / CPR;
                                for (int i = 0; i < PASSES; ++i) {
                                    const int grp = (i * RPP + wave * (64 / CPR)) / 16;
                                    const int blk = varlen_group_block(t * VAR_STEP, grp, Nk, tb);
                                    const int64_t ti = paged_table_index(b, blk, tb);
                                    tr.add(ti);
                                    if (t >= nsteps + 3) continue;
                                    const int key = varlen_load_key(t * VAR_STEP, i * RPP + rrow, Nk);
                                    if (paged_block_pow2(key, tb) != blk) return 3;
                                    kr.add(varlen_kv_offset(table[(size_t)ti], key, hk, tb, pool));
                                }
                            }
                        }
                    }
                }
                std::printf("]}");
            }
            // attn_varlen_paged_combine: thread (row, 16-byte chunk); the chunk does not change the addresses' rows
            for (int64_t row = 0; row < (int64_t)max_tokens * heads; ++row) {
                const int h = (int)(row % heads), t = (int)(row / heads);
                if (t >= live) continue;
                const int b = varlen_owner(cu.data(), B, t);
                if (b < 0) continue;
                const int cu_b = cu[(size_t)b], cu_b1 = cu[(size_t)b + 1];
                const int64_t i = (int64_t)t - cu_b;
                if (!varlen_row_stored(cu_b, i, varlen_q_len(cu_b, cu_b1), live)) continue;
                const int chunks = varlen_tile_chunks(cu_b, cu_b1, lens[(size_t)b], max_kv, varlen_row_tile(i, tpt), tpt,
                                                      causal, span, splits);
                if (chunks <= 1) continue;
                merged.insert(row);
                for (int s = 0; s < chunks; ++s) {
                    const int64_t pr = varlen_partial_row(s, t, h, max_tokens, heads);
                    prd.add(pr);
                    read.insert(pr);
                }
            }
            int64_t both = 0;
            for (const int64_t r : direct) both += merged.count(r);
            std::printf("], ");
            print_range("partial_written", pw, ", ");
            print_range("partial_read", prd, ", ");
            print_range("table", tr, ", ");
            print_range("kv", kr, ", ");
            std::printf("\"partial_rows\": %" PRId64 ", \"written\": %zu, \"read\": %zu, \"same_set\": %s, \"dup\": %" PRId64
                        ", \"direct\": %zu, \"merged\": %zu, \"direct_and_merged\": %" PRId64 ", \"bad_step\": %" PRId64 "}\n",
                        partial_rows, written.size(), read.size(), written == read ? "true" : "false", dup, direct.size(),
                        merged.size(), both, bad_step);
        } else {
            std::fprintf(stderr, "varlen_split_check: bad command: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
