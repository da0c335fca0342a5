// CPU driver for csrc/varlen_plan.h (tests/test_varlen_plan.py builds and
// runs it; no HIP).  One command per input line, one JSON line out:
//   cu B c0 .. cB                      -> set cu_seqlens_q
//   lens B l0 .. l(B-1)                -> set seq_lens
//   table bs num_blocks max_blocks B e0 e1 ..   (B * max_blocks entries)
//   pool page_stride token_stride head_stride
//   tiles max_tokens G                 -> tiles_upper and (b, tile) of workgroups
//                                         0 .. tiles_upper + 2
//   owner t0 t1                        -> varlen_owner of tokens t0 .. t1-1
//   mask n_kv q_len G causal           -> key_end per tile, last visible key per token
//   append seq_len q_len cap           -> position per token (-1: dropped)
//   kvoff entry key hk                 -> varlen_kv_offset
//   sweep max_tokens heads kv_heads D max_kv causal q_t q_h
//                                      -> every address attn_varlen_paged forms for the
//                                         state above, as ranges, and the rows it stores
//   fast dtype D heads kv_heads bs scale aligned s0 .. s9
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
        } else if (cmd == "tiles") {
            int max_tokens = 0, G = 0;
            in >> max_tokens >> G;
            if (!in || G <= 0 || VAR_BM % G || cu.empty()) return 2;
            const int64_t upper = varlen_tiles_upper(max_tokens, G, B);
            std::printf("{\"upper\": %" PRId64 ", \"map\": [", upper);
            for (int64_t w = 0; w < upper + 3; ++w) {
                const VarTile t = varlen_find_tile(cu.data(), B, VAR_BM / G, upper, w);
                std::printf("%s[%d, %d]", w ? ", " : "", t.b, t.tile);
            }
            std::printf("]}\n");
        } else if (cmd == "owner") {
            int t0 = 0, t1 = 0;
            in >> t0 >> t1;
            if (!in || cu.empty()) return 2;
            std::printf("{\"owner\": [");
            for (int t = t0; t < t1; ++t) std::printf("%s%d", t > t0 ? ", " : "", varlen_owner(cu.data(), B, t));
            std::printf("]}\n");
        } else if (cmd == "mask") {
            int n_kv = 0, q_len = 0, G = 0, causal = 0;
            in >> n_kv >> q_len >> G >> causal;
            if (!in || G <= 0 || VAR_BM % G) return 2;
            const int tpt = VAR_BM / G;
            std::printf("{\"key_end\": [");
            for (int t = 0; t * tpt < q_len; ++t)
                std::printf("%s%d", t ? ", " : "", varlen_key_end(n_kv, q_len, t, tpt, causal));
            std::printf("], \"limit\": [");
            for (int i = 0; i < q_len; ++i) std::printf("%s%d", i ? ", " : "", varlen_row_limit(n_kv, q_len, i, causal));
            std::printf("]}\n");
        } else if (cmd == "append") {
            int seq_len = 0, q_len = 0;
            int64_t cap = 0;
            in >> seq_len >> q_len >> cap;
            if (!in) return 2;
            std::printf("{\"pos\": [");
            for (int i = 0; i < q_len; ++i)
                std::printf("%s%" PRId64, i ? ", " : "", varlen_append_pos(seq_len, q_len, i, cap));
            std::printf("]}\n");
        } else if (cmd == "kvoff") {
            int entry = 0, key = 0, hk = 0;
            in >> entry >> key >> hk;
            if (!in || tb.log2_bs < 0) return 2;
            std::printf("{\"off\": %" PRId64 "}\n", varlen_kv_offset(entry, key, hk, tb, pool));
        } else if (cmd == "sweep") {
            int max_tokens = 0, heads = 0, kv_heads = 0, D = 0, max_kv = 0, causal = 0;
            int64_t q_t = 0, q_h = 0;
            in >> max_tokens >> heads >> kv_heads >> D >> max_kv >> causal >> q_t >> q_h;
            if (!in || cu.empty() || (int)lens.size() != B || TB != B || tb.log2_bs < 4 || max_tokens <= 0 ||
                kv_heads <= 0 || heads % kv_heads || VAR_BM % (heads / kv_heads) || !(D == 64 || D == 128))
                return 2;
            // the kernel's own arithmetic, thread by thread (varlen_attn.hip)
            const int G = heads / kv_heads, tpt = VAR_BM / G;
            const int CPR = D / 8, RPP = 256 / CPR, PASSES = VAR_STEP / RPP;
            const int64_t upper = varlen_tiles_upper(max_tokens, G, B);
            const int live = varlen_tokens_live(cu[(size_t)B], max_tokens);
            Range qr, tr, kr, sr;
            std::set<std::pair<int, int>> stored;
            int64_t steps = 0, dup = 0, visible_past_end = 0;
            for (int64_t w = 0; w < upper; ++w) {
                const VarTile f = varlen_find_tile(cu.data(), B, tpt, upper, w);
                if (f.b < 0) continue;
                const int b = f.b, cu_b = cu[(size_t)b];
                const int q_len = varlen_q_len(cu_b, cu[(size_t)b + 1]);
                const int Nk = varlen_n_kv(lens[(size_t)b], max_kv);
                const int key_end = varlen_key_end(Nk, q_len, f.tile, tpt, causal);
                const int nsteps = (key_end + VAR_STEP - 1) / VAR_STEP;
                steps += nsteps;
                for (int hk = 0; hk < kv_heads; ++hk) {
                    for (int r = 0; r < VAR_BM; ++r) {
                        const int64_t qi = (int64_t)f.tile * tpt + r / G;
                        const int hq = hk * G + r % G;
                        const int tok = varlen_token(cu_b, qi, max_tokens);
                        qr.add((int64_t)tok * q_t + (int64_t)hq * q_h);
                        if (qi < q_len && varlen_row_limit(Nk, q_len, (int)qi, causal) >= key_end) ++visible_past_end;
                        if (varlen_row_stored(cu_b, qi, q_len, live)) {
                            sr.add(tok);
                            if (!stored.insert({tok, hq}).second) ++dup;
                        }
                    }
                    // rows are loaded up to step nsteps + 2, entries fetched up to step nsteps + 3
                    for (int t = 0; t < (nsteps ? nsteps + 4 : 0); ++t) {
                        for (int tid = 0; tid < 256; ++tid) {
                            const int wave = tid / 64, rrow = tid / CPR;
                            for (int i = 0; i < PASSES; ++i) {
                                const int grp = (i * RPP + wave * (64 / CPR)) / 16;
                                const int blk = varlen_group_block(t * VAR_STEP, grp, Nk, tb);
                                const int64_t ti = paged_table_index(b, blk, tb);
                                tr.add(ti);
                                if (t >= nsteps + 3) continue;
                                const int key = varlen_load_key(t * VAR_STEP, i * RPP + rrow, Nk);
                                // the uniform entry is the entry of this lane's own (clamped) key
                                if (paged_block_pow2(key, tb) != blk) return 3;
                                const int64_t off = varlen_kv_offset(table[(size_t)ti], key, hk, tb, pool);
                                kr.add(off);
                            }
                        }
                    }
                }
            }
            std::printf("{");
            print_range("q", qr, ", ");
            print_range("table", tr, ", ");
            print_range("kv", kr, ", ");
            print_range("stored", sr, ", ");
            std::printf("\"rows\": %zu, \"dup\": %" PRId64 ", \"steps\": %" PRId64 ", \"visible_past_end\": %" PRId64 "}\n",
                        stored.size(), dup, steps, visible_past_end);
        } else if (cmd == "fast") {
            int dtype = 0, D = 0, heads = 0, kv_heads = 0, bs = 0, aligned = 0;
            int64_t s[10];
            double scale = 0;
            in >> dtype >> D >> heads >> kv_heads >> bs >> scale >> aligned;
            for (auto& x : s) in >> x;
            if (!in) return 2;
            std::printf("{\"fast\": %s}\n",
                        varlen_fast_path(dtype, D, heads, kv_heads, bs, (float)scale, s, aligned != 0) ? "true" : "false");
        } else {
            std::fprintf(stderr, "varlen_plan_check: bad command: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
