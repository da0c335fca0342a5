// CPU driver for csrc/paged_plan.h and csrc/decode_plan.h (tests/
// test_paged_plan.py builds and runs it; no HIP).  One command per input
// line, one JSON line out:
//   plan B Hkv max_kv rows D            -> chunk, splits, workspace bytes
//   fast dtype D rows bs scale aligned s0 .. s11
//                                       -> the MFMA kernel (true) or the generic one
//   table bs num_blocks max_blocks B e0 e1 ..   (B * max_blocks entries)
//   pool page_stride token_stride head_stride   -> set the state the next two use
//   range b hk n                        -> offsets of keys 0 .. n-1 (and, for a
//                                          power-of-two block size, whether the
//                                          shift-and-mask form agrees)
//   addr b j hk                         -> page, offset of one key
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "paged_plan.h"

int main() {
    using namespace pli;
    std::vector<int32_t> table;
    PagedTable tb{};
    PagedPool pool{};
    int B = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "plan") {
            int64_t b = 0, hkv = 0, rows = 0;
            int max_kv = 0, D = 0;
            in >> b >> hkv >> max_kv >> rows >> D;
            if (!in) return 2;
            const PagedPlan p = plan_paged(b, hkv, max_kv, rows, D);
            std::printf("{\"chunk\": %d, \"splits\": %d, \"ws\": %" PRId64 "}\n", p.chunk, p.splits, p.workspace_bytes);
        } else if (cmd == "fast") {
            int dtype = 0, D = 0, bs = 0, aligned = 0;
            int64_t rows = 0, s[12];
            double scale = 0;
            in >> dtype >> D >> rows >> bs >> scale >> aligned;
            for (auto& x : s) in >> x;
            if (!in) return 2;
            std::printf("{\"fast\": %s}\n", paged_fast_path(dtype, D, rows, bs, (float)scale, s, aligned != 0) ? "true" : "false");
        } else if (cmd == "table") {
            int bs = 0, nb = 0, mb = 0;
            in >> bs >> nb >> mb >> B;
            if (!in || bs <= 0 || nb <= 0 || mb <= 0 || B <= 0) return 2;
            tb = paged_table(bs, nb, mb);
            table.assign((size_t)B * mb, 0);
            for (auto& e : table) in >> e;
            if (!in) return 2;
            std::printf("{\"log2_bs\": %d}\n", tb.log2_bs);
        } else if (cmd == "pool") {
            in >> pool.page_stride >> pool.token_stride >> pool.head_stride;
            if (!in) return 2;
            std::printf("{}\n");
        } else if (cmd == "range" || cmd == "addr") {
            int b = 0, hk = 0, j0 = 0, n = 1;
            if (cmd == "range") in >> b >> hk >> n;
            else in >> b >> j0 >> hk;
            if (!in || table.empty() || b < 0 || b >= B || j0 < 0 || n < 0) return 2;
            bool pow2_agrees = true;
            std::printf("{\"off\": [");
            for (int j = j0; j < j0 + n; ++j) {
                const int64_t off = paged_key_offset(table.data(), b, j, hk, tb, pool);
                if (tb.log2_bs >= 0) {
                    // what attn_decode_paged computes: entry fetched raw, clamped at use
                    const int e = table[(size_t)paged_table_index(b, paged_block_pow2(j, tb), tb)];
                    pow2_agrees = pow2_agrees && paged_offset_pow2(paged_clamp_page(e, tb), j, hk, tb, pool) == off;
                }
                std::printf("%s%" PRId64, j > j0 ? ", " : "", off);
            }
            std::printf("], \"page\": %d, \"pow2_agrees\": %s}\n",
                        paged_page_of(table.data(), b, paged_block_of(j0, tb), tb), pow2_agrees ? "true" : "false");
        } else {
            std::fprintf(stderr, "paged_plan_check: bad command: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
