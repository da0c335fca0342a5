// Self-checking host replay of csrc/grouped_mxfp4_splitk_plan.h (tests/test_grouped_mxfp4_splitk_plan.py): the split
// rule, its chunks and passes, the workspace size against what is written and read, the gathered X staging and the W offsets.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "grouped_mxfp4_splitk_plan.h"

using namespace pli;

static int bad = 0, checked = 0;
static void expect(bool ok, const char* what, long long a = 0, long long b = 0, long long c = 0) {
    if (++checked, !ok) ++bad, printf("FAIL %s %lld %lld %lld\n", what, a, b, c);
}
template <class F> static void lanes(F f) {  // every (wave, lane) of a workgroup
    for (int t = 0; t < 256; ++t) f(t >> 6, t & 63);
}

static void replay(const std::vector<int>& counts, int rows_bound, int n, int k, bool sw, int splits, bool use_gather,
                   int64_t ldx8, int64_t ldw, int64_t lds) {
    const int E = (int)counts.size(), ks = k / kFp8aKStep, nw = sw ? 2 : 1;
    std::vector<int32_t> offsets(E + 1, 0);
    for (int e = 0; e < E; ++e) offsets[e + 1] = offsets[e] + counts[e];
    const int rows = offsets[E], tokens = rows / 2 + 3;
    std::vector<int32_t> gather(rows);
    for (int r = 0; r < rows; ++r) gather[r] = use_gather ? (int)((r * 7919LL + 3) % (tokens - 1)) : r;
    const size_t bytes = gsk4_workspace_size(E, rows_bound, n, k, sw, splits);
    const Gsk4Plan p = gsk4_plan(true, E, rows_bound, n, k, sw, splits, 4096, bytes);
    expect(p.splits >= 2 && rows <= rows_bound && bytes % 16 == 0, "not a split shape", rows_bound, n, k);
    const int64_t x_extent = (int64_t)((use_gather ? tokens : rows) - 1) * ldx8 + k;
    const int64_t w_extent = (int64_t)(n - 1) * ldw + k / 2, s_extent = (int64_t)(n - 1) * lds + k / kMxfp4aBlock;
    std::vector<uint8_t> written(bytes / 4, 0), read(bytes / 4, 0);
    int64_t wrong = 0, oob = 0, top = -1, once = 0;
    for (int e = 0; e < E; ++e)
        for (int c = 0; c < p.splits && offsets[e] < offsets[e + 1]; ++c)  // an expert without rows: the workgroups leave
            for (int n0 = 0; n0 < n; n0 += kGmx4TN) {
                const int rbeg = offsets[e], rend = offsets[e + 1];
                const int s0 = mxsk_chunk_begin(c, p.per), len = mxsk_chunk_end(c, p.per, ks) - s0;
                int done = 0;
                for (int ps = 0; ps < gsk4_passes(len); ++ps) {
                    const int plen = gsk4_pass_len(len, ps), first = s0 + ps * kGsk4StageSteps;
                    std::vector<int> staged(std::min(std::max(plen, 1), kGsk4StageSteps) * kGsk4ImgBytes / kFp8aChunk, 0);
                    for (int i = 0; i < plen; ++i, ++done)
                        lanes([&](int wave, int lane) {
                            const int row = fp8a_stage_row(wave, lane), ch = fp8a_stage_chunk(wave, lane);
                            const int sr = gmx4_sorted_row(rbeg, row, rend), dst = gsk4_stage_lds(i, wave, lane);
                            const int64_t src = gmx4_x_off(gather[sr], ldx8, first + i, ch);
                            const bool in = sr >= rbeg && sr < rend && sr == std::min(rbeg + row, rend - 1) && dst >= 0 &&
                                            dst + kFp8aChunk <= plen * kGsk4ImgBytes && src >= 0 && src + kFp8aChunk <= x_extent;
                            if (in) ++staged[dst / kFp8aChunk];
                            oob += !in;
                            wrong += dst != gsk4_frag_lds(i, row, ch);  // the read side finds the chunk where it landed
                            const int wrow = mxsk_w_row(wave, lane), step = first + i;
                            const int64_t so = mxfp4a_scale_off(n0, wrow, n, lds, 0) + (int64_t)step * (kMxfp4aKStep / kMxfp4aBlock);
                            oob += so < 0 || so + 4 > s_extent || so % 4 != 0;
                            for (int kh = 0; kh < 2; ++kh) {
                                const int64_t wo = mxsk_w_off(MXSK_E2M1, n0, wrow, n, ldw, 0, kh, lane, 0) + (int64_t)step * kMxfp4aWRowBytes;
                                oob += wo < 0 || wo + kFp8aChunk > w_extent || wo % 16 != 0;
                                wrong += wo != mxsk_w_off(MXSK_E2M1, n0, wrow, n, ldw, step, kh, lane, 0);  // the kernel's base + step
                            }
                        });
                    expect(plen >= 1 && plen <= kGsk4StageSteps && std::count(staged.begin(), staged.end(), 1) == plen * kGsk4ImgBytes / kFp8aChunk,
                           "a pass outside the stage, or an X piece staged never or twice", c, ps, plen);
                }
                expect(done == len && len >= 1, "the passes do not tile the chunk", c, len, done);
                lanes([&](int wave, int lane) {
                    for (int r = 0; r < 16 * nw; ++r) {
                        const int row = rbeg + mxsk_acc_m(0, lane), ncol = n0 + mxsk_acc_n(wave, lane, r & 15);
                        if (row >= rend || row >= rows_bound || n0 + mxsk_acc_n(wave, lane, r & 12) >= n) continue;  // the kernel's mask
                        const int64_t idx = gsk4_ws_index(c, row, r >> 4, ncol, rows_bound, n, nw);
                        if (idx < 0 || idx >= (int64_t)written.size() || ncol >= n) { ++oob; continue; }
                        wrong += (r & 3) == 0 && idx % 4 != 0;  // the 16-byte store
                        ++written[idx];
                        top = std::max(top, idx);
                    }
                });
            }
    for (int64_t i = 0; i < mxsk_reduce_items(rows_bound, n); ++i)  // the reduce: rows of an expert only
        for (int j = 0; j < nw * p.splits * 4 && gsk4_reduce_row(i, n) < offsets[E]; ++j)
            ++read[gsk4_ws_index(j / (4 * nw), gsk4_reduce_row(i, n), j / 4 % nw, gsk4_reduce_col(i, n) + j % 4, rows_bound, n, nw)];
    for (size_t idx = 0; idx < written.size(); ++idx) {
        const bool live = (int)(idx / ((size_t)nw * n) % rows_bound) < rows;  // [c][row][m][col]
        once += written[idx] == live && read[idx] == live;
    }
    expect(once == (int64_t)written.size(), "a partial written, or read by the reduce, never or twice, or outside the sorted rows", rows, n, once);
    // the last sorted row of the last chunk is the largest index: with rows == rows_bound the size is exactly it + 1
    expect(rows < rows_bound ? top < (int64_t)written.size() : (top + 1) * 4 == (int64_t)bytes, "the workspace size is not the largest index + 1", top, bytes);
    expect(wrong == 0, "a staged chunk, W offset or store out of place", rows_bound, n, wrong);
    expect(oob == 0, "an offset outside its operand, the LDS stage or the workspace", rows_bound, n, oob);
}

int main() {
    // the rule at the MoEConfig defaults; for every ks, the rule and forced splits: S chunks tile [0, ks), none empty
    expect(gsk4_splits(8, 2, 4096, 14336, 0) == 16 && gsk4_splits(8, 2, 14336, 4096, 0) == 5, "the rule at the default shapes");
    for (int ks = 1; ks <= 160; ++ks)
        for (int s = 0; s <= 20; ++s) {
            const int S = gsk4_splits(4, 7, 256, ks * 128, s), per = S ? (ks + S - 1) / S : 0;
            bool ok = S >= 1 && S <= kGsk4MaxSplits && (s == 0 || S <= s) && (s != 0 || S == 1 || per >= kGsk4MinSteps);
            for (int c = 0, at = 0; c < S; at = mxsk_chunk_end(c++, per, ks))
                ok = ok && mxsk_chunk_begin(c, per) == at && mxsk_chunk_end(c, per, ks) > at && (c + 1 < S || mxsk_chunk_end(c, per, ks) == ks);
            expect(ok, "S outside the rule, or a chunk empty or out of place", ks, s, S);
        }
    // empty, one-row and full experts, ragged n, padded leading dimensions, with and without gather, plain and SwiGLU,
    // the rule and forced splits, one step per chunk, and chunks of two passes (k 2560 in two chunks: 8 + 2 steps each)
    replay({0, 1, 2, 5}, 11, 144, 640, false, 2, true, 640, 320, 20);
    replay({0, 1, 2, 5}, 11, 144, 640, true, 5, true, 640 + 16, 320 + 48, 20 + 4);
    replay({32, 0, 0, 0}, 32, 16, 2048, true, 0, false, 2048, 1024, 64);
    replay({3, 0, 29, 0}, 32, 256, 2048, false, 3, true, 2048 + 32, 1024 + 16, 64 + 8);
    replay({1, 1, 1, 1}, 4, 144, 2560, true, 2, true, 2560, 1280, 80);
    printf("%s %d\n", bad ? "FAILED" : "ok", checked);
    return bad != 0;
}
