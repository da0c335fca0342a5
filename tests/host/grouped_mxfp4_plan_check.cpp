// Self-checking host replay of csrc/grouped_mxfp4_plan.h (tests/test_grouped_mxfp4_plan.py): the slot ->
// (expert, slab) scan and, per MC, gemm_grouped_mxfp4's gathered X staging, operand k maps, bounds and stores.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "grouped_mxfp4_plan.h"

using namespace pli;

static int bad = 0, checked = 0;
static void expect(bool ok, const char* what, long long a = 0, long long b = 0, long long c = 0) {
    if (++checked, !ok) ++bad, printf("FAIL %s %lld %lld %lld\n", what, a, b, c);
}

static void replay(const std::vector<int>& counts, int rows_bound, int n, int k, bool use_gather, int64_t ldx8,
                   int64_t ldw, int64_t lds, int64_t ldc) {
    const int E = (int)counts.size(), ks = k / kFp8aKStep, mc = gmx4_mc(rows_bound), stage_bytes = mc * kMxskBlockBytes;
    std::vector<int32_t> offsets(E + 1, 0);
    for (int e = 0; e < E; ++e) offsets[e + 1] = offsets[e] + counts[e];
    const int rows = offsets[E], tokens = rows / 2 + 3;
    std::vector<int32_t> gather(rows);
    for (int r = 0; r < rows; ++r) gather[r] = use_gather ? (int)((r * 7919LL + 3) % (tokens - 1)) : r;
    const Gmx4Call call{E, rows_bound, n, k, ldx8, ldw, lds, ldc, 4096, 8192};
    expect(gmx4_route(call) == GMX4_MX && rows <= rows_bound, "not an MX shape", rows_bound, n, k);
    const int64_t slots = gmx4_slots(rows_bound, E);
    const int64_t x_extent = (int64_t)((use_gather ? tokens : rows) - 1) * ldx8 + k, w_extent = (int64_t)(n - 1) * ldw + k / 2;
    const int64_t s_extent = (int64_t)(n - 1) * lds + k / kMxfp4aBlock, c_extent = (int64_t)(rows_bound - 1) * ldc + n;
    std::vector<int> covered(rows, 0);
    std::vector<uint8_t> stored((size_t)c_extent, 0);
    int64_t wrong = 0, oob = 0, real_slots = 0;
    for (int e = 0; e < E; ++e) real_slots += (counts[e] + kGmx4SlabM - 1) / kGmx4SlabM;
    expect(real_slots <= slots, "more slabs than slots", real_slots, slots);
    for (int slot = 0; slot < slots; ++slot) {
        const Gmx4Slab sl = gmx4_slab(offsets.data(), E, slot);
        expect((sl.expert >= 0) == (slot < real_slots), "a slot past the real count has an expert", slot, sl.expert);
        if (sl.expert < 0) continue;
        const int end = std::min(sl.rbeg + kGmx4SlabM, sl.rend);
        expect(sl.rbeg >= offsets[sl.expert] && sl.rend == offsets[sl.expert + 1] && sl.rbeg < sl.rend && end - sl.rbeg <= kMxskBlockM * mc,
               "a slab outside its expert or above MC blocks", slot, sl.rbeg, sl.rend);
        for (int r = sl.rbeg; r < end; ++r) ++covered[r];
        for (int tn = 0; tn < fp8a_tiles(n, kGmx4TN); ++tn) {
            const int n0 = tn * kGmx4TN;
            for (int step = 0; step < ks; ++step) {
                std::vector<int64_t> ximg(stage_bytes, -1);  // source byte offset in x8 of each LDS byte
                std::vector<int> staged(stage_bytes / kFp8aChunk, 0);
                for (int wave = 0; wave < 4; ++wave)
                    for (int i = 0; i < mc; ++i)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int pc = mxsk_x_piece(wave, i), dst = fp8a_stage_lds(pc, lane);
                            const int row = fp8a_stage_row(pc, lane), ch = fp8a_stage_chunk(pc, lane);
                            const int sr = gmx4_sorted_row(sl.rbeg, row, sl.rend);
                            if (sr < sl.rbeg || sr >= sl.rend) { ++oob; continue; }
                            const int64_t src = gmx4_x_off(gather[sr], ldx8, step, ch);
                            if (dst < 0 || dst + kFp8aChunk > stage_bytes || src < 0 || src + kFp8aChunk > x_extent) { ++oob; continue; }
                            ++staged[dst / kFp8aChunk];
                            wrong += dst != fp8a_frag_lds(row, ch);  // the read side finds the chunk where it landed
                            for (int b = 0; b < kFp8aChunk; ++b) ximg[dst + b] = src + b;
                        }
                expect(std::count(staged.begin(), staged.end(), 1) == (int64_t)staged.size(), "an X piece staged never or twice", mc, step);
                for (int wave = 0; wave < 4; ++wave)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int kh = 0; kh < 2; ++kh) {
                            const int wrow = mxsk_w_row(wave, lane), crow = mxfp4a_w_row(n0, wrow, n);
                            for (int j = 0; j < 32; ++j) {  // element j: nibble j & 1 of byte j >> 1 of the one chunk
                                const int kk = mxfp4a_frag_k(kh, lane, j);
                                const int64_t got = mxsk_w_off(MXSK_E2M1, n0, wrow, n, ldw, step, kh, lane, 0) + (j >> 1);
                                wrong += got != (int64_t)crow * ldw + (step * kFp8aKStep + kk) / 2 || (kk & 1) != (j & 1);
                                oob += got < 0 || got >= w_extent;
                            }
                            const int64_t so = mxfp4a_scale_off(n0, wrow, n, lds, step);
                            oob += so < 0 || so + 4 > s_extent || so % 4 != 0;
                            wrong += so + mxfp4a_scale_shift(kh, lane) / 8 !=
                                     (int64_t)crow * lds + (step * kFp8aKStep + mxfp4a_frag_k(kh, lane, 0)) / kMxfp4aBlock;
                            // the X operand of every m block: byte b holds the k the W element it meets holds
                            for (int blk = 0; blk < mc; ++blk)
                                for (int b = 0; b < 32; ++b) {
                                    const int row = mxsk_x_row(blk, lane);
                                    const int off = fp8a_frag_lds(row, mxsk_x_chunk(MXSK_E2M1, kh, lane, b >> 4)) + (b & 15);
                                    if (off < 0 || off >= stage_bytes) { ++oob; continue; }
                                    const int64_t tok = gather[gmx4_sorted_row(sl.rbeg, row, sl.rend)];
                                    wrong += ximg[off] != tok * ldx8 + step * kFp8aKStep + mxfp4a_xfrag_k(kh, lane, b);
                                }
                        }
            }
            for (int wave = 0; wave < 4; ++wave)
                for (int blk = 0; blk < mc; ++blk)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int r = 0; r < 16; ++r) {
                            const int row = sl.rbeg + mxsk_acc_m(blk, lane), ncol = n0 + mxsk_acc_n(wave, lane, r);
                            if (row >= sl.rend || n0 + mxsk_acc_n(wave, lane, r & ~3) >= n) continue;  // the kernel's mask
                            const int64_t idx = gmx4_c_index(row, ncol, ldc);
                            if (idx < 0 || idx >= c_extent || ncol >= n || row >= end) { ++oob; continue; }
                            wrong += (r & 3) == 0 && idx % 4 != 0;  // the 8-byte store
                            ++stored[idx];
                        }
        }
    }
    expect(std::count(covered.begin(), covered.end(), 1) == rows, "a sorted row in no slab or in two", rows);
    int64_t once = 0;
    for (int r = 0; r < rows_bound; ++r)
        for (int j = 0; j < n; ++j) once += stored[gmx4_c_index(r, j, ldc)] == (r < rows ? 1 : 0);
    expect(once == (int64_t)rows_bound * n && std::count(stored.begin(), stored.end(), 0) == c_extent - (int64_t)rows * n,
           "a C element stored never or twice, or outside the sorted rows", rows, n);
    expect(wrong == 0, "an operand byte, scale byte or store of another (row, k)", rows_bound, n, wrong);
    expect(oob == 0, "an offset outside its operand, the LDS stage or C", rows_bound, n, oob);
}

int main() {
    // each MC, empty / one-row / slab-crossing experts, ragged n, padded leading dimensions, with and without gather
    replay({0, 1, 0, 20}, 21, 144, 256, true, 256, 128, 8, 144);
    replay({1, 33, 0, 30}, 64, 16, 128, true, 128 + 16, 64 + 48, 4 + 4, 16 + 8);
    replay({17, 0, 96, 1}, 114, 144, 384, false, 384, 192, 12, 144);
    replay({0, 1, 33, 130}, 164, 144, 256, true, 256 + 16, 128 + 16, 8 + 4, 144 + 4);
    replay({128, 0, 300, 129}, 600, 128, 128, true, 128, 64, 4, 128);
    printf("%s %d\n", bad ? "FAILED" : "ok", checked);
    return bad != 0;
}
