// Self-checking host replay of csrc/mx_splitk_plan.h (tests/test_mx_splitk_plan.py): the split rule and its chunks for
// every (ks, S) up to ks = 128, and gemm_mx_splitk's index arithmetic for each MC and both weight formats over a
// handful of shapes.  Per workgroup and K-step: every 16-byte piece of the X stage is staged once; every byte of the
// W operand registers is the k the instruction pairs with the X byte it meets, and the scale byte is its block's; no
// offset leaves w / w_exp / x8, the LDS stage or the workspace.  Per launch: every partial element is written once.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mx_splitk_plan.h"

using namespace pli;

static int bad = 0, checked = 0;
static void expect(bool ok, const char* what, long long a = 0, long long b = 0, long long c = 0) {
    if (++checked, !ok) ++bad, printf("FAIL %s %lld %lld %lld\n", what, a, b, c);
}

// chunks of a resolved plan: a partition of [0, ks) into S non-empty runs
static void check_chunks(int ks, int s, int per) {
    std::vector<int> seen(ks, 0);
    bool empty = false;
    for (int c = 0; c < s; ++c) {
        const int b = mxsk_chunk_begin(c, per), e = mxsk_chunk_end(c, per, ks);
        empty |= e <= b;
        for (int i = b; i < e && i < ks; ++i) ++seen[i];
    }
    expect(!empty && std::count(seen.begin(), seen.end(), 1) == ks, "chunks are not a partition", ks, s, per);
}

static void replay(int fmt, int m, int n, int k, int splits, int64_t ldx8, int64_t ldw, int64_t lds) {
    const size_t need = mxsk_workspace_size(m, n, k, splits);
    const MxskPlan p = mxsk_plan(true, m, n, k, splits, 4096, need);
    expect(p.splits >= 2 && need == mxsk_ws_bytes(m, n, p.splits) && p.mc == mxsk_mc(m), "not a split shape", m, n, k);
    const int ks = k / kFp8aKStep, mc = p.mc, stage_bytes = mc * kMxskBlockBytes;
    check_chunks(ks, p.splits, p.per);
    const int wbytes = fmt == MXSK_E2M1 ? k / 2 : k;
    const int64_t w_extent = (int64_t)(n - 1) * ldw + wbytes, x_extent = (int64_t)(m - 1) * ldx8 + k;
    const int64_t s_extent = (int64_t)(n - 1) * lds + k / kMxfp4aBlock;
    std::vector<uint8_t> stored((size_t)p.splits * m * n, 0);
    int64_t wrong = 0, oob = 0;
    for (int tm = 0; tm < p.tiles_m; ++tm)
        for (int tn = 0; tn < p.tiles_n; ++tn)
            for (int c = 0; c < p.splits; ++c) {
                const int m0 = tm * kFp8aTM, n0 = tn * kFp8aTN;
                for (int step = mxsk_chunk_begin(c, p.per); step < mxsk_chunk_end(c, p.per, ks); ++step) {
                    std::vector<int64_t> ximg(stage_bytes, -1);  // source byte offset in x8 of each LDS byte
                    std::vector<int> staged(stage_bytes / kFp8aChunk, 0);
                    for (int wave = 0; wave < 4; ++wave)
                        for (int i = 0; i < mc; ++i)
                            for (int lane = 0; lane < 64; ++lane) {
                                const int pc = mxsk_x_piece(wave, i), dst = fp8a_stage_lds(pc, lane);
                                const int row = fp8a_stage_row(pc, lane), ch = fp8a_stage_chunk(pc, lane);
                                const int64_t src = fp8a_src_off(m0, row, m, ldx8, step, ch);
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
                                // k (inside the instruction's 64) of W register byte / element j of this lane
                                for (int j = 0; j < 32; ++j) {
                                    int64_t got, want;
                                    int kk;  // k inside the K-step
                                    if (fmt == MXSK_E2M1) {  // element j, nibble j & 1 of byte j >> 1 of the one chunk
                                        kk = mxfp4a_frag_k(kh, lane, j);
                                        got = mxsk_w_off(fmt, n0, wrow, n, ldw, step, kh, lane, 0) + (j >> 1);
                                        want = (int64_t)crow * ldw + (step * kFp8aKStep + kk) / 2;
                                        wrong += (kk & 1) != (j & 1);
                                    } else {  // byte j of the two halves: the k of the X byte it meets (fp8a_frag_k)
                                        kk = fp8a_frag_k(kh, lane, j);
                                        got = mxsk_w_off(fmt, n0, wrow, n, ldw, step, kh, lane, j >> 4) + (j & 15);
                                        want = (int64_t)crow * ldw + step * kFp8aKStep + kk;
                                    }
                                    wrong += got != want;
                                    oob += got < 0 || got >= w_extent;
                                }
                                if (fmt == MXSK_E2M1) {
                                    const int64_t so = mxfp4a_scale_off(n0, wrow, n, lds, step);
                                    const int shift = mxfp4a_scale_shift(kh, lane);
                                    oob += so < 0 || so + 4 > s_extent || so % 4 != 0;
                                    wrong += so + shift / 8 != (int64_t)crow * lds + (step * kFp8aKStep + mxfp4a_frag_k(kh, lane, 0)) / kMxfp4aBlock;
                                }
                                // the X operand of every m block: byte b holds the k its W counterpart holds
                                for (int blk = 0; blk < mc; ++blk)
                                    for (int b = 0; b < 32; ++b) {
                                        const int row = mxsk_x_row(blk, lane), xrow = m0 + row < m ? m0 + row : m - 1;
                                        const int off = fp8a_frag_lds(row, mxsk_x_chunk(fmt, kh, lane, b >> 4)) + (b & 15);
                                        if (off < 0 || off >= stage_bytes) { ++oob; continue; }
                                        const int kk = fmt == MXSK_E2M1 ? mxfp4a_xfrag_k(kh, lane, b) : fp8a_frag_k(kh, lane, b);
                                        wrong += ximg[off] != (int64_t)xrow * ldx8 + step * kFp8aKStep + kk;
                                    }
                            }
                }
                for (int wave = 0; wave < 4; ++wave)
                    for (int blk = 0; blk < mc; ++blk)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int r = 0; r < 16; ++r) {
                                const int mrow = m0 + mxsk_acc_m(blk, lane), ncol = n0 + mxsk_acc_n(wave, lane, r);
                                if (mrow >= m || n0 + mxsk_acc_n(wave, lane, r & ~3) >= n) continue;  // the kernel's mask
                                const int64_t idx = mxsk_ws_index(c, mrow, ncol, m, n);
                                if (idx < 0 || (size_t)(idx + 1) * 4 > need || ncol >= n) { ++oob; continue; }
                                wrong += (r & 3) == 0 && idx % 4 != 0;  // the 16-byte store
                                ++stored[idx];
                            }
            }
    expect(wrong == 0, "an operand byte, scale byte or store of another (row, k)", fmt, m, wrong);
    expect(oob == 0, "an offset outside its operand, the LDS stage or the workspace", fmt, m, oob);
    expect(std::count(stored.begin(), stored.end(), 1) == (int64_t)stored.size(), "a partial element written never or twice", fmt, m, n);
}

int main() {
    static_assert(kMxskStages * kMxskMaxMC * kMxskBlockBytes == 49152, "three stages of 128 rows: 48 KiB");
    // 1. every (ks, S): forced splits resolve to a partition without an empty chunk, at most min(ks, 16, S) chunks
    for (int ks = 1; ks <= 128; ++ks)
        for (int s = 0; s <= 20; ++s) {
            const int got = mxsk_splits(64, 128, ks * kFp8aKStep, s);
            expect(got >= 1 && got <= kMxskMaxSplits && got <= ks && (s == 0 || got <= s), "S out of range", ks, s, got);
            if (s == 0) expect(got == 1 || (ks + got - 1) / got >= kMxskMinSteps, "the rule leaves a short chunk", ks, got);
            check_chunks(ks, got, (ks + got - 1) / got);
            expect(mxsk_workspace_size(64, 128, ks * kFp8aKStep, s) == (got >= 2 ? mxsk_ws_bytes(64, 128, got) : 0), "size", ks, s);
        }
    // the rule: the smallest S with tiles * S >= 256, capped; above 128 tiles only a forced count splits
    expect(mxsk_splits(256, 14336, 4096, 0) == 1 && mxsk_splits(256, 14336, 4096, 2) == 2, "the tile cap");
    expect(mxsk_splits(64, 4096, 4096, 0) == 8 && mxsk_splits(64, 14336, 4096, 0) == 3 && mxsk_splits(64, 4096, 14336, 0) == 8 &&
           mxsk_splits(256, 8192, 8192, 0) == 2 && mxsk_splits(128, 128, 16384, 0) == 16 && mxsk_splits(64, 4096, 512, 0) == 1, "the rule");
    // where the shape rules the route out
    expect(mxsk_splits(16, 4096, 4096, 0) == 0 && mxsk_splits(257, 4096, 4096, 0) == 0 && mxsk_splits(64, 4098, 4096, 0) == 0 &&
           mxsk_splits(64, 4096, 4160, 0) == 0 && mxsk_splits(64, 4096, 4096, -1) == 0 && mxsk_splits(17, 4, 1024, 2) == 2, "shape conditions");
    // the pointer conditions of the plan
    const size_t need = mxsk_workspace_size(64, 256, 1024, 2);
    expect(need == 2u * 64 * 256 * 4 && mxsk_plan(true, 64, 256, 1024, 2, 4096, need).splits == 2 &&
           mxsk_plan(true, 64, 256, 1024, 2, 4096, need - 1).splits == 1 && mxsk_plan(true, 64, 256, 1024, 2, 0, need).splits == 1 &&
           mxsk_plan(true, 64, 256, 1024, 2, 4104, need).splits == 1 && mxsk_plan(false, 64, 256, 1024, 2, 4096, need).splits == 1 &&
           mxsk_plan(true, 64, 256, 1024, 1, 4096, need).splits == 1, "plan conditions");
    // 2., 3. each MC, ragged m and n, two m tiles, unequal chunks, padded leading dimensions, both formats
    for (int fmt : {MXSK_E4M3, MXSK_E2M1}) {
        const int d = fmt == MXSK_E2M1 ? 2 : 1;
        replay(fmt, 17, 128, 256, 2, 256, 256 / d, 8);
        replay(fmt, 33, 132, 640, 3, 640 + 16, 640 / d + 48, 20 + 4);
        replay(fmt, 65, 260, 640, 5, 640, 640 / d, 20);
        replay(fmt, 97, 4, 1024, 3, 1024, 1024 / d + 16, 32);
        replay(fmt, 129, 132, 384, 2, 384 + 32, 384 / d, 12 + 8);
        replay(fmt, 256, 128, 2048, 0, 2048, 2048 / d, 64);
    }
    printf("%s %d\n", bad ? "FAILED" : "ok", checked);
    return bad != 0;
}
