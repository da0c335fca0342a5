// Self-checking host replay of the W side of gemm_mxfp4_mx (csrc/gemm_mxfp4.hip) from csrc/mxfp4a_plan.h over a
// handful of shapes, and of the route rule of pli_gemm_mxfp4 (tests/test_mxfp4a_plan.py).  Per tile and K-step: every
// 16-byte chunk of the W image is staged once; every e2m1 operand slot reads the nibble of its (row, k); every lane's
// scale byte is w_exp[row][k / 32] of the operand it accompanies; no offset leaves w4 / w_exp / x8 or the LDS stage;
// the 16 lanes of each ds_read_b128 phase of a W fragment fall on 16 distinct slots of a 256-byte line; every byte of
// the e4m3 operand holds the k the instruction pairs it with.  Per launch: every C element is stored once.  The X
// image and the accumulator map are gemm_fp8_mx's (fp8a_plan_check.cpp).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mxfp4a_plan.h"

using namespace pli;

static int bad = 0, checked = 0;
static void expect(bool ok, const char* what, long long a = 0, long long b = 0, long long c = 0) {
    if (++checked, !ok) ++bad, printf("FAIL %s %lld %lld %lld\n", what, a, b, c);
}

// the W image, scale bytes and X sources of one tile and K-step
static void replay_step(int n0, int m0, int m, int n, int k, int64_t ldx8, int64_t ldw, int64_t lds, int step) {
    std::vector<int64_t> img(kMxfp4aWImgBytes, -1);  // source byte offset in w4 held by each LDS byte
    std::vector<int64_t> ximg(kFp8aImgBytes, -1);    // source byte offset in x8 held by each byte of the X image
    std::vector<int> staged(kFp8aTN * kMxfp4aWChunks, 0);
    int64_t wrong = 0, oob = 0;
    const int64_t w_extent = (int64_t)(n - 1) * ldw + k / 2, s_extent = (int64_t)(n - 1) * lds + k / kMxfp4aBlock;
    const int64_t x_extent = (int64_t)(m - 1) * ldx8 + k;
    for (int wave = 0; wave < 4; ++wave) {
        for (int i = 0; i < kMxfp4aWPiecesPerWave; ++i)
            for (int lane = 0; lane < 64; ++lane) {
                const int p = mxfp4a_stage_piece(wave, i), row = mxfp4a_stage_row(p, lane);
                const int c = mxfp4a_stage_chunk(p, lane), dst = mxfp4a_stage_lds(p, lane);
                const int64_t src = mxfp4a_w_off(n0, row, n, ldw, step, c);
                oob += src < 0 || src + kFp8aChunk > w_extent || dst < 0 || dst + kFp8aChunk > kMxfp4aWImgBytes;
                if (row < 0 || row >= kFp8aTN || c < 0 || c >= kMxfp4aWChunks) { ++wrong; continue; }
                ++staged[row * kMxfp4aWChunks + c];
                // the DMA is lane-linear: the slot the read side computes must be the one the lane lands in
                wrong += dst != mxfp4a_frag_lds(row, c);
                for (int b = 0; b < kFp8aChunk && dst >= 0 && dst + kFp8aChunk <= kMxfp4aWImgBytes; ++b) img[dst + b] = src + b;
            }
        for (int i = 0; i < kFp8aPiecesPerWave; ++i)
            for (int lane = 0; lane < 64; ++lane) {
                const int p = fp8a_stage_piece(wave, i);
                const int64_t src = fp8a_src_off(m0, fp8a_stage_row(p, lane), m, ldx8, step, fp8a_stage_chunk(p, lane));
                const int dst = kMxfp4aWImgBytes + fp8a_stage_lds(p, lane);
                oob += src < 0 || src + kFp8aChunk > x_extent || dst < kMxfp4aWImgBytes || dst + kFp8aChunk > kMxfp4aStageBytes;
                for (int b = 0; b < kFp8aChunk && dst >= kMxfp4aWImgBytes && dst + kFp8aChunk <= kMxfp4aStageBytes; ++b)
                    ximg[dst - kMxfp4aWImgBytes + b] = src + b;
            }
    }
    expect(std::count(staged.begin(), staged.end(), 1) == (int64_t)staged.size(), "a W chunk staged never or twice", n0, step);
    for (int wave = 0; wave < 4; ++wave)
        for (int tt = 0; tt < 2; ++tt)
            for (int kh = 0; kh < 2; ++kh) {
                int slots[64];
                for (int lane = 0; lane < 64; ++lane) {
                    const int row = fp8a_frag_row(wave & 1, tt, lane), crow = mxfp4a_w_row(n0, row, n);
                    const int off = mxfp4a_frag_lds(row, mxfp4a_frag_chunk(kh, lane));
                    slots[lane] = off / kFp8aChunk % 16;
                    if (off < 0 || off + kFp8aChunk > kMxfp4aWImgBytes) { ++oob; continue; }
                    for (int j = 0; j < kMxfp4aBlock; ++j) {  // element j: nibble j & 1 of byte j >> 1
                        const int kk = step * kMxfp4aKStep + mxfp4a_frag_k(kh, lane, j);
                        wrong += img[off + (j >> 1)] != (int64_t)crow * ldw + kk / 2 || (j & 1) != (kk & 1);
                    }
                    // the scale operand: byte shift / 8 of the dword at scale_off, selected as byte 0 after the shift
                    const int64_t soff = mxfp4a_scale_off(n0, row, n, lds, step);
                    const int shift = mxfp4a_scale_shift(kh, lane);
                    oob += soff < 0 || soff + 4 > s_extent || soff % 4 != 0;
                    wrong += shift < 0 || shift > 24 || shift % 8 != 0 ||
                             soff + shift / 8 != (int64_t)crow * lds + (step * kMxfp4aKStep + mxfp4a_frag_k(kh, lane, 0)) / kMxfp4aBlock;
                }
                // the X operand: byte b of a lane must hold the k the instruction pairs it with, that of element
                // 16 (lane >> 5) + (b & 15) of the e2m1 operand of lane half b >> 4
                for (int lane = 0; lane < 64; ++lane)
                    for (int b = 0; b < 32; ++b) {
                        const int row = fp8a_frag_row(wave >> 1, tt, lane), xrow = m0 + row < m ? m0 + row : m - 1;
                        const int off = fp8a_frag_lds(row, mxfp4a_xfrag_chunk(kh, lane, b >> 4)) + (b & 15);
                        const int kk = mxfp4a_xfrag_k(kh, lane, b);
                        wrong += kk != mxfp4a_frag_k(kh, 32 * (b >> 4), 16 * (lane >> 5) + (b & 15)) ||
                                 ximg[off] != (int64_t)xrow * ldx8 + step * kMxfp4aKStep + kk;
                    }
                for (int g = 0; g < 64; g += 16) {
                    std::sort(slots + g, slots + g + 16);
                    expect(std::adjacent_find(slots + g, slots + g + 16) == slots + g + 16, "a ds_read_b128 phase repeats a slot", wave, tt, kh);
                }
            }
    expect(wrong == 0, "an operand slot or scale byte of another (row, k)", n0, step, wrong);
    expect(oob == 0, "an offset outside its operand or the LDS stage", n0, step, oob);
}

static void replay_mx(int m, int n, int k, int64_t ldx8, int64_t ldw, int64_t lds, int64_t ldc) {
    const Mxfp4aCall call{m, n, k, ldx8, ldw, lds, ldc, 4096, 8192, 12288, 16384};
    expect(mxfp4a_route(call) == MXFP4A_MX, "not a gemm_mxfp4_mx shape", m, n, k);
    const int tiles_m = fp8a_tiles(m, kFp8aTM), tiles_n = fp8a_tiles(n, kFp8aTN);
    std::vector<uint8_t> stored((size_t)m * n, 0);
    int64_t c_bad = 0;
    for (int tile = 0; tile < tiles_m * tiles_n; ++tile) {
        const int m0 = fp8a_tile_m(tile, tiles_m, tiles_n) * kFp8aTM, n0 = fp8a_tile_n(tile, tiles_m, tiles_n) * kFp8aTN;
        expect(m0 >= 0 && m0 < m && n0 >= 0 && n0 < n, "a tile outside C", tile);
        for (int step = 0; step < k / kMxfp4aKStep; ++step) replay_step(n0, m0, m, n, k, ldx8, ldw, lds, step);
        for (int wave = 0; wave < 4; ++wave)
            for (int mt = 0; mt < 2; ++mt)
                for (int nt = 0; nt < 2; ++nt)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int g = 0; g < 4; ++g) {
                            const int mrow = m0 + fp8a_acc_m(wave >> 1, mt, lane), nloc = fp8a_acc_n(wave & 1, nt, lane, 4 * g);
                            if (mrow >= m || n0 + nloc >= n) continue;  // the kernel's mask
                            c_bad += ((int64_t)mrow * ldc + n0 + nloc) % kFp8aStoreN != 0;
                            for (int r = 0; r < 4; ++r) {
                                c_bad += fp8a_acc_n(wave & 1, nt, lane, 4 * g + r) != nloc + r || n0 + nloc + r >= n;
                                ++stored[(size_t)mrow * n + n0 + nloc + r];
                            }
                        }
    }
    expect(c_bad == 0 && std::count(stored.begin(), stored.end(), 1) == (int64_t)stored.size(), "C not stored exactly once", m, n, k);
}

static int route(Mxfp4aCall a) { return mxfp4a_route(a); }

int main() {
    static_assert(kMxfp4aLdsBytes == 49152 && kMxfp4aWPieces == 8 && kMxfp4aWPiecesPerWave == 2, "the plan's sizes");
    const int S = kMxfp4aStages, KS = kMxfp4aKStep;
    // one step, stages, stages + 1; ragged m and n; several tiles; a short band; padded leading dimensions
    replay_mx(17, 4, KS, KS, KS / 2, 4, 4);
    replay_mx(128, 128, KS * S, KS * S, KS * S / 2, KS * S / 32, 128);
    replay_mx(129, 132, KS * (S + 1), KS * (S + 1) + 16, KS * (S + 1) / 2 + 48, KS * (S + 1) / 32 + 4, 140);
    replay_mx(127, 124, KS, KS + 32, KS / 2 + 16, 8, 128);
    replay_mx(259, 3 * 128 + 4, KS * S, KS * S, KS * S / 2, KS * S / 32 + 12, 3 * 128 + 4);
    replay_mx((kFp8aGroupM + 1) * 128 + 5, 132, KS, KS, KS / 2, 4, 132);

    // the route rule on each side of each condition
    const Mxfp4aCall ok{64, 128, 256, 256, 128, 8, 128, 4096, 8192, 12288, 16384};
    auto with = [&](auto set) { Mxfp4aCall a = ok; set(a); return route(a); };
    const int E = MXFP4A_EMPTY, MX = MXFP4A_MX, G = MXFP4A_GENERIC;
    expect(route(ok) == MX, "route: the base call");
    expect(with([](Mxfp4aCall& a) { a.m = 0; }) == E && with([](Mxfp4aCall& a) { a.n = 0; }) == E && with([](Mxfp4aCall& a) { a.k = 0; }) == E, "route: empty");
    expect(with([](Mxfp4aCall& a) { a.m = 17; }) == MX && with([](Mxfp4aCall& a) { a.m = 16; }) == G, "route: m");
    expect(with([](Mxfp4aCall& a) { a.k = 128; }) == MX && with([](Mxfp4aCall& a) { a.k = 96; }) == G && with([](Mxfp4aCall& a) { a.k = 288; }) == G, "route: k");
    expect(with([](Mxfp4aCall& a) { a.x8 += 16; }) == MX && with([](Mxfp4aCall& a) { a.x8 += 8; }) == G, "route: x8");
    expect(with([](Mxfp4aCall& a) { a.w4 += 16; }) == MX && with([](Mxfp4aCall& a) { a.w4 += 1; }) == G, "route: w4");
    expect(with([](Mxfp4aCall& a) { a.ldx8 = 272; }) == MX && with([](Mxfp4aCall& a) { a.ldx8 = 264; }) == G, "route: ldx8");
    expect(with([](Mxfp4aCall& a) { a.ldw = 144; }) == MX && with([](Mxfp4aCall& a) { a.ldw = 136; }) == G, "route: ldw");
    expect(with([](Mxfp4aCall& a) { a.w_exp += 4; }) == MX && with([](Mxfp4aCall& a) { a.w_exp += 2; }) == G, "route: w_exp");
    expect(with([](Mxfp4aCall& a) { a.lds = 12; }) == MX && with([](Mxfp4aCall& a) { a.lds = 10; }) == G, "route: lds");
    expect(with([](Mxfp4aCall& a) { a.n = a.ldc = 132; }) == MX && with([](Mxfp4aCall& a) { a.n = 130, a.ldc = 132; }) == G, "route: n");
    expect(with([](Mxfp4aCall& a) { a.ldc = 136; }) == MX && with([](Mxfp4aCall& a) { a.ldc = 130; }) == G, "route: ldc");
    expect(with([](Mxfp4aCall& a) { a.c += 8; }) == MX && with([](Mxfp4aCall& a) { a.c += 4; }) == G, "route: c");
    expect(mxfp4a_shape_ok(0) && mxfp4a_shape_ok(96) && !mxfp4a_shape_ok(48), "k % 32");

    printf("%s %d\n", bad ? "FAILED" : "ok", checked);
    return bad != 0;
}
