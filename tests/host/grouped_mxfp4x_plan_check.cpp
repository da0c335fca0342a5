// Self-checking host replay of csrc/grouped_mxfp4x_plan.h (tests/test_grouped_mxfp4x_plan.py): the route rule at its
// boundaries, gemm_grouped_mxfp4_a4's gathered X code and scale-dword sources, and the two / three-image stage layout.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "grouped_mxfp4x_plan.h"

using namespace pli;
using C = Gmx4xCall;

static int bad = 0, checked = 0;
static void expect(bool ok, const char* what, long long a = 0, long long b = 0) {
    if (++checked, !ok) ++bad, printf("FAIL %s %lld %lld\n", what, a, b);
}
template <class M> static int with(C a, M member, long long value) {  // the route with one field set
    a.*member = (std::remove_reference_t<decltype(a.*member)>)value;
    return gmx4x_route(a);
}

static void routes() {
    const C ok{8, 4096, 144, 768, 384, 24, 384, 24, 144, 4096, 8192, 16384};
    const int top = 128 * (kGmx4MaxSlots - ok.experts);  // the most rows whose slots fit the grid
    expect(gmx4x_route(ok) == GMX4X_MX && with(ok, &C::rows_bound, 0) == GMX4X_EMPTY && with(ok, &C::n, 0) == GMX4X_EMPTY, "base, empty");
#define EDGE(F, OUT, IN) {with(ok, &C::F, OUT), with(ok, &C::F, IN)}  // one step outside the rule, the nearest value inside
    const int edges[][2] = {EDGE(k, 0, 256), EDGE(k, 640, 512), EDGE(n, 136, 16), EDGE(x4, 4104, 4112), EDGE(ldx4, 392, 400),
                            EDGE(ldw, 392, 400), EDGE(x_exp, 8194, 8196), EDGE(ldxs, 26, 28), EDGE(lds, 26, 28), EDGE(ldc, 146, 148),
                            EDGE(c, 16388, 16392), EDGE(rows_bound, top + 1, top)};
    for (const auto& e : edges) expect(e[0] == GMX4X_GENERIC && e[1] == GMX4X_MX, "the route at a boundary of the rule", &e - edges);
}

// every (image row, chunk) of the X image and every fragment row's scale dwords, per slab and K-step
static void sources(const std::vector<int>& counts, int k, bool use_gather, int64_t ldx4, int64_t ldxs) {
    const int E = (int)counts.size(), ks = k / kMxfp4xKStep;
    std::vector<int32_t> offsets(E + 1, 0);
    for (int e = 0; e < E; ++e) offsets[e + 1] = offsets[e] + counts[e];
    const int rows = offsets[E], tokens = use_gather ? rows / 2 + 3 : rows;
    std::vector<int32_t> gather(rows);
    for (int r = 0; r < rows; ++r) gather[r] = use_gather ? (int)((r * 7919LL + 3) % (tokens - 1)) : r;
    int64_t wrong = 0, oob = 0;
    for (int slot = 0; slot < gmx4_slots(rows, E); ++slot) {
        const Gmx4Slab sl = gmx4_slab(offsets.data(), E, slot);
        for (int step = 0; sl.expert >= 0 && step < ks; ++step) {
            std::vector<int64_t> img(kFp8aImgBytes / kFp8aChunk, -1);  // source offset in x4 of each chunk of the X image
            for (int wave = 0; wave < 4; ++wave)
                for (int i = 0; i < kFp8aPiecesPerWave; ++i)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int p = fp8a_stage_piece(wave, i), row = fp8a_stage_row(p, lane), ch = fp8a_stage_chunk(p, lane);
                        const int sr = gmx4_sorted_row(sl.rbeg, row, sl.rend), dst = fp8a_stage_lds(p, lane);
                        if (sr < sl.rbeg || sr >= sl.rend || dst < 0 || dst + kFp8aChunk > kFp8aImgBytes) { ++oob; continue; }
                        const int64_t tok = gather[sr], src = gmx4x_x_off((int)tok, ldx4, step, ch);
                        oob += src < tok * ldx4 || src + kFp8aChunk > tok * ldx4 + k / 2;  // inside its token's row
                        wrong += dst != fp8a_frag_lds(row, ch) || dst % kFp8aChunk || img[dst / kFp8aChunk] != -1;  // staged once
                        img[dst / kFp8aChunk] = src;
                    }
            for (int wm = 0; wm < 2; ++wm)
                for (int tt = 0; tt < 2; ++tt)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int q = 0; q < kMxfp4xQuarters; ++q) {
                            // the operand's bytes are the codes of k-quarter q of the row's token, its scale byte their block's
                            const int row = fp8a_frag_row(wm, tt, lane);
                            const int64_t tok = gather[gmx4_sorted_row(sl.rbeg, row, sl.rend)];
                            wrong += img[fp8a_frag_lds(row, mxfp4x_frag_chunk(q, lane)) / kFp8aChunk] != tok * ldx4 + (step * kMxfp4xKStep + mxfp4x_frag_k(q, lane, 0)) / 2;
                            const int64_t so = gmx4x_xscale_off((int)tok, ldxs, step, mxfp4x_scale_dword(q));
                            oob += so < tok * ldxs || so + 4 > tok * ldxs + k / kMxfp4aBlock || so % 4 != 0;
                            wrong += so + mxfp4x_scale_shift(q, lane) / 8 != tok * ldxs + step * kMxfp4xStepScales + mxfp4x_scale_block(q, lane);
                        }
        }
    }
    expect(wrong == 0, "an X byte or scale byte of another (token, k), or an image byte staged never or twice", k, wrong);
    expect(oob == 0, "an offset outside its token's row or the image", k, oob);
}

int main() {
    routes();
    sources({0, 1, 33, 130}, 768, true, 384, 24);            // empty expert, ragged last slab, gathered
    sources({128, 0, 300, 5}, 256, false, 128 + 16, 8 + 4);  // exact slab, slab crossing, identity gather, padded rows
    for (bool sw : {false, true}) {  // the stage layout
        std::vector<int> owner(gmx4x_lds_bytes(sw), 0);
        for (int step = 0; step < kMxfp4xStages; ++step)
            for (int image = 0; image <= gmx4x_w_images(sw); ++image)  // the W images, then X
                for (int b = 0; b < kFp8aImgBytes; ++b)
                    ++owner[gmx4x_stage_off(sw, step) + (image < gmx4x_w_images(sw) ? gmx4x_w_img_off(image) : gmx4x_x_img_off(sw)) + b];
        expect(std::count(owner.begin(), owner.end(), 1) == (long long)owner.size() && gmx4x_lds_bytes(sw) <= kGmx4xLdsLimit &&
                   gmx4x_stage_off(sw, kMxfp4xStages) == 0, "images overlap or leave a gap, LDS above the limit, or no stage wrap", sw);
    }
    printf("%s %d\n", bad ? "FAILED" : "ok", checked);
    return bad != 0;
}
