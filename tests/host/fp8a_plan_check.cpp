// Host replay of the tile map of gemm_fp8_mx and of the element map of
// quant_rows_fp8 (csrc/gemm_fp8.hip) from csrc/fp8a_plan.h, and the route rule.
// Built by tests/test_fp8a_plan.py with the host compiler (under
// AddressSanitizer + UBSan where available) and driven through stdin, one
// command per line, one JSON object per line out:
//   route m n k ldx8 ldw ldc x8 w8 c
//   mx m n k ldx8 ldw ldc          every staged chunk, fragment read and C store of the launch
//   quant k vec                    every element a workgroup takes of one row
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fp8a_plan.h"

using namespace pli;

struct MxTally {
    int64_t stage_dup = 0, stage_missing = 0, lds_oob = 0, frag_mismatch = 0, frag_count_bad = 0;
    int64_t c_dup = 0, c_missing = 0, c_oob = 0, c_misaligned = 0;
    int64_t src_lo[2] = {INT64_MAX, INT64_MAX}, src_hi[2] = {-1, -1};
};

// one operand image of one K-step: what each wave stages, then what each wave reads
static void replay_image(MxTally& t, int op, int row0, int rows, int64_t ld, int step) {
    std::vector<int64_t> lds(kFp8aImgBytes, -1);       // source byte offset held by each LDS byte
    std::vector<int> staged(kFp8aTM * 8, 0), read(kFp8aTM * 8, 0);
    for (int wave = 0; wave < 4; ++wave)
        for (int i = 0; i < kFp8aPiecesPerWave; ++i)
            for (int lane = 0; lane < 64; ++lane) {
                const int p = fp8a_stage_piece(wave, i);
                const int row = fp8a_stage_row(p, lane), c = fp8a_stage_chunk(p, lane);
                const int dst = fp8a_stage_lds(p, lane);
                const int64_t src = fp8a_src_off(row0, row, rows, ld, step, c);
                t.src_lo[op] = std::min(t.src_lo[op], src);
                t.src_hi[op] = std::max(t.src_hi[op], src + kFp8aChunk - 1);
                if (row < 0 || row >= kFp8aTM || c < 0 || c >= 8) { ++t.stage_dup; continue; }
                if (++staged[row * 8 + c] > 1) ++t.stage_dup;
                if (dst < 0 || dst + kFp8aChunk > kFp8aImgBytes) { ++t.lds_oob; continue; }
                for (int b = 0; b < kFp8aChunk; ++b) {
                    if (lds[dst + b] != -1) ++t.stage_dup;
                    lds[dst + b] = src + b;
                }
            }
    for (int s : staged) t.stage_missing += s == 0;
    // fragment reads: operand 0 (W) is addressed by wn, operand 1 (X) by wm
    for (int wave = 0; wave < 4; ++wave) {
        const int wq = op == 0 ? (wave & 1) : (wave >> 1);
        for (int tt = 0; tt < 2; ++tt)
            for (int kh = 0; kh < 2; ++kh)
                for (int h = 0; h < 2; ++h)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int row = fp8a_frag_row(wq, tt, lane), c = fp8a_frag_chunk(kh, lane, h);
                        const int off = fp8a_frag_lds(row, c);
                        if (off < 0 || off + kFp8aChunk > kFp8aImgBytes) { ++t.lds_oob; continue; }
                        ++read[row * 8 + c];
                        for (int b = 0; b < kFp8aChunk; ++b) {
                            // byte 16 h + b of the lane's operand is k = fp8a_frag_k(kh, lane, 16 h + b) of the
                            // step: the LDS byte must hold that k of the (clamped) row
                            const int k_in_step = fp8a_frag_k(kh, lane, 16 * h + b);
                            const int rr = row0 + row < rows ? row0 + row : rows - 1;
                            const int64_t want = (int64_t)rr * ld + (int64_t)step * kFp8aKStep + k_in_step;
                            if (lds[off + b] != want) ++t.frag_mismatch;
                        }
                    }
    }
    // each staged chunk feeds exactly one operand slot per wave that owns its rows: two waves share a block
    // row (W) or column (X)
    for (int r : read) t.frag_count_bad += r != 2;
}

static void replay_mx(int m, int n, int k, int64_t ldx8, int64_t ldw, int64_t ldc) {
    MxTally t;
    const int tiles_m = fp8a_tiles(m, kFp8aTM), tiles_n = fp8a_tiles(n, kFp8aTN);
    std::vector<uint8_t> stored((size_t)m * n, 0);
    for (int tile = 0; tile < tiles_m * tiles_n; ++tile) {
        const int m0 = fp8a_tile_m(tile, tiles_m, tiles_n) * kFp8aTM, n0 = fp8a_tile_n(tile, tiles_m, tiles_n) * kFp8aTN;
        if (m0 >= m || n0 >= n || m0 < 0 || n0 < 0) ++t.c_oob;
        for (int step = 0; step < k / kFp8aKStep; ++step) {
            replay_image(t, 0, n0, n, ldw, step);
            replay_image(t, 1, m0, m, ldx8, step);
        }
        for (int wave = 0; wave < 4; ++wave)
            for (int mt = 0; mt < 2; ++mt)
                for (int nt = 0; nt < 2; ++nt)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int g = 0; g < 4; ++g) {
                            const int mrow = m0 + fp8a_acc_m(wave >> 1, mt, lane);
                            const int ncol = n0 + fp8a_acc_n(wave & 1, nt, lane, 4 * g);
                            if (mrow >= m || ncol >= n) continue;  // the kernel's mask
                            if (((int64_t)mrow * ldc + ncol) % kFp8aStoreN != 0) ++t.c_misaligned;
                            for (int r = 0; r < 4; ++r) {
                                const int nn = n0 + fp8a_acc_n(wave & 1, nt, lane, 4 * g + r);
                                if (nn != ncol + r || nn >= n) { ++t.c_oob; continue; }
                                if (++stored[(size_t)mrow * n + nn] > 1) ++t.c_dup;
                            }
                        }
    }
    for (uint8_t s : stored) t.c_missing += s == 0;
    printf("{\"stage_dup\": %lld, \"stage_missing\": %lld, \"lds_oob\": %lld, \"frag_mismatch\": %lld, "
           "\"frag_count_bad\": %lld, \"c_dup\": %lld, \"c_missing\": %lld, \"c_oob\": %lld, \"c_misaligned\": %lld, "
           "\"w\": [%lld, %lld], \"x\": [%lld, %lld], \"w_extent\": %lld, \"x_extent\": %lld, \"tiles\": %d, "
           "\"lds_bytes\": %d}\n",
           (long long)t.stage_dup, (long long)t.stage_missing, (long long)t.lds_oob, (long long)t.frag_mismatch,
           (long long)t.frag_count_bad, (long long)t.c_dup, (long long)t.c_missing, (long long)t.c_oob,
           (long long)t.c_misaligned, (long long)t.src_lo[0], (long long)t.src_hi[0], (long long)t.src_lo[1],
           (long long)t.src_hi[1], (long long)((int64_t)(n - 1) * ldw + k), (long long)((int64_t)(m - 1) * ldx8 + k),
           tiles_m * tiles_n, kFp8aLdsBytes);
}

static void replay_quant(int k, bool vec) {
    std::vector<int> taken(k, 0);
    const int items = vec ? k / 8 : k;
    const int trips = fp8a_quant_trips(items);
    int64_t reread = 0, oob = 0;
    for (int t = 0; t < kFp8aQuantThreads; ++t)
        for (int u = 0; u < trips; ++u) {
            const int it = fp8a_quant_item(t, u);
            if (it >= items) continue;  // the kernel's guard
            const bool held = vec && u < kFp8aQuantHeld;
            for (int e = 0; e < (vec ? 8 : 1); ++e) {
                const int i = (vec ? 8 * it : it) + e;
                if (i < 0 || i >= k) { ++oob; continue; }
                ++taken[i];
                reread += !held;
            }
        }
    int64_t missing = 0, dup = 0;
    for (int c : taken) missing += c == 0, dup += c > 1;
    printf("{\"missing\": %lld, \"dup\": %lld, \"oob\": %lld, \"reread\": %lld, \"reg_k\": %d}\n", (long long)missing,
           (long long)dup, (long long)oob, (long long)reread, kFp8aQuantRegK);
}

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        long long a[9] = {0};
        char cmd[16] = {0};
        const int got = sscanf(line, "%15s %lld %lld %lld %lld %lld %lld %lld %lld %lld", cmd, &a[0], &a[1], &a[2], &a[3],
                               &a[4], &a[5], &a[6], &a[7], &a[8]);
        if (got >= 10 && !strcmp(cmd, "route")) {
            const Fp8aCall c{(int)a[0], (int)a[1], (int)a[2], a[3], a[4], a[5], (uintptr_t)a[6], (uintptr_t)a[7],
                             (uintptr_t)a[8]};
            printf("{\"route\": %d, \"mx_ok\": %d}\n", fp8a_route(c), (int)fp8a_mx_ok(c));
        } else if (got >= 7 && !strcmp(cmd, "mx")) {
            const Fp8aCall c{(int)a[0], (int)a[1], (int)a[2], a[3], a[4], a[5], 0, 0, 0};
            if (fp8a_route(c) != FP8A_MX) printf("{\"error\": \"not a gemm_fp8_mx shape\"}\n");
            else replay_mx((int)a[0], (int)a[1], (int)a[2], a[3], a[4], a[5]);
        } else if (got >= 3 && !strcmp(cmd, "quant")) {
            replay_quant((int)a[0], a[1] != 0);
        } else {
            printf("{\"error\": \"bad command\"}\n");
        }
        fflush(stdout);
    }
    return 0;
}
