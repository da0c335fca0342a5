// Self-checking host replay of the index arithmetic of mxfp4w_vec and mxfp4w_smallm (csrc/linear_mxfp4w.hip) from
// csrc/mxfp4w_plan.h over a fixed shape grid, the route of each alignment class of include/pli.h, and the workspace
// sizes (tests/test_mxfp4w_plan.py).  Per launch: every element of every row is consumed exactly once, with its own
// block's scale byte and the X element of its k; every row is stored by one wave; no load leaves its operand.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "mxfp4w_plan.h"

using namespace pli;

static int bad = 0, checked = 0;
static void expect(bool ok, const char* what, long long a = 0, long long b = 0, long long c = 0) {
    if (++checked, !ok) ++bad, printf("FAIL %s %lld %lld %lld\n", what, a, b, c);
}

struct Tally {
    int m, n, k;
    int64_t ldw, lds, ldx;              // padded leading dimensions
    std::vector<uint8_t> seen, stored;  // [n][k] times consumed; [n] times stored
    int64_t hi[3] = {-1, -1, -1}, lo = 0, wrong = 0;  // extent touched of w4 (bytes), w_exp (bytes), x (elements)
    Tally(int m_, int n_, int k_)
        : m(m_), n(n_), k(k_), ldw(k_ / 2 + 48), lds(k_ / 32 + 5), ldx(k_ + 8), seen((size_t)n_ * k_, 0), stored(n_, 0) {}
    void load(int which, int64_t off, int len) { lo = std::min(lo, off), hi[which] = std::max(hi[which], off + len - 1); }
    // element e of the 16-byte load at w_off of `row`, scaled by the byte at s_off, against X element x_elem of row bb
    void consume(int row, int64_t w_off, int64_t s_off, int e, int bb, int64_t x_elem, bool count) {
        const int64_t i = (w_off - (int64_t)row * ldw) * 2 + e;
        if (i < 0 || i >= k || s_off - (int64_t)row * lds != i / kMxfp4Block || x_elem - (int64_t)bb * ldx != i) ++wrong;
        else if (count && ++seen[(size_t)row * k + i] > 1) ++wrong;
    }
    void finish(const char* kind) {
        const int64_t once = std::count(seen.begin(), seen.end(), 1), rows = std::count(stored.begin(), stored.end(), 1);
        expect(once == (int64_t)n * k && wrong == 0 && rows == n, kind, m, n, k);
        expect(lo >= 0 && hi[0] < (int64_t)(n - 1) * ldw + k / 2 && hi[1] < (int64_t)(n - 1) * lds + k / kMxfp4Block &&
                   hi[2] < (int64_t)(m - 1) * ldx + k, "load outside an operand", m, n, k);
    }
};

static void replay_vec(int m, int n, int k, bool swiglu) {
    Tally t(m, n, k);
    const Mxfp4wVecCfg cfg = mxfp4w_vec_cfg(k, swiglu);
    const int cpl = k <= 2048 ? 1 : k <= 4096 ? 2 : 4, nchunks = k / kMxfp4Block;
    expect(cfg.cpl == cpl && cfg.rows * cfg.cpl * (swiglu ? 2 : 1) * 1024 == 8192, "vec cfg: 8 KiB per wave", k, cfg.rows, cfg.cpl);
    for (int wave = 0; wave < mxfp4w_vec_grid(n, cfg.rows) * kMxfp4wVecWaves; ++wave) {
        const int64_t row0 = mxfp4w_vec_row0(wave / kMxfp4wVecWaves, wave % kMxfp4wVecWaves, cfg.rows);
        for (int c0 = 0; row0 < n && c0 < nchunks; c0 += 64 * cfg.cpl)
            for (int lu = 0; lu < 64 * cfg.cpl; ++lu)
                for (int r = 0; r < cfg.rows; ++r) {
                    const int cc = mxfp4w_vec_chunk(c0, lu % 64, lu / 64), ccl = mxfp4w_vec_chunk_clamped(cc, nchunks);
                    const int row = mxfp4w_vec_row(row0, r, n);
                    const int64_t off = mxfp4w_vec_w_off(row, ccl, t.ldw), soff = mxfp4w_vec_s_off(row, ccl, t.lds);
                    t.load(0, off, 16), t.load(1, soff, 1);
                    for (int bb = 0; bb < m && cc < nchunks && row0 + r < n; ++bb) {  // not a masked chunk or clamped row
                        const int64_t xo = mxfp4w_vec_x_off(bb, cc, t.ldx);
                        t.load(2, xo, kMxfp4Block);
                        for (int e = 0; e < kMxfp4Block; ++e) t.consume(row, off, soff, e, bb, xo + e, bb == 0);
                    }
                }
        for (int r = 0; r < cfg.rows && row0 + r < n; ++r) ++t.stored[row0 + r];
    }
    t.finish("vec");
}

static void replay_smallm(int m, int n, int k) {
    Tally t(m, n, k);
    const int nbg = mxfp4w_smallm_nbg(m), kw = mxfp4w_smallm_kw(k), steps = kw / kMxfp4wSmallmWaveStep;
    for (int n0 = 0; n0 < n; n0 += 16) {
        for (int ws = 0; ws < 4 * steps; ++ws)
            for (int lane = 0; lane < 64; ++lane) {
                const int wave = ws / steps, s = ws % steps, row = mxfp4w_smallm_w_row(n0, lane, n);
                // as the kernel: step-0 addresses plus s * 64 bytes / s * 4 scale bytes / s * 128 elements
                const int kb0 = mxfp4w_smallm_k(wave, kw, 0, lane), kb = mxfp4w_smallm_k(wave, kw, s, lane);
                const int64_t off = mxfp4w_smallm_w_off(row, kb0, t.ldw) + (int64_t)s * kMxfp4wSmallmWaveStep / 2;
                const int64_t soff = mxfp4w_smallm_s_off(row, kb0, t.lds) + (int64_t)s * kMxfp4wSmallmWaveStep / kMxfp4Block;
                t.load(0, off, 16), t.load(1, soff, 1);
                // The MFMA pairs k-slot 8 (lane >> 4) + j of this lane's A operand h (W row lane & 15) with the same slot
                // of every lane's B operand in the lane group, so W and X agree when both carry mxfp4w_smallm_k_of there.
                for (int gh = 0; gh < 4 * nbg; ++gh) {
                    const int gi = gh / 4, h = gh % 4, xr = mxfp4w_smallm_x_row(gi, lane, m);
                    const int64_t xo = mxfp4w_smallm_x_off(xr, kb0, 0, t.ldx) + (int64_t)s * kMxfp4wSmallmWaveStep + 8 * h;
                    t.load(2, xo, 8);
                    for (int j = 0; j < 8; ++j)
                        t.consume(row, off, soff, 8 * h + j, xr, xo + j + (mxfp4w_smallm_k_of(kb, h, j) - (kb + 8 * h + j)), gi == 0);
                }
            }
        for (int r = 0; r < 16 && n0 + r < n; ++r) ++t.stored[n0 + r];
    }
    expect(nbg == (m <= 16 ? 1 : m <= 32 ? 2 : m <= 64 ? 4 : 8), "smallm nbg", m, nbg), t.finish("smallm");
}

int main() {
    // vec: one block, a lane tail, both sides of each configuration's range and trip; N with every tail 1 .. ROWS - 1
    for (int k : {32, 32 * 63, 2048, 2080, 4064, 4096, 4128, 8160, 8192, 8224, 16384 + 32 * 65})
        for (int n : {1, 2, 3, 4, 5, 6, 7, 9, 33, 79})
            for (int m : {1, 16}) replay_vec(m, n, k, false), replay_vec(m, n, k, true);
    // smallm: 1, 2, U, U + 1, 2 U + 1 granules; both sides of every batch-group count
    for (int k : {512, 1024, 512 * 8, 512 * 9, 512 * 17})
        for (int m : {2, 15, 16, 17, 32, 33, 64, 65, 128}) replay_smallm(m, m % 2 ? 16 : 48, k);
    // routes, one per class: {m n k ldx ldw ldc w x c bias ws ws_bytes swiglu}; 3072 = 24 * 64 * 2, the widened weight
    const struct { Mxfp4wCall c; int want; } routes[] = {
        {{4, 64, 0, 0, 0, 64, 4096, 8192, 12288, 0, 0, 0, false}, MXFP4W_EMPTY},
        {{kMxfp4wSmallmMinM, 64, 512, 512, 256, 64, 4096, 8192, 12288, 0, 0, 0, false}, MXFP4W_SMALLM},
        {{kMxfp4wSmallmMinM - 1, 64, 512, 512, 256, 64, 4096, 8192, 12288, 0, 0, 0, false}, MXFP4W_VEC},  // one row: the GEMV
        {{4, 64, 256, 256, 128, 64, 4096, 8192, 12288, 0, 0, 0, false}, MXFP4W_VEC},      // k off the 512 granule
        {{16, 24, 512, 512, 256, 24, 4096, 8192, 12288 + 8, 0, 0, 0, false}, MXFP4W_VEC},  // n % 16, C alignment
        {{17, 24, 512, 512, 256, 24, 4096, 8192, 12288, 0, 0, 0, false}, MXFP4W_GENERIC},  // m > 16, no workspace
        {{1, 64, 512, 512, 264, 64, 4097, 8192, 12288, 0, 0, 0, false}, MXFP4W_GENERIC},   // ldw % 16, w4 alignment
        {{17, 24, 64, 64, 32, 24, 4096, 8192, 12288, 0, 1 << 20, 3072, false}, MXFP4W_WIDEN},
        {{17, 24, 64, 64, 32, 24, 4096, 8192, 12288, 0, 1 << 20, 2 * 3072, true}, MXFP4W_WIDEN},
        {{17, 24, 64, 64, 32, 24, 4096, 8192, 12288, 0, 1 << 20, 3072, true}, MXFP4W_BAD_WORKSPACE},
        {{17, 24, 64, 64, 32, 24, 4096, 8192, 12288, 0, (1 << 20) + 8, 3072, false}, MXFP4W_BAD_WORKSPACE},
        {{17, 20, 64, 64, 32, 24, 4096, 8192, 12288, 0, 1 << 20, 3072, false}, MXFP4W_GENERIC},  // n % 8: not pli_gemm's class
    };
    for (const auto& r : routes) expect(mxfp4w_route(r.c) == r.want, "route", &r - routes, mxfp4w_route(r.c), r.want);
    for (int m : {1, 16, 17, 128, 129})
        for (int n : {0, 24, 48})
            for (int k : {0, 48, 64, 512}) {
                const bool none = m <= 16 || (m <= 128 && k % 512 == 0 && n % 16 == 0) || n == 0 || k == 0 || k % 32 != 0;
                const size_t one = none ? 0 : ((size_t)n * k * 2 + 15) / 16 * 16;
                expect(mxfp4w_workspace_size(m, n, k, false) == one && mxfp4w_workspace_size(m, n, k, true) == 2 * one, "workspace size", m, n, k);
            }
    printf("checked %d\n", checked);
    return bad != 0;
}
