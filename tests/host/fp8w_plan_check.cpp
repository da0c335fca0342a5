// Host replay of the index arithmetic of linear_fp8w_vec and
// linear_fp8w_smallm (csrc/linear_fp8w.hip) from csrc/fp8w_plan.h, and the
// route rule.  Built by tests/test_fp8w_plan.py with the host compiler (under
// AddressSanitizer + UBSan where available) and driven through stdin, one
// command per line, one JSON object per line out:
//   vec m n k ldw ldx swiglu       every load and consumed code of the launch
//   smallm m n k ldw ldx           the same for the MFMA kernel
//   route m n k ldx ldw ldc w x c bias ws ws_bytes swiglu
//   wsize m n k swiglu
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fp8w_plan.h"

using namespace pli;

struct Tally {
    int m, n, k;
    int64_t ldw, ldx;
    std::vector<uint8_t> seen;  // [n][k]: times code (row, i) was consumed
    int64_t w_lo = INT64_MAX, w_hi = -1, x_lo = INT64_MAX, x_hi = -1;
    int64_t xk_mismatch = 0, stored_rows_bad = 0, dup = 0;
    std::vector<uint8_t> stored;  // [n]: rows whose outputs a wave stores
    Tally(int m_, int n_, int k_, int64_t ldw_, int64_t ldx_)
        : m(m_), n(n_), k(k_), ldw(ldw_), ldx(ldx_), seen((size_t)n_ * k_, 0), stored(n_, 0) {}
    void w_load(int64_t off) {  // a 16-byte load at byte offset off
        w_lo = std::min(w_lo, off);
        w_hi = std::max(w_hi, off + 15);
    }
    void x_load(int64_t off, int elems) {  // elems 16-bit elements at element offset off
        x_lo = std::min(x_lo, off);
        x_hi = std::max(x_hi, off + elems - 1);
    }
    void consume(int row, int64_t w_off, int e, int bb, int64_t x_elem) {
        const int64_t i = w_off + e - (int64_t)row * ldw;  // code index in its row
        if (bb == 0) {
            if (i < 0 || i >= k) { ++dup; return; }
            if (++seen[(size_t)row * k + i] > 1) ++dup;
        }
        if (x_elem - (int64_t)bb * ldx != i) ++xk_mismatch;
    }
    void print(const char* kind, int rows, int cpl, int64_t bytes_in_flight) {
        int64_t missing = 0;
        for (uint8_t s : seen) missing += s == 0;
        int64_t unstored = 0;
        for (uint8_t s : stored) unstored += s != 1;
        printf("{\"kind\": \"%s\", \"rows\": %d, \"cpl\": %d, \"bytes_in_flight\": %lld, \"missing\": %lld, "
               "\"dup\": %lld, \"xk_mismatch\": %lld, \"unstored\": %lld, \"w\": [%lld, %lld], \"x\": [%lld, %lld], "
               "\"w_extent\": %lld, \"x_extent\": %lld}\n",
               kind, rows, cpl, (long long)bytes_in_flight, (long long)missing, (long long)dup,
               (long long)xk_mismatch, (long long)unstored, (long long)w_lo, (long long)w_hi, (long long)x_lo,
               (long long)x_hi, (long long)((int64_t)(n - 1) * ldw + k), (long long)((int64_t)(m - 1) * ldx + k));
    }
};

static void replay_vec(int m, int n, int k, int64_t ldw, int64_t ldx, bool swiglu) {
    Tally t(m, n, k, ldw, ldx);
    const Fp8wVecCfg cfg = fp8w_vec_cfg(k, swiglu);
    const int nchunks = k / kFp8wChunk;
    const int grid = fp8w_vec_grid(n, cfg.rows);
    for (int block = 0; block < grid; ++block)
        for (int wave = 0; wave < kFp8wVecWaves; ++wave) {
            const int64_t row0 = fp8w_vec_row0(block, wave, cfg.rows);
            if (row0 >= n) continue;
            for (int c0 = 0; c0 < nchunks; c0 += 64 * cfg.cpl)
                for (int lane = 0; lane < 64; ++lane)
                    for (int u = 0; u < cfg.cpl; ++u) {
                        const int cc = fp8w_vec_chunk(c0, lane, u);
                        const int ccl = fp8w_vec_chunk_clamped(cc, nchunks);
                        for (int r = 0; r < cfg.rows; ++r) {
                            const int row = fp8w_vec_row(row0, r, n);
                            const int64_t off = fp8w_vec_w_off(row, ccl, ldw);
                            t.w_load(off);
                            if (cc >= nchunks || row0 + r >= n) continue;  // masked chunk / a clamped row is not stored
                            for (int bb = 0; bb < m; ++bb) {
                                const int64_t xo = fp8w_vec_x_off(bb, cc, ldx);
                                if (r == 0) t.x_load(xo, 16);
                                for (int e = 0; e < 16; ++e) t.consume(row, off, e, bb, xo + e);
                            }
                        }
                    }
            for (int r = 0; r < cfg.rows; ++r)
                if (row0 + r < n) ++t.stored[row0 + r];
        }
    t.print("vec", cfg.rows, cfg.cpl, (int64_t)cfg.rows * cfg.cpl * (swiglu ? 2 : 1) * 1024);
}

static void replay_smallm(int m, int n, int k, int64_t ldw, int64_t ldx) {
    Tally t(m, n, k, ldw, ldx);
    const int nbg = fp8w_smallm_nbg(m), kw = fp8w_smallm_kw(k), steps = kw / kFp8wSmallmWaveStep;
    for (int n0 = 0; n0 < n; n0 += 16) {
        for (int wave = 0; wave < 4; ++wave)
            for (int s = 0; s < steps; ++s)
                for (int lane = 0; lane < 64; ++lane) {
                    const int row = fp8w_smallm_w_row(n0, lane, n);
                    const int kb = fp8w_smallm_k(wave, kw, s, lane);
                    const int64_t off = fp8w_smallm_w_off(row, kb, ldw);
                    t.w_load(off);
                    // The MFMA pairs slot 8 (lane >> 4) + j of this lane's A operand (W row lane & 15) with the
                    // same slot of EVERY lane's B operand in the lane group (X rows), so W and X agree when the
                    // k of slot (h, j) depends on (wave, step, lane >> 4) only and is the same on both sides.
                    for (int h = 0; h < 2; ++h)
                        for (int j = 0; j < 8; ++j) {
                            const int kk = fp8w_smallm_k_of(kb, h, j);  // the code's k: element 8 h + j of the load
                            if (off + 8 * h + j - (int64_t)row * ldw != kk) ++t.xk_mismatch;
                            if (kk < 0 || kk >= k) ++t.dup;
                            else if (++t.seen[(size_t)row * k + kk] > 1) ++t.dup;
                        }
                    for (int gi = 0; gi < nbg; ++gi) {
                        const int xr = fp8w_smallm_x_row(gi, lane, m);
                        for (int h = 0; h < 2; ++h) {
                            const int64_t xo = fp8w_smallm_x_off(xr, kb, h, ldx);
                            t.x_load(xo, 8);
                            for (int j = 0; j < 8; ++j)
                                if (xo + j - (int64_t)xr * ldx != fp8w_smallm_k_of(kb, h, j)) ++t.xk_mismatch;
                        }
                    }
                }
        for (int r = 0; r < 16 && n0 + r < n; ++r) ++t.stored[n0 + r];
    }
    t.print("smallm", 16, nbg, (int64_t)kFp8wSmallmUnroll * 1024);
}

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        long long a[13] = {0};
        char cmd[32] = {0};
        const int got = sscanf(line, "%31s %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", cmd, a, a + 1,
                               a + 2, a + 3, a + 4, a + 5, a + 6, a + 7, a + 8, a + 9, a + 10, a + 11, a + 12);
        if (got < 1) continue;
        if (!strcmp(cmd, "vec") && got == 7) {
            replay_vec((int)a[0], (int)a[1], (int)a[2], a[3], a[4], a[5] != 0);
        } else if (!strcmp(cmd, "smallm") && got == 6) {
            replay_smallm((int)a[0], (int)a[1], (int)a[2], a[3], a[4]);
        } else if (!strcmp(cmd, "route") && got == 14) {
            const Fp8wCall c{(int)a[0], (int)a[1], (int)a[2], a[3], a[4], a[5], (uintptr_t)a[6], (uintptr_t)a[7],
                             (uintptr_t)a[8], (uintptr_t)a[9], (uintptr_t)a[10], (size_t)a[11], a[12] != 0};
            printf("{\"route\": %d, \"need\": %zu}\n", fp8w_route(c), fp8w_workspace_need(c.n, c.k, c.swiglu));
        } else if (!strcmp(cmd, "wsize") && got == 5) {
            printf("{\"bytes\": %zu}\n", fp8w_workspace_size((int)a[0], (int)a[1], (int)a[2], a[3] != 0));
        } else {
            printf("{\"error\": \"bad command\"}\n");
        }
    }
    return 0;
}
