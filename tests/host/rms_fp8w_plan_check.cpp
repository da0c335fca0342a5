// Host replay of the index arithmetic of rms_gemm_fp8w
// (csrc/decode_fused_fp8w.hip) from csrc/rms_fp8w_plan.h and the fp8w_vec_*
// functions of csrc/fp8w_plan.h it reuses.  Built by tests/test_rms_fp8w_plan.py
// with the host compiler (under AddressSanitizer + UBSan where available) and
// driven through stdin, one command per line, one JSON object per line out:
//   rms m k swiglu ldw ngroups n0 n1 n2
// every weight load, every consumed code with the LDS X element it is paired
// with, and every stored (group, row) of the launch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rms_fp8w_plan.h"

using namespace pli;

static void replay(int m, int k, bool swiglu, int64_t ldw, int ngroups, const int* n) {
    const Fp8wVecCfg cfg = fp8w_vec_cfg(k, swiglu);
    const int nchunks = k / kFp8wChunk;
    const int ntot = rms_fp8w_total(n, ngroups);
    const int grid = rms_fp8w_grid(ntot, cfg.rows);  // what the launcher passes to the launch
    const int64_t lds_elems = (int64_t)(rms_fp8w_lds_bytes(m, k) / 2);
    std::vector<std::vector<uint8_t>> seen(ngroups), stored(ngroups);
    for (int g = 0; g < ngroups; ++g) {
        seen[g].assign((size_t)n[g] * k, 0);
        stored[g].assign(n[g], 0);
    }
    int64_t w_oob = 0, x_oob = 0, xk_mismatch = 0, dup = 0, clamp_mismatch = 0, active_waves = 0;
    for (int block = 0; block < grid; ++block)
        for (int wave = 0; wave < kFp8wVecWaves; ++wave) {
            const int64_t row0 = fp8w_vec_row0(block, wave, cfg.rows);
            if (row0 >= ntot) continue;  // an inactive wave: barriers only
            ++active_waves;
            for (int c0 = 0; c0 < nchunks; c0 += 64 * cfg.cpl)
                for (int lane = 0; lane < 64; ++lane)
                    for (int u = 0; u < cfg.cpl; ++u) {
                        const int cc = fp8w_vec_chunk(c0, lane, u);
                        const int ccl = fp8w_vec_chunk_clamped(cc, nchunks);
                        for (int r = 0; r < cfg.rows; ++r) {
                            const RmsFp8wRow lr = rms_fp8w_load_row(row0 + r, n, ngroups);
                            if (lr.group < 0 || lr.group >= ngroups || lr.row < 0 || lr.row >= n[lr.group]) {
                                ++w_oob;
                                continue;
                            }
                            const int64_t off = fp8w_vec_w_off(lr.row, ccl, ldw);
                            // the 16 bytes of the load inside group lr.group's operand [0, (n_g - 1) ldw + k)
                            if (off < 0 || off + 15 >= (int64_t)(n[lr.group] - 1) * ldw + k) ++w_oob;
                            if (cc >= nchunks || row0 + r >= ntot) continue;  // masked chunk / clamped row
                            const RmsFp8wRow orow = rms_fp8w_resolve(row0 + r, n, ngroups);
                            if (orow.group != lr.group || orow.row != lr.row) ++clamp_mismatch;
                            for (int bb = 0; bb < m; ++bb) {
                                const int64_t xo = rms_fp8w_x_off(bb, cc, k);
                                if (xo < 0 || xo + 15 >= lds_elems) ++x_oob;
                                for (int e = 0; e < 16; ++e) {
                                    const int64_t i = off + e - (int64_t)lr.row * ldw;  // the code's k
                                    if (xo + e - (int64_t)bb * k != i) ++xk_mismatch;
                                    if (bb == 0) {
                                        if (i < 0 || i >= k) ++dup;
                                        else if (++seen[lr.group][(size_t)lr.row * k + i] > 1) ++dup;
                                    }
                                }
                            }
                        }
                    }
            for (int r = 0; r < cfg.rows; ++r) {
                if (row0 + r >= ntot) break;
                const RmsFp8wRow orow = rms_fp8w_resolve(row0 + r, n, ngroups);
                if (orow.group >= ngroups || orow.row >= n[orow.group]) ++w_oob;
                else ++stored[orow.group][orow.row];
            }
        }
    int64_t missing = 0, unstored = 0;
    for (int g = 0; g < ngroups; ++g) {
        for (uint8_t s : seen[g]) missing += s == 0;
        for (uint8_t s : stored[g]) unstored += s != 1;
    }
    // the first workgroup past the grid would have no active wave, the last one inside has at least one
    const bool grid_tight = fp8w_vec_row0(grid, 0, cfg.rows) >= ntot && fp8w_vec_row0(grid - 1, 0, cfg.rows) < ntot;
    const int rpt = rms_fp8w_norm_rpt(k);
    printf("{\"rows\": %d, \"cpl\": %d, \"grid\": %d, \"grid_tight\": %d, \"active_waves\": %lld, \"rpt\": %d, "
           "\"norm_cover\": %d, \"lds_bytes\": %zu, \"missing\": %lld, \"dup\": %lld, \"xk_mismatch\": %lld, "
           "\"unstored\": %lld, \"w_oob\": %lld, \"x_oob\": %lld, \"clamp_mismatch\": %lld}\n",
           cfg.rows, cfg.cpl, grid, (int)grid_tight, (long long)active_waves, rpt,
           (int)(256 * rpt * kRmsFp8wNormChunk >= k), rms_fp8w_lds_bytes(m, k), (long long)missing, (long long)dup,
           (long long)xk_mismatch, (long long)unstored, (long long)w_oob, (long long)x_oob,
           (long long)clamp_mismatch);
}

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        long long a[8] = {0};
        char cmd[32] = {0};
        const int got = sscanf(line, "%31s %lld %lld %lld %lld %lld %lld %lld %lld", cmd, a, a + 1, a + 2, a + 3, a + 4,
                               a + 5, a + 6, a + 7);
        if (got == 9 && !strcmp(cmd, "rms") && a[0] >= 1 && a[0] <= kRmsFp8wMaxM && a[1] > 0 &&
            a[1] % kFp8wChunk == 0 && a[1] <= kRmsFp8wMaxK && a[3] >= a[1] && a[4] >= 1 &&
            a[4] <= kRmsFp8wMaxGroups) {
            const int n[3] = {(int)a[5], (int)a[6], (int)a[7]};
            bool ok = true;
            for (int g = 0; g < (int)a[4]; ++g) ok = ok && n[g] > 0;
            if (ok) {
                replay((int)a[0], (int)a[1], a[2] != 0, a[3], (int)a[4], n);
                continue;
            }
        }
        printf("{\"error\": \"bad command\"}\n");
    }
    return 0;
}
