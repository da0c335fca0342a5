// CPU driver for csrc/flash_plan.h (tests/test_flash_plan.py builds and runs
// it; no HIP): one call per input line,
//   B H Hkv Nq Nk D dtype(bf16|f16|f32) causal s0 .. s11 scale variant cus q k v o
// (element strides qb qh qn kb kh kn vb vh vn ob oh on, four fake addresses),
// one JSON line out: the plan, the route, and -- for the v13 / pp64 families --
// the grid and the 64 argument words.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "flash_plan.h"

int main() {
    using namespace pli;
    static const char* const kFamily[] = {"generic", "v2", "v7", "v12", "v13", "pp64", "unknown"};
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        FlashCall f{};
        int Hkv = 0, causal = 0, variant = 0;
        std::string dtype;
        int64_t s[12];
        double scale = 0;
        uint64_t p[4];
        in >> f.B >> f.H >> Hkv >> f.Nq >> f.Nk >> f.D >> dtype >> causal;
        for (auto& x : s) in >> x;
        in >> scale >> variant >> f.cus;
        for (auto& x : p) in >> x;
        if (!in || Hkv <= 0 || f.H % Hkv != 0) {
            std::fprintf(stderr, "flash_plan_check: bad case: %s\n", line.c_str());
            return 2;
        }
        f.group = f.H / Hkv;
        f.fp16 = dtype == "f16";
        f.causal = causal != 0;
        f.st = V7Strides{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9], s[10], s[11]};
        f.scale = (float)scale;
        f.mfma_operands = dtype != "f32" && ((p[0] | p[1] | p[2] | p[3]) & 15) == 0;
        const FlashPlan plan = plan_flash(f, variant);
        std::printf("{\"family\": \"%s\", \"route\": \"%s\", \"variant\": %d, \"sub\": %d, \"persistent\": %s, "
                    "\"thr\": %g, \"muoff\": %g",
                    kFamily[(int)plan.family], flash_route(f, plan).name, plan.variant, plan.sub,
                    plan.persistent ? "true" : "false", plan.thr, plan.muoff);
        if (plan.family == FlashFamily::v13 || plan.family == FlashFamily::pp64) {
            const V13Launch L = pack_v13(f, plan, (const void*)(uintptr_t)p[0], (const void*)(uintptr_t)p[1],
                                         (const void*)(uintptr_t)p[2], (void*)(uintptr_t)p[3]);
            std::printf(", \"error\": \"%s\", \"grid\": %d, \"D\": %d, \"pp64\": %d, \"fp16\": %d, \"causal\": %d, "
                        "\"ragged\": %d, \"args\": [",
                        L.error, L.grid, L.D, L.pp64, L.fp16, L.causal, L.ragged);
            for (int i = 0; i < 64; ++i) std::printf("%s%" PRIu32, i ? ", " : "", L.args.w[i]);
            std::printf("]");
        }
        std::printf("}\n");
    }
    return 0;
}
