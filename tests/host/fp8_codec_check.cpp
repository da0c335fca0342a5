// CPU driver for csrc/fp8_codec.h and the fp8 fast / generic rules of
// csrc/paged_plan.h and csrc/varlen_plan.h (tests/test_fp8_codec.py builds and
// runs it; no HIP).  One command per input line, one JSON line out:
//   decode                               -> the fp32 bit patterns of all 256 codes
//   encode u0 u1 ..                      -> the codes of the fp32 values with these
//                                           bit patterns (decimal uint32)
//   paged dtype D rows bs scale aligned s0 .. s11
//                                        -> paged_fast_path (as 16-bit strides) and
//                                           paged_fast_path_fp8 of the same line
//   varlen dtype D heads kv_heads bs scale aligned s0 .. s9
//                                        -> the same for the varlen rules
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "fp8_codec.h"
#include "varlen_plan.h"

int main() {
    using namespace pli;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "decode") {
            std::printf("{\"bits\": [");
            for (int c = 0; c < 256; ++c) std::printf("%s%" PRIu32, c ? ", " : "", fp8_f32_bits(fp8_e4m3_decode((uint8_t)c)));
            std::printf("]}\n");
        } else if (cmd == "encode") {
            std::printf("{\"codes\": [");
            uint32_t u = 0;
            for (int i = 0; in >> u; ++i) std::printf("%s%d", i ? ", " : "", (int)fp8_e4m3_encode(fp8_bits_f32(u)));
            std::printf("]}\n");
        } else if (cmd == "paged") {
            int dtype = 0, D = 0, bs = 0, aligned = 0;
            int64_t rows = 0, s[12];
            double scale = 0;
            in >> dtype >> D >> rows >> bs >> scale >> aligned;
            for (auto& x : s) in >> x;
            if (!in) return 2;
            std::printf("{\"fast\": %s, \"fast_fp8\": %s}\n",
                        paged_fast_path(dtype, D, rows, bs, (float)scale, s, aligned != 0) ? "true" : "false",
                        paged_fast_path_fp8(dtype, D, rows, bs, (float)scale, s, aligned != 0) ? "true" : "false");
        } else if (cmd == "varlen") {
            int dtype = 0, D = 0, heads = 0, kv_heads = 0, bs = 0, aligned = 0;
            int64_t s[10];
            double scale = 0;
            in >> dtype >> D >> heads >> kv_heads >> bs >> scale >> aligned;
            for (auto& x : s) in >> x;
            if (!in) return 2;
            std::printf("{\"fast\": %s, \"fast_fp8\": %s}\n",
                        varlen_fast_path(dtype, D, heads, kv_heads, bs, (float)scale, s, aligned != 0) ? "true" : "false",
                        varlen_fast_path_fp8(dtype, D, heads, kv_heads, bs, (float)scale, s, aligned != 0) ? "true" : "false");
        } else {
            std::fprintf(stderr, "fp8_codec_check: bad command: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
