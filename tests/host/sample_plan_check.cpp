// Host replay of csrc/sample_plan.h (tests/test_sample_plan.py): the functions
// the sampling kernel calls, compiled with the host compiler and run alone.
// One command per input line, one JSON object per output line:
//   philox c0 c1 c2 c3 k0 k1        -> the four output words
//   u seed offset row0 count        -> float bits of sample_philox_u for rows row0 .. row0 + count - 1
//   keys16 dtype                    -> the key transform over all 2^16 patterns of fp16 (1) / bf16 (2)
//   keys32 count                    -> ... over a sweep of fp32 patterns (edges, denormals, `count` random)
//   cover vocab                     -> the wave / step / lane map over one row
//   weight xbits mbits tbits        -> sample_weight_fx of three fp32 bit patterns
//   scale fbits s                   -> sample_scale_fx
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sample_plan.h"

using namespace pli;

static float f32_of(uint32_t b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
}
static uint32_t bits_of(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}
// value of a 16-bit pattern as a double (NaN stays NaN)
static double value16(uint32_t b, int dtype) {
    if (dtype == 2) return (double)f32_of(b << 16);
    const int s = (b >> 15) & 1, e = (b >> 10) & 31, m = b & 1023;
    double v;
    if (e == 31)
        v = m ? NAN : INFINITY;
    else if (e == 0)
        v = ldexp((double)m, -24);
    else
        v = ldexp((double)(m + 1024), e - 25);
    return s ? -v : v;
}

struct KV {
    uint32_t key, bits;
    double value;  // canonical: NaN -> -inf, -0 -> +0
};

// strict order preservation over a set of patterns: along ascending keys the canonical values ascend, and two
// patterns share a key iff they share a canonical value
static void check_keys(std::vector<KV>& v, int dtype) {
    long violations = 0, digit_mismatch = 0, unkey_mismatch = 0, nan_not_lowest = 0;
    const uint32_t lowest = sample_key_neg_inf(dtype);
    for (KV& e : v) {
        double x = e.value;
        if (x != x) {
            x = -INFINITY;
            if (e.key != lowest) ++nan_not_lowest;
        }
        if (x == 0) x = 0.0;  // (-0 -> +0)
        e.value = x;
        if (e.key < lowest) ++violations;
        // digits from the top rebuild the key
        uint32_t prefix = 0;
        for (int p = 0; p < sample_digit_passes(dtype); ++p) {
            if (sample_prefix(e.key, p, dtype) != prefix) ++digit_mismatch;
            const uint32_t d = sample_digit(e.key, p, dtype);
            if (d > 255) ++digit_mismatch;
            prefix = (prefix << kSampleDigitBits) | d;
        }
        if (prefix != e.key) ++digit_mismatch;
        // the inverse gives the canonical value back
        const uint32_t back = dtype == 0 ? sample_unkey_f32(e.key) : sample_unkey_16(e.key);
        const double bv = dtype == 0 ? (double)f32_of(back) : value16(back, dtype);
        if (!(bv == x) || (x == 0 && back != 0)) ++unkey_mismatch;
        if (sample_key(back, dtype) != e.key) ++unkey_mismatch;
    }
    std::sort(v.begin(), v.end(), [](const KV& a, const KV& b) { return a.key < b.key; });
    long distinct = v.empty() ? 0 : 1;
    for (size_t i = 1; i < v.size(); ++i) {
        const bool keq = v[i].key == v[i - 1].key, veq = v[i].value == v[i - 1].value;
        if (keq != veq) ++violations;
        if (!keq && !(v[i].value > v[i - 1].value)) ++violations;
        if (!keq) ++distinct;
    }
    printf("{\"n\": %zu, \"violations\": %ld, \"digit_mismatch\": %ld, \"unkey_mismatch\": %ld, "
           "\"nan_not_lowest\": %ld, \"distinct\": %ld, \"lowest\": %u, \"highest\": %u}\n",
           v.size(), violations, digit_mismatch, unkey_mismatch, nan_not_lowest, distinct, lowest,
           sample_key_pos_inf(dtype));
}

int main() {
    char line[512];
    while (fgets(line, sizeof(line), stdin)) {
        char cmd[32] = {0};
        if (sscanf(line, "%31s", cmd) != 1) continue;
        const char* rest = line + strlen(cmd);
        if (!strcmp(cmd, "philox")) {
            uint32_t a[6];
            if (sscanf(rest, "%u %u %u %u %u %u", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) != 6) return 2;
            const Philox4 o = philox4x32_10(a[0], a[1], a[2], a[3], a[4], a[5]);
            printf("{\"out\": [%u, %u, %u, %u]}\n", o.v[0], o.v[1], o.v[2], o.v[3]);
        } else if (!strcmp(cmd, "u")) {
            uint64_t seed;
            int64_t offset;
            uint32_t row0;
            int count;
            if (sscanf(rest, "%" SCNu64 " %" SCNd64 " %u %d", &seed, &offset, &row0, &count) != 4) return 2;
            printf("{\"u_bits\": [");
            for (int i = 0; i < count; ++i) {
                const float u = sample_philox_u(seed, offset, row0 + (uint32_t)i);
                if (!(u >= 0.0f && u < 1.0f)) return 3;
                printf("%s%u", i ? ", " : "", bits_of(u));
            }
            printf("]}\n");
        } else if (!strcmp(cmd, "keys16")) {
            int dtype;
            if (sscanf(rest, "%d", &dtype) != 1 || (dtype != 1 && dtype != 2)) return 2;
            std::vector<KV> v;
            for (uint32_t b = 0; b < 65536; ++b) v.push_back(KV{sample_key(b, dtype), b, value16(b, dtype)});
            check_keys(v, dtype);
        } else if (!strcmp(cmd, "keys32")) {
            int count;
            if (sscanf(rest, "%d", &count) != 1) return 2;
            std::vector<uint32_t> pat = {0u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u,
                                         0x7f800001u, 0xff800001u, 0x7fffffffu, 0xffffffffu, 0x7f7fffffu, 0xff7fffffu,
                                         0x00800000u, 0x80800000u, 0x3f800000u, 0xbf800000u};
            for (uint32_t m = 1; m < 0x00800000u; m = m * 3 + 1) {  // denormals of both signs
                pat.push_back(m);
                pat.push_back(m | 0x80000000u);
            }
            for (uint32_t e = 0; e < 256; ++e)  // every exponent, both signs, three mantissas
                for (uint32_t m : {0u, 1u, 0x7fffffu}) {
                    pat.push_back((e << 23) | m);
                    pat.push_back((e << 23) | m | 0x80000000u);
                }
            uint64_t s = 0x2545F4914F6CDD1Dull;
            for (int i = 0; i < count; ++i) {
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                pat.push_back((uint32_t)(s >> 32));
            }
            std::vector<KV> v;
            for (uint32_t b : pat) v.push_back(KV{sample_key(b, 0), b, (double)f32_of(b)});
            check_keys(v, 0);
        } else if (!strcmp(cmd, "cover")) {
            int vocab;
            if (sscanf(rest, "%d", &vocab) != 1 || vocab < 1 || vocab > kSampleMaxVocab) {
                printf("{\"error\": \"vocab\"}\n");
                continue;
            }
            const int seg = sample_seg_len(vocab), steps = sample_seg_steps(vocab);
            std::vector<int> seen((size_t)vocab, 0);
            long dup = 0, disorder = 0;
            int prev = -1;
            for (int w = 0; w < kSampleWaves; ++w)
                for (int st = 0; st < steps; ++st)
                    for (int l = 0; l < 64; ++l) {
                        const int i = sample_index(w, st, l, seg);
                        if (i < 0) return 3;
                        if (i >= vocab) continue;  // (the kernel's bound check)
                        if (seen[(size_t)i]++) ++dup;
                        if (i != prev + 1) ++disorder;  // wave, step, lane order IS index order
                        prev = i;
                    }
            long missing = 0;
            for (int i = 0; i < vocab; ++i) missing += seen[(size_t)i] == 0;
            printf("{\"seg\": %d, \"steps\": %d, \"waves\": %d, \"threads\": %d, \"missing\": %ld, \"dup\": %ld, "
                   "\"disorder\": %ld, \"max_vocab\": %d}\n",
                   seg, steps, kSampleWaves, kSampleThreads, missing, dup, disorder, kSampleMaxVocab);
        } else if (!strcmp(cmd, "weight")) {
            uint32_t x, m, t;
            if (sscanf(rest, "%u %u %u", &x, &m, &t) != 3) return 2;
            printf("{\"w\": %" PRIu64 "}\n", sample_weight_fx(f32_of(x), f32_of(m), f32_of(t)));
        } else if (!strcmp(cmd, "scale")) {
            uint32_t f;
            uint64_t s;
            if (sscanf(rest, "%u %" SCNu64, &f, &s) != 2) return 2;
            printf("{\"v\": %" PRIu64 "}\n", sample_scale_fx(f32_of(f), s));
        } else {
            printf("{\"error\": \"unknown command\"}\n");
        }
    }
    return 0;
}
