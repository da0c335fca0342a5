// Self-checking host program over csrc/fp4_codec.h (tests/test_fp4_codec.py): all 16 codes in both nibble positions
// against the table of include/pli.h, all 256 scale bytes, and the encoder at every value, every midpoint, their fp32
// neighbours, +-0, saturation and NaN against a nearest-of-8 in double with ties to the even code.  Exits 1 on a failure.
#include <cmath>
#include <cstdio>
#include <initializer_list>

#include "fp4_codec.h"

using namespace pli;

static int bad = 0, checked = 0;
static void expect(bool ok, const char* what, double a, double b) {
    if (++checked, !ok) ++bad, printf("FAIL %s %.9g %.9g\n", what, a, b);
}

int main() {
    const float grid[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
    for (int b = 0; b < 256; ++b) {
        for (int pos = 0; pos < 2; ++pos) {
            const int code = (b >> (4 * pos)) & 15;
            const float want = code & 8 ? -grid[code & 7] : grid[code & 7];  // code 8 is -0
            expect(fp8_f32_bits(fp4_e2m1_decode(fp4_nibble((uint8_t)b, pos))) == fp8_f32_bits(want), "decode", b, pos);
        }
        const float s = e8m0_decode((uint8_t)b);
        expect(b == 255 ? s != s : (double)s == std::ldexp(1.0, b - 127), "scale", b, s);
    }
    float xs[64] = {0.f, 6.5f, 7.f, 1e30f, INFINITY};
    int n = 5;
    for (int i = 0; i < 8; ++i)
        for (float v : {grid[i], i < 7 ? 0.5f * (grid[i] + grid[i + 1]) : 6.f})
            for (float x : {v, std::nextafterf(v, -1.f), std::nextafterf(v, 8.f)}) xs[n++] = x;
    for (int i = 0; i < n; ++i)
        for (float x : {xs[i], -xs[i]}) {
            const double a = std::fmin(std::fabs((double)x), 6.0);
            int want = 0;
            for (int c = 1; c < 8; ++c) {  // nearest; at equal distance the even code
                const double d = std::fabs(grid[c] - a), dw = std::fabs(grid[want] - a);
                if (d < dw || (d == dw && c % 2 == 0)) want = c;
            }
            expect(fp4_e2m1_encode(x) == (want | (std::signbit(x) ? 8 : 0)), "encode", x, fp4_e2m1_encode(x));
        }
    expect((fp4_e2m1_encode(NAN) & 7) == 7, "encode NaN saturates", 0, 0), printf("checked %d\n", checked);
    return bad != 0;
}
