// Host check of protopformer_amd/csrc/order_keys.h, the ordering policy of the ranking kernels: a stand-alone program built with the host
// compiler (tests/test_order_keys_cpu.py), no GPU.  A fixed table of floats -- the edge values, a fixed linear-congruential sequence of bit
// patterns over all exponents, two NaN payloads -- and every property the kernels rely on.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "order_keys.h"

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++failures <= 20) {                       \
                printf("FAIL %s: ", #cond);               \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
        }                                                 \
    } while (0)

static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static float from_bits(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }

int main() {
    const float dmin = from_bits(1u);                       // smallest denormal
    std::vector<float> vals = {0.0f, -0.0f, dmin, -dmin, FLT_MIN, -FLT_MIN, 1.0f, -1.0f, FLT_MAX, -FLT_MAX, INFINITY, -INFINITY};
    uint32_t x = 12345u;
    while (vals.size() < 3000) {
        x = x * 1664525u + 1013904223u;                     // all 32 bits: every exponent and both signs turn up
        const float v = from_bits(x);
        if (v == v) vals.push_back(v);
    }
    const float nans[2] = {from_bits(0x7fc00000u), from_bits(0xffc12345u)};
    const size_t n = vals.size();

    for (size_t i = 0; i < n; ++i) {
        const float a = vals[i];
        CHECK(bits(key_value(order_key(a))) == bits(a), "round trip of %08x", bits(a));
        CHECK(!comes_before(a, 3, a, 3), "irreflexive at %08x", bits(a));
        CHECK(score_key(a) > 0u && score_key(a) >= score_key(-INFINITY), "score_key(%08x) above the NaN key", bits(a));
        for (size_t j = 0; j < n; ++j) {
            const float b = vals[j];
            if (a < b) CHECK(order_key(a) < order_key(b), "order_key increasing %08x %08x", bits(a), bits(b));
            if (a <= b) CHECK(score_key(a) <= score_key(b), "score_key non-decreasing %08x %08x", bits(a), bits(b));
            if (a == b) CHECK(score_key(a) == score_key(b), "score_key equal on equal values %08x %08x", bits(a), bits(b));
            // distinct (value, id) pairs: exactly one comes first -- different values with any ids, equal values with different ids
            for (int ia = 0; ia < 2; ++ia)
                for (int ib = 0; ib < 2; ++ib) {
                    if (a == b && ia == ib) continue;
                    CHECK(comes_before(a, ia, b, ib) != comes_before(b, ib, a, ia), "exactly one of (%08x, %d) (%08x, %d)", bits(a), ia, bits(b), ib);
                }
        }
        for (float q : nans) {
            CHECK(!comes_before(a, 0, q, 1) && !comes_before(q, 1, a, 0) && !comes_before(q, 0, a, 1) && !comes_before(a, 1, q, 0),
                  "NaN against %08x", bits(a));
        }
    }
    CHECK(order_key(-0.0f) < order_key(0.0f), "-0 one below +0");
    CHECK(score_key(-0.0f) == score_key(0.0f), "score_key(-0) == score_key(+0)");
    for (float q : nans) {
        CHECK(bits(key_value(order_key(q))) == bits(q), "round trip of NaN %08x", bits(q));
        CHECK(score_key(q) == 0u && 0u < score_key(-INFINITY), "NaN lowest");
        CHECK(!comes_before(q, 0, q, 1) && !comes_before(q, 1, q, 0) && !comes_before(q, 0, q, 0), "NaN against NaN");
    }
    // the integer form the cell order uses
    CHECK(comes_before(5ull, 9, 4ull, 0) && !comes_before(4ull, 0, 5ull, 9) && comes_before(4ull, 0, 4ull, 1) && !comes_before(4ull, 1, 4ull, 1),
          "64-bit keys");

    if (failures) {
        printf("order keys: %d failures\n", failures);
        return 1;
    }
    printf("order keys: ok (%zu values, %zu pairs)\n", n, n * n);
    return 0;
}
