// Host check of pixel_order_key (protopformer_amd/csrc/order_keys.h), the composite 64-bit key ppf_pixel_order's contract is written in: a
// stand-alone program built with the host compiler (tests/test_pixel_faithfulness_cpu.py), no GPU.  Over a table of edge values and over
// random pairs the key must be strictly monotone in the order "larger score_key first, then the smaller index": a < b exactly when
// (score a, index a) comes before (score b, index b), and equal only for the same index with scores of the same key.
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

// the order of the contract, written without the key under test: by score_key descending (comes_before on the integer keys), then by index
static bool before(float a, uint32_t ia, float b, uint32_t ib) {
    const uint32_t ka = score_key(a), kb = score_key(b);
    return ka > kb || (ka == kb && ia < ib);
}

static void check_pair(float a, uint32_t ia, float b, uint32_t ib) {
    const uint64_t ka = pixel_order_key(a, ia), kb = pixel_order_key(b, ib);
    CHECK((ka < kb) == before(a, ia, b, ib), "(%08x, %u) against (%08x, %u)", bits(a), ia, bits(b), ib);
    CHECK((ka == kb) == (score_key(a) == score_key(b) && ia == ib), "equality of (%08x, %u) (%08x, %u)", bits(a), ia, bits(b), ib);
    CHECK((uint32_t)ka == ia && (uint32_t)(ka >> 32) == ~score_key(a), "the words of the key of (%08x, %u)", bits(a), ia);
}

int main() {
    const float dmin = from_bits(1u);                       // smallest denormal
    const std::vector<float> vals = {0.0f, -0.0f, dmin, -dmin, FLT_MIN, -FLT_MIN, 1.0f, -1.0f, 1.0f + FLT_EPSILON, FLT_MAX, -FLT_MAX, INFINITY,
                                     -INFINITY, from_bits(0x7fc00000u), from_bits(0xffc12345u), from_bits(0x7f800001u)};
    const std::vector<uint32_t> ids = {0u, 1u, 2u, 50175u, 65534u, 65535u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
    size_t pairs = 0;
    for (float a : vals)
        for (float b : vals)
            for (uint32_t ia : ids)
                for (uint32_t ib : ids) { check_pair(a, ia, b, ib); ++pairs; }

    uint32_t x = 2463534242u;
    auto next = [&x]() { x = x * 1664525u + 1013904223u; return x; };
    for (int t = 0; t < 2000000; ++t) {                     // random bit patterns (NaNs included), indices of a row and beyond
        const float a = from_bits(next()), b = (t & 3) ? from_bits(next()) : a;
        const uint32_t ia = next() >> ((t & 4) ? 16 : 0), ib = (t & 8) ? ia : next() >> 16;
        check_pair(a, ia, b, ib);
        ++pairs;
    }

    // a sorted row: ascending keys are the order itself, whatever the sort
    std::vector<float> row = {0.5f, -0.0f, from_bits(0x7fc00000u), 0.5f, 0.0f, INFINITY, -INFINITY, from_bits(0xffc00000u), 2.0f};
    const uint32_t want[9] = {5, 8, 0, 3, 1, 4, 6, 2, 7};   // inf, 2, the two 0.5 by index, the zeros by index, -inf, the NaNs by index
    for (int r = 0; r < 9; ++r) {
        int smaller = 0;
        for (uint32_t j = 0; j < 9; ++j) smaller += pixel_order_key(row[j], j) < pixel_order_key(row[want[r]], want[r]);
        CHECK(smaller == r, "pixel %u has rank %d, expected %d", want[r], smaller, r);
    }

    if (failures) {
        printf("pixel order key: %d failures\n", failures);
        return 1;
    }
    printf("pixel order key: ok (%zu pairs)\n", pairs);
    return 0;
}
