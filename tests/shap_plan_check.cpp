// Host check of protopformer_amd/csrc/shap_plan.h, the index rules of the KernelSHAP kernels: a stand-alone program built with the host
// compiler (tests/test_shap_plan_cpu.py), no GPU.  The size rule over honest and hostile tables, the membership rank exhaustively for
// d = 4, the two player maps against each other, and the bit packing at d = 196.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "shap_plan.h"

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

// table[t] = round(2^24 * P(size <= t + 1)), P(size = k) ~ 1 / (k (d - k)); the library's table is computed in exact arithmetic by Python,
// this one in long double: the rule under test holds for any table
static std::vector<int32_t> size_table(int d) {
    long double total = 0;
    for (int k = 1; k < d; ++k) total += 1.0L / ((long double)k * (d - k));
    std::vector<int32_t> t(d - 1);
    long double run = 0;
    for (int k = 1; k < d; ++k) {
        run += 1.0L / ((long double)k * (d - k));
        t[k - 1] = (int32_t)llroundl(run / total * (long double)SHAP_TABLE_ONE);
    }
    t[d - 2] = SHAP_TABLE_ONE;
    return t;
}

int main() {
    long checks = 0;
    // ---- the size rule
    for (int s = SHAP_MIN_S; s <= SHAP_MAX_S; ++s) {
        const int d = s * s;
        const std::vector<int32_t> t = size_table(d);
        for (int k = 0; k + 1 < d - 1; ++k) CHECK(t[k] <= t[k + 1], "d=%d: table not non-decreasing at %d", d, k);
        CHECK(t[d - 2] == SHAP_TABLE_ONE, "d=%d: the table ends at %d", d, t[d - 2]);
        CHECK(shap_size(t.data(), d, 0u) == 1 + (t[0] <= 0 ? 1 : 0), "d=%d: the smallest draw", d);
        CHECK(shap_size(t.data(), d, (1u << 24) - 1u) <= d - 1, "d=%d: the largest draw", d);
        int last = 0;
        for (int k = 0; k + 3 <= d; ++k) {
            for (int64_t u : {(int64_t)t[k] - 1, (int64_t)t[k]}) {
                if (u < 0 || u >= (1 << 24)) continue;
                const int size = shap_size(t.data(), d, (uint32_t)u);
                int want = 1;
                for (int q = 0; q + 3 <= d; ++q) want += t[q] <= u ? 1 : 0;
                CHECK(size == want && size >= 1 && size <= d - 1, "d=%d u=%lld: size %d, want %d", d, (long long)u, size, want);
                CHECK(size >= last, "d=%d: the size falls as the draw grows", d);
                CHECK(u != t[k] || size >= k + 2, "d=%d: a draw at table[%d] has passed %d entries", d, k, k + 1);
                last = size;
                ++checks;
            }
        }
        // hostile tables: the size stays in [1, d - 1] whatever they hold (the entry past d - 3 is never read as a size)
        std::vector<int32_t> zero(d - 1, 0), neg(d - 1, INT32_MIN), big(d - 1, INT32_MAX);
        for (uint32_t u : {0u, 12345u, (1u << 24) - 1u}) {
            CHECK(shap_size(zero.data(), d, u) == d - 1, "d=%d: all-zero table", d);
            CHECK(shap_size(neg.data(), d, u) == d - 1, "d=%d: negative table", d);
            CHECK(shap_size(big.data(), d, u) == 1, "d=%d: huge table", d);
        }
    }
    // ---- the pair counter: both samples of a pair share it; the range is the contract's
    CHECK(shap_pair_counter(0) == 0x80000001u && shap_pair_counter(1) == 0x80000001u && shap_pair_counter(2) == 0x80000002u, "first pairs");
    CHECK(shap_pair_counter(SHAP_MAX_N - 1) == 0x80000001u + (uint32_t)(SHAP_MAX_N / 2 - 1) && shap_pair_counter(SHAP_MAX_N - 1) <= 0xC0000000u, "last pair");
    // ---- the membership rank, exhaustively for d = 4 over keys with ties and both ends of the range
    const uint32_t alphabet[4] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu};
    for (int code = 0; code < 256; ++code) {
        uint32_t keys[4];
        for (int q = 0; q < 4; ++q) keys[q] = alphabet[(code >> (2 * q)) & 3];
        std::vector<std::pair<uint32_t, int>> sorted;
        for (int q = 0; q < 4; ++q) sorted.push_back({keys[q], q});
        std::sort(sorted.begin(), sorted.end());                              // (key, player) ascending: the contract's order
        int seen = 0;
        for (int pos = 0; pos < 4; ++pos) {
            const int q = sorted[pos].second;
            CHECK(shap_rank(keys, 4, q) == pos, "keys %d: player %d has rank %d, its place in the sort is %d", code, q, shap_rank(keys, 4, q), pos);
            seen |= 1 << shap_rank(keys, 4, q);
        }
        CHECK(seen == 15, "keys %d: the ranks are no permutation", code);
        for (int size = 1; size <= 3; ++size) {
            int members = 0;
            for (int q = 0; q < 4; ++q) members += shap_member(keys, 4, q, size) ? 1 : 0;
            CHECK(members == size, "keys %d: %d members at size %d", code, members, size);
            for (int pos = 0; pos < 4; ++pos)
                CHECK(shap_member(keys, 4, sorted[pos].second, size) == (pos < size), "keys %d size %d: place %d", code, size, pos);
            ++checks;
        }
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b)
                if (a != b)
                    CHECK(shap_key_before(keys[a], a, keys[b], b) != shap_key_before(keys[b], b, keys[a], a), "keys %d: exactly one of %d, %d first", code,
                          a, b);
        CHECK(!shap_key_before(keys[0], 0, keys[0], 0), "irreflexive");
    }
    // ---- the player maps: (image size, grid side, players per side)
    const int shapes[][3] = {{224, 14, 7}, {224, 14, 14}, {224, 14, 2}, {64, 4, 2}, {64, 4, 4}, {32, 2, 2}, {448, 28, 14}};
    for (const auto& sh : shapes) {
        const int H = sh[0], side = sh[1], s = sh[2], d = s * s, patch = H / side, r = side / s;
        CHECK(side % s == 0 && H % side == 0 && (H / s) % 4 == 0, "shape %d %d %d is no valid case", H, side, s);
        std::vector<int> pixels(d, 0), cells(d, 0);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < H; ++x) {
                const int q = shap_pixel_player(y, x, H, s);
                CHECK(q >= 0 && q < d, "pixel (%d, %d): player %d", y, x, q);
                if (q < 0 || q >= d) continue;
                ++pixels[q];
                CHECK(q == shap_cell_player(y / patch, x / patch, r, s), "H=%d s=%d: pixel (%d, %d) and its cell disagree", H, s, y, x);
                CHECK(q == shap_pixel_player(y, x & ~3, H, s), "H=%d s=%d: a 16-byte vector straddles two players at (%d, %d)", H, s, y, x);
                CHECK(q == (y / (H / s)) * s + x / (H / s), "H=%d s=%d: the contract's formula at (%d, %d)", H, s, y, x);
                ++checks;
            }
        for (int g = 0; g < side * side; ++g) ++cells[shap_cell_player(g / side, g % side, r, s)];
        for (int q = 0; q < d; ++q) {
            CHECK(pixels[q] == (H / s) * (H / s), "H=%d s=%d: player %d has %d pixels", H, s, q, pixels[q]);
            CHECK(cells[q] == r * r, "side=%d s=%d: player %d has %d cells", side, s, q, cells[q]);
        }
    }
    // ---- the bit packing at d = 196: seven words, four bits in the last
    {
        const int d = SHAP_MAX_D, Wd = shap_words(d);
        CHECK(Wd == SHAP_MAX_WORDS && Wd == 7 && shap_words(4) == 1 && shap_words(32) == 1 && shap_words(33) == 2 && shap_words(64) == 2, "word counts");
        int valid = 0;
        for (int w = 0; w < Wd; ++w) valid += __builtin_popcount(shap_valid_mask(w, d));
        CHECK(valid == d && shap_valid_mask(5, d) == 0xFFFFFFFFu && shap_valid_mask(6, d) == 0xFu && shap_valid_mask(7, d) == 0u, "valid bits");
        CHECK(shap_valid_mask(0, 4) == 0xFu && shap_valid_mask(0, 32) == 0xFFFFFFFFu && shap_valid_mask(1, 32) == 0u && shap_valid_mask(1, 49) == 0x1FFFFu,
              "valid bits of other sizes");
        for (int q = 0; q < d; ++q) {
            uint32_t words[SHAP_MAX_WORDS] = {0, 0, 0, 0, 0, 0, 0};
            CHECK(shap_word_of(q) == q / 32 && shap_bit_of(q) == (1u << (q % 32)) && shap_word_of(q) < Wd, "player %d: word and bit", q);
            words[shap_word_of(q)] |= shap_bit_of(q);
            int in = 0, out = 0;
            for (int p = 0; p < d; ++p) in += shap_has(words, p) ? 1 : 0;
            CHECK(in == 1 && shap_has(words, q), "player %d: %d members after one bit", q, in);
            uint32_t other[SHAP_MAX_WORDS];
            for (int w = 0; w < Wd; ++w) {
                other[w] = shap_complement(words[w], w, d);
                CHECK((other[w] & ~shap_valid_mask(w, d)) == 0u, "player %d: unused bits set in word %d of the complement", q, w);
                CHECK(shap_complement(other[w], w, d) == words[w], "player %d: the complement of the complement, word %d", q, w);
                out += __builtin_popcount(other[w]);
            }
            CHECK(out == d - 1 && !shap_has(other, q), "player %d: the complement has %d members", q, out);
            ++checks;
        }
    }
    if (failures) {
        printf("shap plan: %d failures\n", failures);
        return 1;
    }
    printf("shap plan: ok (%ld checks)\n", checks);
    return 0;
}
