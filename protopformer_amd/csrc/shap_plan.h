// The index rules of the KernelSHAP pass (shap.hip; the contract is in include/ppf_hip.h) as arithmetic that a host program can check
// without a GPU: which player a pixel and a grid cell belong to, the size of a coalition from its 24-bit draw and the size table, the
// membership of a player from the counting rank of its key, and the packing of a coalition into 32-bit words.  No HIP header is needed
// to include this file; tests/shap_plan_check.cpp compiles it with the host compiler.
#pragma once
#include <stdint.h>

#ifndef PPF_HD
#if defined(__HIPCC__)                                                        // the same definition as order_keys.h's
#define PPF_HD __host__ __device__ __forceinline__
#else
#define PPF_HD inline
#endif
#endif

constexpr int SHAP_MIN_S = 2, SHAP_MAX_S = 14;                                // players per side
constexpr int SHAP_MAX_D = SHAP_MAX_S * SHAP_MAX_S;                           // 196 players
constexpr int SHAP_MAX_WORDS = (SHAP_MAX_D + 31) / 32;                        // 7 words of 32 membership bits
constexpr int SHAP_TABLE_ONE = 1 << 24;                                       // the size table's last entry: the whole distribution
constexpr uint32_t SHAP_COUNTER_BASE = 0x80000001u;                           // Philox counter word 1 of pair 0
constexpr uint32_t SHAP_SIZE_CALL = 0xFFFFFFFFu;                              // Philox counter word 0 of the size draw
constexpr int SHAP_MAX_N = 1 << 30;

PPF_HD int shap_words(int d) { return (d + 31) >> 5; }

// counter word 1 of pair j = n >> 1 of sample n: inside [0x80000001, 0xC0000000] for n < 2^31
PPF_HD uint32_t shap_pair_counter(int n) { return SHAP_COUNTER_BASE + (uint32_t)(n >> 1); }

// player of pixel (y, x) of an H x H image with s players per side (s divides H)
PPF_HD int shap_pixel_player(int y, int x, int H, int s) {
    const int w = H / s;
    return (y / w) * s + x / w;
}
// player of grid cell (gy, gx) when a player is r x r cells
PPF_HD int shap_cell_player(int gy, int gx, int r, int s) { return (gy / r) * s + gx / r; }

// size of the even coalition of a pair from its 24-bit draw u: 1 + #{t in [0, d-3] : table[t] <= u}, in [1, d-1] whatever the table holds
PPF_HD int shap_size(const int32_t* table, int d, uint32_t u) {
    int size = 1;
    for (int t = 0; t + 3 <= d; ++t) size += (int64_t)table[t] <= (int64_t)u ? 1 : 0;
    return size;
}

// does (key_r, r) come before (key_q, q)?  Lexicographic, ascending: unique per player, so the counting rank is a permutation.
PPF_HD bool shap_key_before(uint32_t key_r, int r, uint32_t key_q, int q) { return key_r < key_q || (key_r == key_q && r < q); }

// the counting rank of player q among the d keys
PPF_HD int shap_rank(const uint32_t* keys, int d, int q) {
    int rank = 0;
    const uint32_t kq = keys[q];
    for (int r = 0; r < d; ++r) rank += shap_key_before(keys[r], r, kq, q) ? 1 : 0;
    return rank;
}
// q is in the even coalition of its pair iff its rank is below the size: a uniform subset of that size
PPF_HD bool shap_member(const uint32_t* keys, int d, int q, int size) { return shap_rank(keys, d, q) < size; }

// bit q % 32 of word q / 32
PPF_HD int shap_word_of(int q) { return q >> 5; }
PPF_HD uint32_t shap_bit_of(int q) { return 1u << (q & 31); }
PPF_HD bool shap_has(const uint32_t* words, int q) { return (words[shap_word_of(q)] & shap_bit_of(q)) != 0; }
// the bits of word w that name a player: unused bits stay 0
PPF_HD uint32_t shap_valid_mask(int w, int d) {
    const int left = d - 32 * w;
    return left >= 32 ? 0xFFFFFFFFu : left <= 0 ? 0u : (1u << left) - 1u;
}
// word w of the odd coalition of a pair: the complement of the even one's
PPF_HD uint32_t shap_complement(uint32_t word, int w, int d) { return ~word & shap_valid_mask(w, d); }
