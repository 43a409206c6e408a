// The library's one policy for ordering floats and breaking ties, as arithmetic that a host program can check without a GPU: the
// order-preserving integer image of an fp32 value and the "comes before" relation of every ranking kernel (rollout.hip, interp.hip,
// faithful.hip, proto_bank.hip, explain.hip, head.hip; the device code built on it is ppf_select.h).  No HIP header is needed to include
// this file; tests/order_keys_check.cpp compiles it with the host compiler.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)                                                        // the same definition as gemm_layout.h's
#define PPF_HD __host__ __device__ __forceinline__
#else
#define PPF_HD inline
#endif

// ascending integer image of a float: a < b  <=>  order_key(a) < order_key(b) for non-NaN a, b, with -0 one below +0
PPF_HD uint32_t order_key(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
PPF_HD float key_value(uint32_t key) { return __builtin_bit_cast(float, (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key); }

// the key of a score that is ranked: NaN lowest, then -inf .. -0 == +0 .. +inf
PPF_HD uint32_t score_key(float v) {
    if (v != v) return 0u;
    if (v == 0.0f) v = 0.0f;                                                  // -0 ranks as +0: the tie goes to the smaller id
    return order_key(v);                                                      // -inf -> 0x007fffff, above the NaN key
}

// one ascending 64-bit key per (score, index) of a row: a < b  <=>  (score a, index a) comes before (score b, index b) under score_key
// descending, then the smaller index.  Unique per row, so any correct sort of these keys gives the same order (ppf_pixel_order;
// tests/pixel_key_check.cpp).
PPF_HD uint64_t pixel_order_key(float score, uint32_t index) { return ((uint64_t)(~score_key(score)) << 32) | index; }

// does (v, id) come before (w, jd)?  Larger value first, equal values by smaller id; V: float, or an integer key.  A NaN never compares
// greater or equal: with a NaN on either side neither comes before the other.
template <typename V>
PPF_HD bool comes_before(V v, int id, V w, int jd) { return v > w || (v == w && id < jd); }
