// Faithfulness of an explanation: deletion / insertion curves (Petsiuk et al., RISE, 2018) from what an eval forward leaves on the device.
// Remove the grid cells an explanation names, most important first, and the class probability should fall; show only those cells and it
// should come back.  Three launches; the model forwards between them are the caller's (interpret.faithfulness_curves).  The reference has
// no such pass.
//   * cell_order_kernel: one workgroup of NT threads per (sample, class) row.  In evidence mode the threads lie along the reserved tokens:
//     act_full[b] is [P][T] with T contiguous, so with R = NT / T prototype rows per pass thread tid reads element p0 * T + tid -- one
//     contiguous run per pass -- and keeps the fp64 sum of its own token t = tid % T over the prototypes p = tid / T, + R, + 2R, ...  The R
//     partial sums of a token meet in LDS and are added in ascending slice order by one thread, then rounded once to fp32.  Every product
//     double(w) * double(a) of two fp32 values is exact, and every sum starts from +0 (a sum of -0 terms is +0, as numpy's).
//     The cells are then ranked by counting in LDS as topk_sorted_kernel does (count_before of ppf_select.h): one 64-bit key per cell (tier,
//     then score_key: the score's bits mapped to an ascending integer with -0 == +0 and NaN below -inf), rank = number of cells with a larger
//     key, or the same key and a smaller cell.  The key is made from the fp32 score that is returned, so the order can be verified from it.
//   * patch_perturb_kernel: streaming.  A thread owns one 16-byte vector of x (it never straddles a cell: the patch width is a multiple
//     of 4), reads it and the baseline once and writes it to all S * M copies from registers; counts [S] are wave-uniform loads.
//     Workgroups of 128 threads: 294 of them at B = 1, 3 x 224 x 224.
//   * class_prob_kernel: one wave per row of logits, two passes over the row (maximum, then the sum of expf in fp64), shuffle reductions;
//     only the probability of the asked class is written, the softmax rows never exist.
// Deterministic: no atomics on floating-point data, fixed summation order.
#include <limits.h>
#include <math.h>

#include "ppf_common.h"
#include "ppf_hip.h"
#include "ppf_select.h"

namespace {

constexpr int NT_ORDER = 1024;          // threads of a cell_order workgroup = the largest grid (one thread per cell when ranking)
constexpr int MAX_CELLS = 1024;
constexpr int NT_PERTURB = 128;
constexpr int NT_PROB = 256;            // four rows per workgroup

enum { MODE_EVIDENCE = 0, MODE_ATTENTION = 1, MODE_RANDOM = 2 };

// grid: B * M workgroups of NT_ORDER threads
__global__ __launch_bounds__(NT_ORDER) void cell_order_kernel(const float* __restrict__ act_full, const int* __restrict__ idx,
                                                              const float* __restrict__ token_attn, const float* __restrict__ weight, float scale,
                                                              const int* __restrict__ classes, const long long* __restrict__ image_id, uint64_t seed,
                                                              int mode, int P, int C, int T, int G, int M, int* __restrict__ order,
                                                              int* __restrict__ rank, float* __restrict__ score) {
    __shared__ double part[NT_ORDER];                                         // partial sums, slice-major: part[r * T + t]
    __shared__ unsigned long long key[MAX_CELLS];
    __shared__ float tot[MAX_CELLS];                                          // evidence of reserved token t
    __shared__ int inv[MAX_CELLS];                                            // the smallest reserved token at cell g, INT_MAX if none
    const int tid = threadIdx.x;
    const int row = blockIdx.x, b = row / M;
    const size_t out0 = (size_t)row * G;
    const int c = classes[row];
    if (c < 0 || c >= C) {                                                    // workgroup-uniform
        if (tid < G) { order[out0 + tid] = -1; rank[out0 + tid] = -1; score[out0 + tid] = 0.0f; }
        return;
    }

    float s = 0.0f;
    int tier = 0;
    if (mode == MODE_EVIDENCE) {
        const int R = NT_ORDER / T;                                           // prototype rows per pass (T <= G <= NT_ORDER)
        const int r = tid / T, t = tid - r * T;
        if (r < R && r < P) {
            const float* __restrict__ a = act_full + (size_t)b * P * T + t;
            const float* __restrict__ wrow = weight + (size_t)c * P;
            double acc = 0.0;
#pragma unroll 4
            for (int p = r; p < P; p += R) acc += (double)__fmul_rn(scale, wrow[p]) * (double)a[(size_t)p * T];
            part[tid] = acc;
        }
        if (tid < G) inv[tid] = INT_MAX;
        __syncthreads();
        if (tid < T) {
            const int slices = R < P ? R : P;
            double sum = part[tid];
            for (int q = 1; q < slices; ++q) sum += part[q * T + tid];        // fixed order
            tot[tid] = (float)sum;
            const int g = idx[(size_t)b * T + tid];
            if (g >= 0 && g < G) atomicMin(&inv[g], tid);                     // a cell listed twice takes its smallest token
        }
        __syncthreads();
        if (tid < G) {
            const int t0 = inv[tid];
            tier = t0 == INT_MAX ? 1 : 0;
            s = tier ? token_attn[(size_t)b * G + tid] : tot[t0];
        }
    } else if (tid < G) {
        if (mode == MODE_ATTENTION) {
            s = token_attn[(size_t)b * G + tid];
        } else {
            const uint64_t id = (uint64_t)image_id[b];
            const uint4 w = philox4x32_10(make_uint4((uint32_t)tid, 0u, (uint32_t)id, (uint32_t)(id >> 32)),
                                          make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
            s = (float)(w.x >> 8) * (1.0f / 16777216.0f);                     // exact: 24 bits
        }
    }
    if (tid < G) {
        key[tid] = ((unsigned long long)(1 - tier) << 32) | score_key(s);
        score[out0 + tid] = s;
    }
    __syncthreads();
    if (tid < G) {
        const int rk = count_before(key, G, tid);
        rank[out0 + tid] = rk;
        order[out0 + rk] = tid;                                               // the order is total: every rk in [0, G) is written once
    }
}

// One thread per 16-byte vector of x.  grid: ceil(B * Cc * H * W / 4 / NT_PERTURB)
__global__ __launch_bounds__(NT_PERTURB) void patch_perturb_kernel(const float4* __restrict__ x, const float4* __restrict__ base, float base_const,
                                                                   const int* __restrict__ rank, const int* __restrict__ counts, int S, int insertion,
                                                                   int M, int G, int side, int patch, int W4, int H, long long vec_per_img,
                                                                   long long nvec, float4* __restrict__ out) {
    const long long v = (long long)blockIdx.x * NT_PERTURB + threadIdx.x;
    if (v >= nvec) return;
    const long long b = v / vec_per_img, e = v - b * vec_per_img;            // e = (channel * H + y) * W4 + x4
    const int x4 = (int)(e % W4), y = (int)((e / W4) % H);
    const int g = (y / patch) * side + (x4 * 4) / patch;
    const float4 xv = x[v];
    const float4 bv = base ? base[v] : make_float4(base_const, base_const, base_const, base_const);
    const long long copy = nvec * M;                                          // vectors of one step: out is [S][B][M][vec_per_img]
    for (int m = 0; m < M; ++m) {
        const int r = rank[((size_t)b * M + m) * G + g];
        float4* __restrict__ o = out + ((size_t)b * M + m) * vec_per_img + e;
        for (int st = 0; st < S; ++st) {
            const bool named = r < counts[st];                                // among the first counts[st] cells of the order
            const bool keep = r < 0 || named == (insertion != 0);
            o[(size_t)st * copy] = make_float4(keep ? xv.x : bv.x, keep ? xv.y : bv.y, keep ? xv.z : bv.z, keep ? xv.w : bv.w);
        }
    }
}

// One wave per row.  grid: ceil(R / 4) workgroups of NT_PROB threads
__global__ __launch_bounds__(NT_PROB) void class_prob_kernel(const float* __restrict__ logits, const int* __restrict__ cls, int R, int C,
                                                             float* __restrict__ prob) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (NT_PROB / 64) + (threadIdx.x >> 6);
    if (r >= R) return;                                                       // wave-uniform
    const float* __restrict__ l = logits + (size_t)r * C;
    float mx = -INFINITY;
    bool has_nan = false;
    for (int j = lane; j < C; j += 64) {
        const float v = l[j];
        has_nan |= v != v;
        mx = fmaxf(mx, v);
    }
    mx = wave_max(mx);
    const bool row_nan = __any(has_nan) != 0;                                     // fmaxf drops a NaN: it is carried separately
    double sum = 0.0;
    for (int j = lane; j < C; j += 64) sum += (double)expf(l[j] - mx);        // the second pass hits the cache
    sum = wave_sum_f64(sum);
    if (lane == 0) {
        const int c = cls[r];
        float p = NAN;
        if (c >= 0 && c < C && !row_nan) p = (float)((double)expf(l[c] - mx) / sum);
        prob[r] = p;
    }
}

}  // namespace

extern "C" {

int ppf_cell_order(const float* act_full, const int* idx, const float* token_attn, const float* weight, float scale, const int* classes,
                   const void* image_id_i64, uint64_t seed, int mode, int B, int P, int C, int T, int G, int M, int* order, int* rank, float* score,
                   hipStream_t stream) {
    PPF_CHECK_ARG(mode == MODE_EVIDENCE || mode == MODE_ATTENTION || mode == MODE_RANDOM, PPF_ERR_ARG,
                  "ppf_cell_order: mode=%d must be 0 (evidence), 1 (attention) or 2 (random)", mode);
    PPF_CHECK_ARG(G >= 1 && G <= MAX_CELLS, PPF_ERR_SHAPE, "ppf_cell_order: G=%d grid cells outside [1, %d]", G, MAX_CELLS);
    PPF_CHECK_ARG(M >= 1 && M <= 8, PPF_ERR_SHAPE, "ppf_cell_order: M=%d outside [1, 8] (classes ordered per sample)", M);
    PPF_CHECK_ARG(B >= 1 && C >= 1, PPF_ERR_SHAPE, "ppf_cell_order: bad shape B=%d C=%d (both >= 1)", B, C);
    PPF_CHECK_ARG((long long)B * M <= INT_MAX, PPF_ERR_SHAPE, "ppf_cell_order: B=%d x M=%d rows exceed the grid", B, M);
    PPF_CHECK_ARG(classes && order && rank && score, PPF_ERR_ARG, "ppf_cell_order: null pointer (classes, order, rank, score)");
    if (mode == MODE_EVIDENCE) {
        PPF_CHECK_ARG(T >= 1 && T <= G, PPF_ERR_SHAPE, "ppf_cell_order: T=%d reserved tokens outside [1, G=%d]", T, G);
        PPF_CHECK_ARG(P >= 1, PPF_ERR_SHAPE, "ppf_cell_order: P=%d prototypes (>= 1)", P);
        PPF_CHECK_ARG(act_full && idx && token_attn && weight, PPF_ERR_ARG, "ppf_cell_order: the evidence order needs act_full, idx, token_attn and weight");
    } else if (mode == MODE_ATTENTION) {
        PPF_CHECK_ARG(token_attn != nullptr, PPF_ERR_ARG, "ppf_cell_order: the attention order needs token_attn");
    } else {
        PPF_CHECK_ARG(image_id_i64 != nullptr, PPF_ERR_ARG, "ppf_cell_order: the random order needs image_id");
    }
    return ppf_launch<cell_order_kernel>(dim3((unsigned)(B * M)), dim3(NT_ORDER), 0, stream, "ppf_cell_order", act_full, idx, token_attn, weight, scale,
                                         classes, (const long long*)image_id_i64, seed, mode, P, C, T, G, M, order, rank, score);
}

int ppf_patch_perturb(const float* x, const int* rank, const int* counts, int S, int insertion, const float* baseline, float baseline_const, int B,
                      int M, int Cc, int H, int W, int G, float* out, hipStream_t stream) {
    PPF_CHECK_ARG(B >= 1 && Cc >= 1 && S >= 1, PPF_ERR_SHAPE, "ppf_patch_perturb: bad shape B=%d Cc=%d S=%d (all >= 1)", B, Cc, S);
    PPF_CHECK_ARG(M >= 1 && M <= 8, PPF_ERR_SHAPE, "ppf_patch_perturb: M=%d outside [1, 8]", M);
    PPF_CHECK_ARG(G >= 1 && G <= MAX_CELLS, PPF_ERR_SHAPE, "ppf_patch_perturb: G=%d grid cells outside [1, %d]", G, MAX_CELLS);
    PPF_CHECK_ARG(H >= 1 && H == W, PPF_ERR_SHAPE, "ppf_patch_perturb: H=%d W=%d (square images only)", H, W);
    int side = (int)lround(sqrt((double)G));
    PPF_CHECK_ARG(side * side == G, PPF_ERR_SHAPE, "ppf_patch_perturb: G=%d is not a square grid", G);
    PPF_CHECK_ARG(H % side == 0, PPF_ERR_SHAPE, "ppf_patch_perturb: the grid side %d (G=%d) does not divide H=%d", side, G, H);
    const int patch = H / side;
    PPF_CHECK_ARG(patch % 4 == 0, PPF_ERR_SHAPE, "ppf_patch_perturb: patch width %d (H=%d / side %d) is not a multiple of 4 (16-byte vectors)", patch, H,
                  side);
    PPF_CHECK_ARG(insertion == 0 || insertion == 1, PPF_ERR_ARG, "ppf_patch_perturb: insertion=%d must be 0 (deletion) or 1", insertion);
    PPF_CHECK_ARG(x && rank && counts && out, PPF_ERR_ARG, "ppf_patch_perturb: null pointer (only baseline may be NULL)");
    PPF_CHECK_ARG((((uintptr_t)x | (uintptr_t)out | (uintptr_t)baseline) & 15) == 0, PPF_ERR_ALIGN,
                  "ppf_patch_perturb: x, baseline and out must be 16-byte aligned");
    const long long vec_per_img = (long long)Cc * H * (W / 4), nvec = vec_per_img * B, blocks = (nvec + NT_PERTURB - 1) / NT_PERTURB;
    PPF_CHECK_ARG(blocks <= INT_MAX, PPF_ERR_SHAPE, "ppf_patch_perturb: B=%d x Cc=%d x H=%d x W=%d exceeds the grid", B, Cc, H, W);
    return ppf_launch<patch_perturb_kernel>(dim3((unsigned)blocks), dim3(NT_PERTURB), 0, stream, "ppf_patch_perturb", (const float4*)x,
                                            (const float4*)baseline, baseline_const, rank, counts, S, insertion, M, G, side, patch, W / 4, H, vec_per_img,
                                            nvec, (float4*)out);
}

int ppf_class_prob(const float* logits, const int* cls, int R, int C, float* prob, hipStream_t stream) {
    PPF_CHECK_ARG(R >= 1 && C >= 1, PPF_ERR_SHAPE, "ppf_class_prob: bad shape R=%d C=%d (both >= 1)", R, C);
    PPF_CHECK_ARG(logits && cls && prob, PPF_ERR_ARG, "ppf_class_prob: null pointer");
    const int per = NT_PROB / 64;
    return ppf_launch<class_prob_kernel>(dim3((unsigned)((R + per - 1) / per)), dim3(NT_PROB), 0, stream, "ppf_class_prob", logits, cls, R, C, prob);
}

}  // extern "C"
