// Explanations against the truth on PartsWorld: how much of a score map lies on each primitive of the rendered scene.  The contract is in
// include/ppf_hip.h (ppf_part_mass and the view rule PPF_VIEW_SRC); the numpy referee is interpret.part_mass(device=False).  The reference
// has no such pass.
//   * part_mass_kernel: one workgroup of NT_PM threads per score row [S][S].  A lane reads 16-byte score vectors t, t + NT, ... (single
//     elements when S % 4 != 0 or the pointer is not 16-byte aligned), gathers one partmap byte per pixel through the view rule (the
//     column and row tables ((2i + 1) n) / (2S) are built once per workgroup in LDS) and adds max(s, 0) and max(-s, 0) in fp64 (every
//     term exact) to the bin of the pixel's code.  Two forms of the bins, chosen at compile time by PPF_PART_MASS_BINS and picked by
//     measurement (profiles/partcheck_cost.txt: 28.46 us against 34.82 us at 256 rows of 224 x 224, K = 4):
//       1  lane-private bins in LDS (the default), [bin][lane] so that a wave's accesses never share a bank, one read-add-write per pixel;
//       0  registers: NB = 3 + K is a template parameter and every bin is touched by an unrolled compare-and-select, so no array is
//          indexed with the runtime code (a runtime index would put the bins into scratch).
//     Then the lane partials meet by butterfly shuffles per wave and the NT / 64 wave totals are added in wave order by one lane per bin:
//     a fixed order, no floating-point atomics, bit-identical from run to run.
//     What it costs is the gather: 20.86 us without it, next to 17.48 us for ppf_grad_box_mass on the same scores.  Gathering the view's
//     codes into LDS ahead of the sums was tried and was slower (42.54 us) and is gone.
//   PPF_PART_MASS_KO (measurement builds of scripts/bench_partcheck.py, never a result): 1 takes the code from the pixel index in place of
//   the gathered byte; 2 adds every pixel to bin 0 without select chain or LDS bins (the codes are still gathered).
#include <float.h>
#include <limits.h>

#include "ppf_common.h"
#include "ppf_hip.h"

#ifndef PPF_PART_MASS_BINS
#define PPF_PART_MASS_BINS 1
#endif
#ifndef PPF_PART_MASS_KO
#define PPF_PART_MASS_KO 0
#endif

namespace {

constexpr int NT_PM = 512, PM_WAVES = NT_PM / 64;
constexpr int PM_TAB = 2048;                                                  // view columns and rows whose frame column and row are tabulated in LDS
constexpr int PM_MIN_BINS = 4, PM_MAX_BINS = 11;                              // 3 + K, K in [1, 8]

struct PmRow {                                                                // what a workgroup needs of its row
    const float* score;
    const uint8_t* map;
    int S, H, W;
};

__device__ __forceinline__ PmRow pm_row(const float* score, const uint8_t* partmap, int rows_per_img, int S, int H, int W, int* tab) {
    const int r = blockIdx.x;
    for (int x = threadIdx.x; x < S && x < PM_TAB; x += NT_PM) {              // the view rule once per column and row: its 64-bit division stays out of the loops
        tab[x] = PPF_VIEW_SRC(x, W, S);
        tab[PM_TAB + x] = PPF_VIEW_SRC(x, H, S);
    }
    __syncthreads();
    return PmRow{score + (size_t)r * S * S, partmap + (size_t)(r / rows_per_img) * H * W, S, H, W};
}

__device__ __forceinline__ int pm_col(const PmRow& q, const int* tab, int x) { return x < PM_TAB ? tab[x] : PPF_VIEW_SRC(x, q.W, q.S); }
__device__ __forceinline__ int pm_line(const PmRow& q, const int* tab, int y) { return y < PM_TAB ? tab[PM_TAB + y] : PPF_VIEW_SRC(y, q.H, q.S); }

// Walks the row: f(s, code) per pixel, in the lane's fixed order.  Four vectors and their codes are fetched before the first is added: a
// code is a byte load behind an LDS read, and with one vector per iteration that chain's latency stood in every iteration (46.96 us
// against 28.46 us for the LDS bins, profiles/partcheck_cost.txt).  Written out, not left to an unroll pragma: f may hold wave-wide
// operations, and a loop with those is not unrolled with a remainder.
template <int VEC, typename F>
__device__ __forceinline__ void pm_walk(const PmRow& q, const int* tab, F f) {
    constexpr int U = 4;
    const int nv = q.S * q.S / VEC, Sv = q.S / VEC;                           // VEC divides S
    auto fetch = [&](int i, float (&v)[VEC], uint32_t& word) {                // the scores of vector i and their codes, one per byte
        if constexpr (VEC == 4) {
            const float4 t = reinterpret_cast<const float4*>(q.score)[i];
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
            v[0] = q.score[i];
        }
        word = 0;
#if PPF_PART_MASS_KO == 1
#pragma unroll
        for (int k = 0; k < VEC; ++k) word |= (uint32_t)((i + k) & 3) << (8 * k);
#else
        const int y = i / Sv, x0 = (i - y * Sv) * VEC;
        const uint8_t* __restrict__ mrow = q.map + (size_t)pm_line(q, tab, y) * q.W;
#pragma unroll
        for (int k = 0; k < VEC; ++k) word |= (uint32_t)mrow[pm_col(q, tab, x0 + k)] << (8 * k);
#endif
    };
    auto apply = [&](const float (&v)[VEC], uint32_t word) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) f(v[k], (int)((word >> (8 * k)) & 255u));
    };
    int i = threadIdx.x;
    for (; nv - i > (U - 1) * NT_PM; i += U * NT_PM) {                        // nv may be close to 2^31: no sum that could pass it
        float v[U][VEC];
        uint32_t w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) fetch(i + u * NT_PM, v[u], w[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) apply(v[u], w[u]);
    }
    for (; i < nv; i += NT_PM) {
        float v[VEC];
        uint32_t w;
        fetch(i, v, w);
        apply(v, w);
    }
}

// The lane partials of bin j (get(j) -> pos, neg, count) to pos / neg / count [r][NB], and the lane's bad count to nonfinite[r].
template <typename G>
__device__ __forceinline__ void pm_finish(int NB, G get, int bad, double* __restrict__ pos, double* __restrict__ neg, int* __restrict__ count,
                                          int* __restrict__ nonfinite) {
    __shared__ double s_pos[PM_WAVES][PM_MAX_BINS], s_neg[PM_WAVES][PM_MAX_BINS];
    __shared__ int s_cnt[PM_WAVES][PM_MAX_BINS], s_bad[PM_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, r = blockIdx.x;
    for (int j = 0; j < NB; ++j) {
        double p, n;
        int c;
        get(j, p, n, c);
        p = wave_sum_f64(p);
        n = wave_sum_f64(n);
        c = wave_sum_i32(c);
        if ((tid & 63) == 0) { s_pos[wave][j] = p; s_neg[wave][j] = n; s_cnt[wave][j] = c; }
    }
    bad = wave_sum_i32(bad);
    if ((tid & 63) == 0) s_bad[wave] = bad;
    __syncthreads();
    if (tid < NB) {
        double p = s_pos[0][tid], n = s_neg[0][tid];
        int c = s_cnt[0][tid];
        for (int w = 1; w < PM_WAVES; ++w) { p += s_pos[w][tid]; n += s_neg[w][tid]; c += s_cnt[w][tid]; }          // fixed order
        pos[(size_t)r * NB + tid] = p;
        neg[(size_t)r * NB + tid] = n;
        count[(size_t)r * NB + tid] = c;
    }
    if (tid == 0 && nonfinite) {
        int b = s_bad[0];
        for (int w = 1; w < PM_WAVES; ++w) b += s_bad[w];
        nonfinite[r] = b;
    }
}

// bins in registers: the unrolled compare-and-select over the NB bins.  Per bin one compare, one select of the mask 1.0 / 0.0 (its high
// word; the low one is 0 either way) and two fp64 FMAs -- dp * 1.0 + p is p + dp with its one rounding, dp * 0.0 + p is p, and dp is
// finite by then --, and the count is the population count of the compare's wave mask, which the scalar unit adds: a lane's c[] is its
// wave's count.
template <int VEC, int NB>
__global__ __launch_bounds__(NT_PM) void part_mass_select_kernel(const float* __restrict__ score, const uint8_t* __restrict__ partmap, int rows_per_img,
                                                                 int S, int H, int W, double* __restrict__ pos, double* __restrict__ neg,
                                                                 int* __restrict__ count, int* __restrict__ nonfinite) {
    __shared__ int tab[2 * PM_TAB];
    const PmRow q = pm_row(score, partmap, rows_per_img, S, H, W, tab);
    double p[NB], n[NB];
    int c[NB], bad = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) { p[j] = 0.0; n[j] = 0.0; c[j] = 0; }
    auto add = [&](float s, int code) {
        const bool fin = fabsf(s) <= FLT_MAX;                                 // false for inf and NaN
        bad += __popcll(__ballot(!fin || code >= NB));
        const double dp = (fin && s > 0.0f) ? (double)s : 0.0, dn = (fin && s < 0.0f) ? -(double)s : 0.0;
#if PPF_PART_MASS_KO == 2
        p[0] += dp; n[0] += dn; c[0] += code;
#else
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const bool hit = code == j;
            const double m = hit ? 1.0 : 0.0;
            p[j] = __builtin_fma(dp, m, p[j]);
            n[j] = __builtin_fma(dn, m, n[j]);
            c[j] += __popcll(__ballot(hit));
        }
#endif
    };
    pm_walk<VEC>(q, tab, add);
    const bool first = (threadIdx.x & 63) == 0;                               // the counts are per wave already: lane 0 speaks for it
    pm_finish(NB, [&](int j, double& pj, double& nj, int& cj) {
#pragma unroll
        for (int i = 0; i < NB; ++i)                                          // static indices only: j is uniform, the select is free
            if (i == j) { pj = p[i]; nj = n[i]; cj = first ? c[i] : 0; }
    }, first ? bad : 0, pos, neg, count, nonfinite);
}

// lane-private bins in LDS: mass [2 NB][NT_PM] doubles (bin 2 code + (s < 0)), then cnt [NB][NT_PM] ints, then the column table
template <int VEC>
__global__ __launch_bounds__(NT_PM) void part_mass_lds_kernel(const float* __restrict__ score, const uint8_t* __restrict__ partmap, int rows_per_img, int S,
                                                              int H, int W, int NB, double* __restrict__ pos, double* __restrict__ neg,
                                                              int* __restrict__ count, int* __restrict__ nonfinite) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pm_smem[];
    double* mass = reinterpret_cast<double*>(pm_smem);
    int* cnt = reinterpret_cast<int*>(mass + 2 * NB * NT_PM);
    int* tab = cnt + NB * NT_PM;
    const int tid = threadIdx.x;
    for (int j = 0; j < 2 * NB; ++j) mass[j * NT_PM + tid] = 0.0;             // the lane's own bins: no barrier between these and its own adds
    for (int j = 0; j < NB; ++j) cnt[j * NT_PM + tid] = 0;
    const PmRow q = pm_row(score, partmap, rows_per_img, S, H, W, tab);
    int bad = 0;
    pm_walk<VEC>(q, tab, [&](float s, int code) {
        const float a = fabsf(s);
        const bool fin = a <= FLT_MAX;
        bad += (!fin || code >= NB) ? 1 : 0;
#if PPF_PART_MASS_KO == 2
        mass[(s < 0.0f ? NT_PM : 0) + tid] += fin ? (double)a : 0.0;
        cnt[tid] += code;
#else
        if (code < NB) {
            mass[(2 * code + (s < 0.0f ? 1 : 0)) * NT_PM + tid] += fin ? (double)a : 0.0;
            cnt[code * NT_PM + tid] += 1;
        }
#endif
    });
    pm_finish(NB, [&](int j, double& pj, double& nj, int& cj) {
        pj = mass[(2 * j) * NT_PM + tid];
        nj = mass[(2 * j + 1) * NT_PM + tid];
        cj = cnt[j * NT_PM + tid];
    }, bad, pos, neg, count, nonfinite);
}

template <int VEC, int NB>
int part_mass_select(int K, dim3 grid, hipStream_t stream, const float* score, const uint8_t* pm, int rows_per_img, int S, int H, int W, double* pos,
                     double* neg, int* count, int* nonfinite) {
    if constexpr (NB > PM_MAX_BINS) {
        return PPF_ERR_SHAPE;                                                 // not reached: K is checked by the caller
    } else {
        if (3 + K == NB)
            return ppf_launch<part_mass_select_kernel<VEC, NB>>(grid, dim3(NT_PM), 0, stream, "ppf_part_mass", score, pm, rows_per_img, S, H, W, pos, neg,
                                                                 count, nonfinite);
        return part_mass_select<VEC, NB + 1>(K, grid, stream, score, pm, rows_per_img, S, H, W, pos, neg, count, nonfinite);
    }
}

}  // namespace

extern "C" {

int ppf_part_mass(const float* score, const void* partmap_u8, int R, int rows_per_img, int S, int H, int W, int K, double* pos, double* neg, int* count,
                  int* nonfinite, hipStream_t stream) {
    PPF_CHECK_ARG(K >= 1 && K <= 8, PPF_ERR_SHAPE, "ppf_part_mass: K=%d parts outside [1, 8]", K);
    PPF_CHECK_ARG(S >= 1, PPF_ERR_SHAPE, "ppf_part_mass: S=%d (S >= 1)", S);
    PPF_CHECK_ARG(H >= 1 && W >= 1, PPF_ERR_SHAPE, "ppf_part_mass: partmap H=%d x W=%d (both >= 1)", H, W);
    PPF_CHECK_ARG(rows_per_img >= 1, PPF_ERR_SHAPE, "ppf_part_mass: rows_per_img=%d (rows_per_img >= 1)", rows_per_img);
    PPF_CHECK_ARG(R >= 1, PPF_ERR_SHAPE, "ppf_part_mass: R=%d (R >= 1)", R);
    PPF_CHECK_ARG(R % rows_per_img == 0, PPF_ERR_SHAPE, "ppf_part_mass: R=%d rows are not whole images of rows_per_img=%d (R %% rows_per_img != 0)", R,
                  rows_per_img);
    PPF_CHECK_ARG((long long)S * S <= INT_MAX, PPF_ERR_SHAPE, "ppf_part_mass: S=%d: S * S exceeds 2^31 - 1", S);
    PPF_CHECK_ARG((long long)H * W <= INT_MAX, PPF_ERR_SHAPE, "ppf_part_mass: H=%d x W=%d: H * W exceeds 2^31 - 1", H, W);
    PPF_CHECK_ARG(score && partmap_u8 && pos && neg && count, PPF_ERR_ARG,
                  "ppf_part_mass: null pointer (score, partmap, pos, neg, count; only nonfinite may be NULL)");
    const uint8_t* pm = (const uint8_t*)partmap_u8;
    const bool vec = S % 4 == 0 && ((uintptr_t)score & 15) == 0;              // S * S * 4 bytes per row keep every row aligned
    const dim3 grid((unsigned)R);
#if PPF_PART_MASS_BINS == 0
    if (vec) return part_mass_select<4, PM_MIN_BINS>(K, grid, stream, score, pm, rows_per_img, S, H, W, pos, neg, count, nonfinite);
    return part_mass_select<1, PM_MIN_BINS>(K, grid, stream, score, pm, rows_per_img, S, H, W, pos, neg, count, nonfinite);
#else
    const int NB = 3 + K;
    const size_t lds = (size_t)NB * NT_PM * (2 * sizeof(double) + sizeof(int)) + 2 * PM_TAB * sizeof(int);       // 129 024 bytes at K = 8
    if (vec) return ppf_launch<part_mass_lds_kernel<4>>(grid, dim3(NT_PM), lds, stream, "ppf_part_mass", score, pm, rows_per_img, S, H, W, NB, pos, neg,
                                                         count, nonfinite);
    return ppf_launch<part_mass_lds_kernel<1>>(grid, dim3(NT_PM), lds, stream, "ppf_part_mass", score, pm, rows_per_img, S, H, W, NB, pos, neg, count,
                                               nonfinite);
#endif
}

}  // extern "C"
