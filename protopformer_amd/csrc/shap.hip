// KernelSHAP (Lundberg & Lee, 2017) on grid cells: Shapley values of d = s x s square players of an image by the sampled least-squares
// fit under the efficiency constraint, with the paired sampling of Covert & Lee (2021).  It needs forwards only, as RISE does; the
// forwards are the caller's.  Coalitions, masked images and the Gram matrix are integer-exact (the contract is in include/ppf_hip.h, the
// index rules in shap_plan.h), so every kernel but the solve and the numpy referees (interpret.shap_*) agree bit for bit.  The reference
// has no such pass.
//   * shap_coalitions_kernel: a workgroup per (image, pair).  The keys of the d players come from ceil(d / 4) Philox calls into LDS, the
//     size from one more call and a counted barrier over the size table; a thread owns one player and counts the keys before its own (a
//     counting rank, as the other ranking kernels: no atomics); a wave's ballot is two coalition words, and the odd coalition of the
//     pair is their complement.
//   * shap_apply_kernel: streaming and write-bound, as patch_perturb_kernel and rise_apply_kernel.  A workgroup lies inside one image and
//     stages the coalition words of its samples in LDS, in stages of SHAP_STAGE samples.  A thread owns one 16-byte vector position
//     (y, x4) of one channel (rise_apply_kernel's three channels per thread pay there for a mask numerator computed once; here there
//     is nothing to share but a bit, and three channels per thread measured slower, 190 - 195 against 163 - 187 us for a 1 GiB chunk on
//     the machines tried: -DPPF_SHAP_CH=3, profiles/shap_cost.txt) and with it ONE player
//     (a player's width is a multiple of 4): its word and bit are taken once, x and the baseline are read once, and every copy is a
//     select written from registers.  Philox is never run here.
//   * shap_gram_kernel: a workgroup per image.  A tile of GRAM_TILE samples is transposed in LDS into one bit-column per player; the Gram
//     entry of a pair of players is the popcount of the AND of their columns (integer adds only, N tiled), and the right-hand sides are
//     the fp64 sums over the samples in ascending order that a column selects.
//   * shap_solve_kernel: a workgroup per image, fp64.  A left-looking Cholesky whose factor lives in the global scratch, column-major so
//     that a thread (one per row) reads and writes its own elements; only the pivot's row is staged in LDS.  One factorisation serves the
//     M + 1 right-hand sides, which are solved in LDS column by column.  Fixed summation order, no atomics: repeats are bit-identical.
#include <limits.h>
#include <math.h>

#include "ppf_common.h"
#include "ppf_hip.h"
#include "shap_plan.h"

namespace {

constexpr int NT_SHAP = 256;            // >= SHAP_MAX_D: a thread per player (coalitions) and per matrix row (solve)
constexpr int NT_APPLY = 256;           // threads of an apply workgroup (128, the size of patch_perturb_kernel, measured the same to 1 %)
constexpr int SHAP_STAGE = 512;         // samples staged in LDS at a time by the apply kernel: 512 * 7 words = 14 KiB (eight workgroups per CU)
#ifndef PPF_SHAP_CH
#define PPF_SHAP_CH 1
#endif
constexpr int SHAP_CH = PPF_SHAP_CH;    // channels a thread of the apply kernel owns (-DPPF_SHAP_CH=3: a measurement build of scripts/bench_shap.py)
constexpr int GRAM_TILE = 1024;         // samples of one Gram tile
constexpr int GRAM_TW = GRAM_TILE / 32; // words of one bit-column
constexpr int GRAM_COL = GRAM_TW + 1;   // column stride in words: odd, so the columns of consecutive players start in different banks
constexpr int GRAM_RAW = 8;             // words per sample of the staging area: >= SHAP_MAX_WORDS (coalition words), >= 8 (class values)
constexpr int SHAP_MAX_M = 8;
static_assert(NT_SHAP >= SHAP_MAX_D && GRAM_RAW >= SHAP_MAX_WORDS && GRAM_RAW >= SHAP_MAX_M, "thread and staging sizes");

// grid: B * N / 2 workgroups, one per (image, pair)
__global__ __launch_bounds__(NT_SHAP) void shap_coalitions_kernel(const long long* __restrict__ image_id, uint64_t seed, const int* __restrict__ table,
                                                                  int N, int d, uint32_t* __restrict__ coal) {
    __shared__ uint32_t keys[NT_SHAP];
    const int tid = threadIdx.x, half = N >> 1;
    const int b = blockIdx.x / half, j = blockIdx.x - b * half;
    const uint64_t id = (uint64_t)image_id[b];
    const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t c1 = shap_pair_counter(2 * j);
    if (tid * 4 < d) {                                                         // call tid: the keys of players 4 tid .. 4 tid + 3 (< NT_SHAP)
        const uint4 w = philox4x32_10(make_uint4((uint32_t)tid, c1, (uint32_t)id, (uint32_t)(id >> 32)), key);
        keys[4 * tid + 0] = w.x; keys[4 * tid + 1] = w.y; keys[4 * tid + 2] = w.z; keys[4 * tid + 3] = w.w;
    }
    const uint4 ws = philox4x32_10(make_uint4(SHAP_SIZE_CALL, c1, (uint32_t)id, (uint32_t)(id >> 32)), key);      // workgroup-uniform
    const long long u = (long long)(ws.x >> 8);
    const bool below = tid + 3 <= d ? (long long)table[tid] <= u : false;      // shap_size's sum, a term per thread
    const int size = 1 + __syncthreads_count(below ? 1 : 0);                   // the barrier also publishes the keys
    const bool in = tid < d ? shap_member(keys, d, tid, size) : false;
    const unsigned long long ballot = __ballot(in ? 1 : 0);                    // players 64 wave .. 64 wave + 63
    const int lane = tid & 63, w = 2 * (tid >> 6) + lane, Wd = shap_words(d);
    if (lane < 2 && w < Wd) {
        const uint32_t word = (uint32_t)(ballot >> (32 * lane));
        uint32_t* __restrict__ o = coal + ((size_t)b * N + 2 * (size_t)j) * Wd + w;
        o[0] = word;
        o[Wd] = shap_complement(word, w, d);
    }
}

// grid: B * groups * blocks_per_img workgroups; a workgroup lies inside one (image, channel group)
__global__ __launch_bounds__(NT_APPLY) void shap_apply_kernel(const float4* __restrict__ x, const float4* __restrict__ base, float base_const,
                                                             const uint32_t* __restrict__ coal, int N, int n0, int Nc, int s, int Wd, int B, int Cc, int H,
                                                             int W4, int blocks_per_img, int groups, float4* __restrict__ out) {
    __shared__ uint32_t cw[SHAP_STAGE * SHAP_MAX_WORDS];
    const int blk = blockIdx.x % blocks_per_img, bg = blockIdx.x / blocks_per_img;
    const int b = bg / groups, ch0 = (bg - b * groups) * SHAP_CH;
    const int v = blk * NT_APPLY + threadIdx.x;                                 // vector position inside a channel plane
    const int plane = H * W4;
    const bool live = v < plane;
    const int y = live ? v / W4 : 0, x0 = live ? (v - y * W4) * 4 : 0;
    const int q = shap_pixel_player(y, x0, H, s);                              // the four pixels of the vector share it
    const int qw = shap_word_of(q);
    const uint32_t qb = shap_bit_of(q);
    float4 xv[SHAP_CH], bv[SHAP_CH];
#pragma unroll
    for (int c = 0; c < SHAP_CH; ++c) {
        const bool on = live && ch0 + c < Cc;
        const size_t at = ((size_t)b * Cc + ch0 + c) * plane + v;
        xv[c] = on ? x[at] : make_float4(0.f, 0.f, 0.f, 0.f);
        bv[c] = on && base ? base[at] : make_float4(base_const, base_const, base_const, base_const);
    }
    const size_t img = (size_t)Cc * plane, copy = img * B;                     // vectors of one image, of one sample's batch
    for (int s0 = 0; s0 < Nc; s0 += SHAP_STAGE) {
        const int count = min(SHAP_STAGE, Nc - s0);
        // Measurement build (scripts/bench_shap.py --variant): -DPPF_SHAP_KNOCKOUT=1 drops the staging and its barriers and takes the
        // membership from the parity of player and sample.  It is no result; the library is built without the switch.
#ifndef PPF_SHAP_KNOCKOUT
        __syncthreads();                                                       // the previous stage has been read
        const uint32_t* __restrict__ src = coal + ((size_t)b * N + n0 + s0) * Wd;       // samples n0 + s0 .. of image b: count * Wd words in a row
        for (int e = threadIdx.x; e < count * Wd; e += NT_APPLY) cw[e] = src[e];
        __syncthreads();
#endif
        if (!live) continue;
        for (int k = 0; k < count; ++k) {
#ifdef PPF_SHAP_KNOCKOUT
            const bool in = ((q + k) & 1) != 0;
#else
            const bool in = (cw[k * Wd + qw] & qb) != 0;
#endif
            float4* __restrict__ o = out + (size_t)(s0 + k) * copy + (size_t)b * img + (size_t)ch0 * plane + v;
#pragma unroll
            for (int c = 0; c < SHAP_CH; ++c) {
                if (ch0 + c >= Cc) break;                                      // workgroup-uniform
                // component by component: a select between the two float4 arrays becomes a select of addresses, and the arrays go to scratch
                o[(size_t)c * plane] = make_float4(in ? xv[c].x : bv[c].x, in ? xv[c].y : bv[c].y, in ? xv[c].z : bv[c].z, in ? xv[c].w : bv[c].w);
            }
        }
    }
}

// grid: B workgroups
__global__ __launch_bounds__(NT_SHAP) void shap_gram_kernel(const uint32_t* __restrict__ coal, const float* __restrict__ val, const float* __restrict__ v0,
                                                            int B, int N, int M, int d, int Wd, int* __restrict__ A, double* __restrict__ bvec) {
    __shared__ uint32_t col[SHAP_MAX_D * GRAM_COL];                            // col[i * GRAM_COL + w]: bit k = player i in sample t0 + 32 w + k
    __shared__ uint32_t raw[GRAM_TILE * GRAM_RAW];                             // the tile's coalition words, then its class values
    float* vt = reinterpret_cast<float*>(raw);
    const int b = blockIdx.x, tid = threadIdx.x;
    int* __restrict__ Ab = A + (size_t)b * d * d;
    double* __restrict__ bb = bvec + (size_t)b * M * d;
    for (int t0 = 0; t0 < N; t0 += GRAM_TILE) {
        const int count = min(GRAM_TILE, N - t0), nw = (count + 31) >> 5;
        __syncthreads();                                                       // the previous tile has been read
        const uint32_t* __restrict__ src = coal + ((size_t)b * N + t0) * Wd;
        for (int e = tid; e < count * Wd; e += NT_SHAP) raw[e] = src[e];
        __syncthreads();
        for (int e = tid; e < nw * d; e += NT_SHAP) {                          // consecutive threads: consecutive players, one LDS word for 32 of them
            const int w = e / d, i = e - w * d, kn = min(32, count - 32 * w);
            uint32_t bits = 0;
            for (int k = 0; k < kn; ++k) bits |= ((raw[(32 * w + k) * Wd + shap_word_of(i)] >> (i & 31)) & 1u) << k;
            col[i * GRAM_COL + w] = bits;
        }
        __syncthreads();                                                       // the columns are written, the coalition words read
        for (int e = tid; e < count * M; e += NT_SHAP) vt[e] = val[((size_t)(t0 + e / M) * B + b) * M + e % M];
        for (int e = tid; e < d * d; e += NT_SHAP) {                           // the thread that owns a pair owns it in every tile
            const int i = e / d, j = e - i * d;
            int c = 0;
            for (int w = 0; w < nw; ++w) c += __popc(col[i * GRAM_COL + w] & col[j * GRAM_COL + w]);
            Ab[e] = t0 ? Ab[e] + c : c;
        }
        __syncthreads();                                                       // the values are written
        for (int e = tid; e < M * d; e += NT_SHAP) {
            const int m = e / d, i = e - m * d;
            const double from = (double)v0[(size_t)b * M + m];
            double acc = t0 ? bb[e] : 0.0;
            for (int k = 0; k < count; ++k)                                    // n ascending: one rounded subtract and one rounded add per term
                if ((col[i * GRAM_COL + (k >> 5)] >> (k & 31)) & 1u) acc += (double)vt[k * M + m] - from;
            bb[e] = acc;
        }
    }
}

// grid: B workgroups.  Lt is the scratch [B][d][d]: Lt[k * d + i] = L[i][k], so column k is contiguous and thread i touches its own row only.
__global__ __launch_bounds__(NT_SHAP) void shap_solve_kernel(const int* __restrict__ A, const double* __restrict__ bvec, const float* __restrict__ v0,
                                                             const float* __restrict__ v1, int M, int d, int s, int r, int side, int G, double* Lt,
                                                             double* __restrict__ phi, float* __restrict__ cell, int* __restrict__ bad) {
    __shared__ double row[SHAP_MAX_D];                                         // L[j][0 .. j-1], the pivot's row
    __shared__ double diag[SHAP_MAX_D];                                        // L[j][j]
    __shared__ double rhs[(SHAP_MAX_M + 1) * SHAP_MAX_D];                      // b_0 .. b_{M-1} and the ones vector; solved in place
    __shared__ double sums[SHAP_MAX_M + 1], delta[SHAP_MAX_M], pivot;
    __shared__ int rowbad[SHAP_MAX_M];
    const int b = blockIdx.x, tid = threadIdx.x, R = M + 1;
    const int* __restrict__ Ab = A + (size_t)b * d * d;
    double* L = Lt + (size_t)b * d * d;
    double* __restrict__ pb = phi + (size_t)b * M * d;
    float* __restrict__ cb = cell + (size_t)b * M * G;
    bool singular = false;
    for (int j = 0; j < d; ++j) {
        for (int k = tid; k < j; k += NT_SHAP) row[k] = L[(size_t)k * d + j];
        __syncthreads();
        double acc = 0.0;
        if (tid >= j && tid < d) {
            acc = (double)Ab[(size_t)tid * d + j];
            for (int k = 0; k < j; ++k) acc -= L[(size_t)k * d + tid] * row[k];          // k ascending: the fixed order
            if (tid == j) pivot = acc;
        }
        __syncthreads();
        const double p = pivot;                                                // workgroup-uniform from here
        if (!(p > 0.0)) { singular = true; break; }                            // <= 0 or NaN
        const double l = sqrt(p);
        if (tid == j) { L[(size_t)j * d + j] = l; diag[j] = l; }
        else if (tid > j && tid < d) L[(size_t)j * d + tid] = acc / l;
        __syncthreads();                                                       // column j is written before the next pivot's row is staged
    }
    if (singular) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        if (tid == 0) bad[b] = 1;
        for (int e = tid; e < M * d; e += NT_SHAP) pb[e] = nan;
        for (int e = tid; e < M * G; e += NT_SHAP) cb[e] = (float)nan;
        return;
    }
    if (tid == 0) bad[b] = 0;
    if (tid < SHAP_MAX_M) rowbad[tid] = 0;
    __syncthreads();
    for (int e = tid; e < R * d; e += NT_SHAP) {
        const int m = e / d, i = e - m * d;
        const double v = m < M ? bvec[((size_t)b * M + m) * d + i] : 1.0;
        rhs[m * SHAP_MAX_D + i] = v;
        if (!isfinite(v)) rowbad[m] = 1;                                       // every writer stores the same value
    }
    if (tid < M) {
        const double dl = (double)v1[(size_t)b * M + tid] - (double)v0[(size_t)b * M + tid];
        delta[tid] = dl;
        if (!isfinite(dl)) rowbad[tid] = 1;
    }
    __syncthreads();
    for (int j = 0; j < d; ++j) {                                              // L z = b, column by column: z_i loses its terms in j ascending
        if (tid < R) rhs[tid * SHAP_MAX_D + j] /= diag[j];
        __syncthreads();
        const int left = d - j - 1;
        for (int e = tid; e < R * left; e += NT_SHAP) {
            const int m = e / left, i = j + 1 + (e - m * left);
            rhs[m * SHAP_MAX_D + i] -= L[(size_t)j * d + i] * rhs[m * SHAP_MAX_D + j];
        }
        __syncthreads();
    }
    for (int j = d - 1; j >= 0; --j) {                                         // L^T x = z: x_i loses its terms in j descending
        if (tid < R) rhs[tid * SHAP_MAX_D + j] /= diag[j];
        __syncthreads();
        for (int e = tid; e < R * j; e += NT_SHAP) {
            const int m = e / j, i = e - m * j;
            rhs[m * SHAP_MAX_D + i] -= L[(size_t)i * d + j] * rhs[m * SHAP_MAX_D + j];
        }
        __syncthreads();
    }
    if (tid < R) {
        double sum = 0.0;
        for (int i = 0; i < d; ++i) sum += rhs[tid * SHAP_MAX_D + i];          // i ascending
        sums[tid] = sum;
    }
    __syncthreads();
    for (int e = tid; e < M * d; e += NT_SHAP) {                               // phi_m = x_m - y (sum x_m - delta_m) / sum y
        const int m = e / d, i = e - m * d;
        const double t = (sums[m] - delta[m]) / sums[M];
        double p = rhs[m * SHAP_MAX_D + i] - rhs[M * SHAP_MAX_D + i] * t;
        if (rowbad[m]) p = __longlong_as_double(0x7ff8000000000000LL);
        rhs[m * SHAP_MAX_D + i] = p;                                           // read by this thread alone so far
        pb[e] = p;
    }
    __syncthreads();
    const double rr = (double)(r * r);
    for (int e = tid; e < M * G; e += NT_SHAP) {
        const int m = e / G, g = e - m * G, gy = g / side, gx = g - gy * side;
        cb[e] = (float)(rhs[m * SHAP_MAX_D + shap_cell_player(gy, gx, r, s)] / rr);
    }
}

// the sizes every entry point shares; d and Wd on success
int shap_sizes(const char* who, int s, int N, int* d, int* Wd) {
    PPF_CHECK_ARG(s >= SHAP_MIN_S && s <= SHAP_MAX_S, PPF_ERR_SHAPE, "%s: s=%d players per side outside [%d, %d]", who, s, SHAP_MIN_S, SHAP_MAX_S);
    PPF_CHECK_ARG(N >= 2 && N <= SHAP_MAX_N && N % 2 == 0, PPF_ERR_SHAPE, "%s: N=%d samples must be even and lie in [2, 2^30]", who, N);
    *d = s * s;
    *Wd = shap_words(*d);
    return 0;
}

}  // namespace

extern "C" {

int ppf_shap_coalitions(const void* image_id_i64, uint64_t seed, const int* table, int B, int N, int s, void* coal_u32, hipStream_t stream) {
    int d = 0, Wd = 0;
    if (int rc = shap_sizes("ppf_shap_coalitions", s, N, &d, &Wd)) return rc;
    PPF_CHECK_ARG(B >= 1, PPF_ERR_SHAPE, "ppf_shap_coalitions: B=%d (>= 1)", B);
    PPF_CHECK_ARG(image_id_i64 && table && coal_u32, PPF_ERR_ARG, "ppf_shap_coalitions: null pointer (image_id, table, coal)");
    const long long blocks = (long long)B * (N / 2);
    PPF_CHECK_ARG(blocks <= INT_MAX, PPF_ERR_SHAPE, "ppf_shap_coalitions: B=%d x N=%d / 2 pairs exceed the grid", B, N);
    return ppf_launch<shap_coalitions_kernel>(dim3((unsigned)blocks), dim3(NT_SHAP), 0, stream, "ppf_shap_coalitions", (const long long*)image_id_i64, seed,
                                              table, N, d, (uint32_t*)coal_u32);
}

int ppf_shap_apply(const float* x, const void* coal_u32, int N, int n0, int Nc, int s, const float* baseline, float baseline_const, int B, int Cc, int H,
                   int W, float* out, hipStream_t stream) {
    int d = 0, Wd = 0;
    if (int rc = shap_sizes("ppf_shap_apply", s, N, &d, &Wd)) return rc;
    PPF_CHECK_ARG(H >= 1 && H == W, PPF_ERR_SHAPE, "ppf_shap_apply: H=%d W=%d (square images only)", H, W);
    PPF_CHECK_ARG(H % s == 0 && (H / s) % 4 == 0, PPF_ERR_SHAPE,
                  "ppf_shap_apply: s=%d must divide H=%d into players whose width is a multiple of 4 (16-byte vectors)", s, H);
    PPF_CHECK_ARG(B >= 1 && Cc >= 1, PPF_ERR_SHAPE, "ppf_shap_apply: bad shape B=%d Cc=%d (both >= 1)", B, Cc);
    PPF_CHECK_ARG(n0 >= 0 && Nc >= 1 && (long long)n0 + Nc <= N, PPF_ERR_SHAPE, "ppf_shap_apply: samples n0=%d .. n0 + Nc=%d - 1 outside [0, N=%d)", n0, Nc,
                  N);
    PPF_CHECK_ARG(x && coal_u32 && out, PPF_ERR_ARG, "ppf_shap_apply: null pointer (only baseline may be NULL)");
    PPF_CHECK_ARG((((uintptr_t)x | (uintptr_t)out | (uintptr_t)baseline) & 15) == 0, PPF_ERR_ALIGN,
                  "ppf_shap_apply: x, baseline and out must be 16-byte aligned");
    PPF_CHECK_ARG((long long)H * (W / 4) <= INT_MAX - NT_APPLY, PPF_ERR_SHAPE, "ppf_shap_apply: H=%d x W=%d exceeds a channel plane of 2^31 vectors", H, W);
    const int W4 = W / 4, blocks_per_img = (H * W4 + NT_APPLY - 1) / NT_APPLY, groups = Cc / SHAP_CH + (Cc % SHAP_CH != 0);
    const long long per_img = (long long)groups * blocks_per_img, blocks = per_img <= INT_MAX ? per_img * B : per_img;     // no overflow: both < 2^31
    PPF_CHECK_ARG(blocks <= INT_MAX, PPF_ERR_SHAPE, "ppf_shap_apply: B=%d x Cc=%d x H=%d x W=%d exceeds the grid", B, Cc, H, W);
    return ppf_launch<shap_apply_kernel>(dim3((unsigned)blocks), dim3(NT_APPLY), 0, stream, "ppf_shap_apply", (const float4*)x, (const float4*)baseline,
                                         baseline_const, (const uint32_t*)coal_u32, N, n0, Nc, s, Wd, B, Cc, H, W4, blocks_per_img, groups, (float4*)out);
}

int ppf_shap_gram(const void* coal_u32, const float* val, const float* v0, int B, int N, int M, int s, int* A, double* bvec, hipStream_t stream) {
    int d = 0, Wd = 0;
    if (int rc = shap_sizes("ppf_shap_gram", s, N, &d, &Wd)) return rc;
    PPF_CHECK_ARG(B >= 1, PPF_ERR_SHAPE, "ppf_shap_gram: B=%d (>= 1)", B);
    PPF_CHECK_ARG(M >= 1 && M <= SHAP_MAX_M, PPF_ERR_SHAPE, "ppf_shap_gram: M=%d outside [1, %d]", M, SHAP_MAX_M);
    PPF_CHECK_ARG(coal_u32 && val && v0 && A && bvec, PPF_ERR_ARG, "ppf_shap_gram: null pointer");
    return ppf_launch<shap_gram_kernel>(dim3((unsigned)B), dim3(NT_SHAP), 0, stream, "ppf_shap_gram", (const uint32_t*)coal_u32, val, v0, B, N, M, d, Wd, A,
                                        bvec);
}

size_t ppf_shap_solve_scratch_bytes(int B, int d) {
    if (B < 1 || d < SHAP_MIN_S * SHAP_MIN_S || d > SHAP_MAX_D) return 0;
    return (size_t)B * d * d * sizeof(double);
}

int ppf_shap_solve(const int* A, const double* bvec, const float* v0, const float* v1, int B, int M, int s, int G, void* scratch, size_t scratch_bytes,
                   double* phi, float* cell, int* bad, hipStream_t stream) {
    PPF_CHECK_ARG(s >= SHAP_MIN_S && s <= SHAP_MAX_S, PPF_ERR_SHAPE, "ppf_shap_solve: s=%d players per side outside [%d, %d]", s, SHAP_MIN_S, SHAP_MAX_S);
    PPF_CHECK_ARG(B >= 1, PPF_ERR_SHAPE, "ppf_shap_solve: B=%d (>= 1)", B);
    PPF_CHECK_ARG(M >= 1 && M <= SHAP_MAX_M, PPF_ERR_SHAPE, "ppf_shap_solve: M=%d outside [1, %d]", M, SHAP_MAX_M);
    PPF_CHECK_ARG(G >= 1 && G <= 1024, PPF_ERR_SHAPE, "ppf_shap_solve: G=%d grid cells outside [1, 1024]", G);
    const int side = (int)lround(sqrt((double)G));
    PPF_CHECK_ARG(side * side == G, PPF_ERR_SHAPE, "ppf_shap_solve: G=%d is not a square grid", G);
    PPF_CHECK_ARG(side % s == 0, PPF_ERR_SHAPE, "ppf_shap_solve: s=%d players per side do not divide the grid side %d (G=%d)", s, side, G);
    PPF_CHECK_ARG(A && bvec && v0 && v1 && scratch && phi && cell && bad, PPF_ERR_ARG, "ppf_shap_solve: null pointer");
    const size_t need = ppf_shap_solve_scratch_bytes(B, s * s);
    PPF_CHECK_ARG(scratch_bytes >= need, PPF_ERR_SHAPE, "ppf_shap_solve: scratch of %zu bytes, %zu needed (ppf_shap_solve_scratch_bytes)", scratch_bytes,
                  need);
    PPF_CHECK_ARG(((uintptr_t)scratch & 7) == 0, PPF_ERR_ALIGN, "ppf_shap_solve: scratch must be 8-byte aligned");
    return ppf_launch<shap_solve_kernel>(dim3((unsigned)B), dim3(NT_SHAP), 0, stream, "ppf_shap_solve", A, bvec, v0, v1, M, s * s, s, side / s, side, G,
                                         (double*)scratch, phi, cell, bad);
}

}  // extern "C"
