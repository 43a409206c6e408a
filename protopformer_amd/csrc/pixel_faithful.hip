// Deletion / insertion curves per pixel (Petsiuk et al., RISE, 2018, as published: pixels are removed in saliency order, and the insertion
// curve starts from a blurred image).  faithful.hip ranks and perturbs the 14 x 14 patch grid; this file does the same for the H * W pixels
// of an image.  Four launches; the model forwards between them are the caller's (interpret.faithfulness_curves).  The reference has no such
// pass.
//   * pixel_order_kernel: a total order of n <= 65536 scores per row.  A row does not fit LDS as 64-bit keys (50 176 x 8 B against 160 KiB),
//     so a workgroup of 1024 threads sorts its row by a stable LSD radix sort, 8 bits per pass, that ping-pongs (key, pixel) pairs through
//     two global buffers of the workgroup's own (400 KB each at 224^2: they stay in the L2).  The 32-bit key is ~score_key: ascending keys
//     are descending scores, and because every pass is stable and the first one reads the pixels in index order, equal keys stay in pixel
//     order -- the low word of pixel_order_key (order_keys.h) never has to be sorted.  Chosen over a bitonic network on the 64-bit keys
//     because the network needs 136 stages over 65 536 padded keys (most of them through global memory) against at most four passes
//     here, and because up-sampled evidence maps have few distinct values: the four digit histograms are taken in ONE read of the scores
//     (they do not depend on the order), and a pass whose digit is the same for the whole row is skipped.  A pass walks the row in tiles
//     of 1024 pixels, one per thread: the lanes of a wave that hold the same digit find each other with eight ballots, the per-wave
//     counts meet in LDS, 256 threads turn them into offsets behind the running base of each digit.  The last pass writes rank[pixel] =
//     position instead of the pair.  Integer LDS atomics only (the histograms): deterministic.
//     The grid is min(R, 256) workgroups that loop over the rows, so the scratch is bounded by 256 rows' worth.
//   * pixel_random_kernel: one Philox call per (image, pixel).
//   * pixel_perturb_kernel: streaming, as patch_perturb_kernel.  A thread owns one 16-byte vector of pixel positions of one image: it
//     reads the M rank vectors once, then per channel the vector of x and of the baseline once, and writes all S * M copies from registers.
//   * gauss_blur_kernel: one launch.  A workgroup stages a 16 x 64 tile with its halo in LDS, runs the horizontal pass into a second LDS
//     array (rounded to fp32 there, as a second launch would round it in memory) and the vertical pass out of it; taps outside the plane
//     are skipped by coordinate.  Every operation is rounded once: plain operators under the contraction pragma below (the HIP headers'
//     __fmul_rn / __fadd_rn are inline functions compiled under the default mode and were fused into an fma here, as ig.hip found).
//     Measured at 768 planes of 224 x 224, r = 5 (profiles/pixel_faithfulness_cost.txt): this form 463 us; a 32-row tile with the taps read
//     from memory in the loops 643 us; the tap loops unrolled over all 33 slots with the taps in registers 517 us (32 rows) and 548 us
//     (16 rows, staging without a division).  The plain loop stayed.
#include <limits.h>

#include "ppf_common.h"
#include "ppf_hip.h"
#include "order_keys.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT_SORT = 1024;           // one pixel per thread and tile
constexpr int NW_SORT = NT_SORT / 64;
constexpr int SORT_WGS = 256;           // workgroups of a launch (one per CU); rows beyond that are looped over
constexpr int MAX_PIXELS = 65536;
constexpr int NT_RANDOM = 256;
constexpr int NT_PERTURB = 128;
constexpr int MAX_M = 8;
constexpr int MAX_RADIUS = 16;
constexpr int BLUR_TH = 16, BLUR_TW = 64, NT_BLUR = 256;

// grid: min(R, SORT_WGS) workgroups of NT_SORT threads; scratch: 4 * n words per workgroup (two buffers of keys [n] + pixels [n])
__global__ __launch_bounds__(NT_SORT) void pixel_order_kernel(const float* __restrict__ score, const int* __restrict__ classes, int R, int n,
                                                              int* __restrict__ rank, uint32_t* scratch) {
    __shared__ uint32_t hist[4][256];                                         // digit counts of pass p, then the running base of each digit
    __shared__ uint32_t cnt[NW_SORT][256];                                    // pixels of the tile with digit d in wave w (zero between tiles)
    __shared__ uint32_t off[NW_SORT][256];                                    // where wave w's pixels with digit d go
    __shared__ int active[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* const buf = scratch + (size_t)blockIdx.x * 4 * (size_t)n;
    for (int i = tid; i < NW_SORT * 256; i += NT_SORT) (&cnt[0][0])[i] = 0;

    for (int row = blockIdx.x; row < R; row += gridDim.x) {                   // everything below is workgroup-uniform control flow
        const float* __restrict__ sc = score + (size_t)row * n;
        int* __restrict__ rk = rank + (size_t)row * n;
        if (classes[row] < 0) {
            for (int i = tid; i < n; i += NT_SORT) rk[i] = -1;
            continue;
        }
        hist[tid >> 8][tid & 255] = 0;                                        // NT_SORT == 4 * 256
        __syncthreads();
        for (int i = tid; i < n; i += NT_SORT) {
            const uint32_t k = ~score_key(sc[i]);
            atomicAdd(&hist[0][k & 255], 1u);
            atomicAdd(&hist[1][(k >> 8) & 255], 1u);
            atomicAdd(&hist[2][(k >> 16) & 255], 1u);
            atomicAdd(&hist[3][k >> 24], 1u);
        }
        __syncthreads();
        if (tid < 4) {                                                        // exclusive scan of pass tid's 256 counts
            uint32_t run = 0;
            int same = 0;
            for (int d = 0; d < 256; ++d) {
                const uint32_t c = hist[tid][d];
                same |= c == (uint32_t)n;
                hist[tid][d] = run;
                run += c;
            }
            active[tid] = !same;                                              // one digit for the whole row: the pass would move nothing
        }
        __syncthreads();
        int last = -1;
        for (int p = 0; p < 4; ++p) last = active[p] ? p : last;
        if (last < 0) {                                                       // all keys equal (or n == 1): pixel order
            for (int i = tid; i < n; i += NT_SORT) rk[i] = i;
            __syncthreads();                                                  // hist and active are rewritten by the next row
            continue;
        }
        bool have = false;                                                    // false: the source is the score row itself, in pixel order
        int cur = 0;                                                          // the buffer that holds the pairs
        for (int p = 0; p <= last; ++p) {
            if (!active[p]) continue;
            const uint32_t* sk = buf + (size_t)cur * 2 * n;
            const uint32_t* si = sk + n;
            uint32_t* dk = buf + (size_t)(cur ^ 1) * 2 * n;
            uint32_t* di = dk + n;
            for (int t0 = 0; t0 < n; t0 += NT_SORT) {
                const int i = t0 + tid;
                const bool valid = i < n;
                uint32_t k = 0, id = (uint32_t)i;
                if (valid) {
                    if (have) { k = sk[i]; id = si[i]; }
                    else k = ~score_key(sc[i]);
                }
                const uint32_t d = (k >> (8 * p)) & 255u;
                unsigned long long peers = __ballot(valid);                   // the valid lanes of this wave with the same digit
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const bool bit = (d >> b) & 1u;
                    const unsigned long long bl = __ballot(bit);
                    peers &= bit ? bl : ~bl;
                }
                const uint32_t before = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
                if (valid && before == 0) cnt[wave][d] = (uint32_t)__popcll(peers);
                __syncthreads();
                if (tid < 256) {
                    uint32_t run = hist[p][tid];
#pragma unroll
                    for (int w = 0; w < NW_SORT; ++w) {
                        const uint32_t c = cnt[w][tid];
                        cnt[w][tid] = 0;
                        off[w][tid] = run;
                        run += c;
                    }
                    hist[p][tid] = run;
                }
                __syncthreads();
                if (valid) {
                    const uint32_t pos = off[wave][d] + before;               // < n: the digit bases partition [0, n)
                    if (p == last) rk[id] = (int)pos;
                    else { dk[pos] = k; di[pos] = id; }
                }
            }
            __syncthreads();                                                  // the pairs are read by other threads in the next pass
            have = true;
            cur ^= 1;
        }
    }
}

// grid: ceil(B * n / NT_RANDOM)
__global__ __launch_bounds__(NT_RANDOM) void pixel_random_kernel(const long long* __restrict__ image_id, uint64_t seed, long long total, int n,
                                                                 float* __restrict__ score) {
    const long long e = (long long)blockIdx.x * NT_RANDOM + threadIdx.x;
    if (e >= total) return;
    const long long b = e / n;
    const uint32_t px = (uint32_t)(e - b * n);
    const uint64_t id = (uint64_t)image_id[b];
    const uint4 w = philox4x32_10(make_uint4(px, 0x80000000u, (uint32_t)id, (uint32_t)(id >> 32)), make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
    score[e] = (float)(w.x >> 8) * (1.0f / 16777216.0f);                      // exact: 24 bits
}

// One thread per 16-byte vector of pixel positions of one image.  grid: ceil(B * H * W / 4 / NT_PERTURB)
__global__ __launch_bounds__(NT_PERTURB) void pixel_perturb_kernel(const float4* __restrict__ x, const float4* __restrict__ base, float base_const,
                                                                   const int4* __restrict__ rank, const int* __restrict__ counts, int S,
                                                                   int insertion, int M, int Cc, long long vec_per_plane, long long nvec,
                                                                   float4* __restrict__ out) {
    const long long v = (long long)blockIdx.x * NT_PERTURB + threadIdx.x;
    if (v >= nvec) return;
    const long long b = v / vec_per_plane, e = v - b * vec_per_plane;         // e = y * W / 4 + x / 4
    int4 r[MAX_M];
#pragma unroll
    for (int m = 0; m < MAX_M; ++m)
        if (m < M) r[m] = rank[((size_t)b * M + m) * vec_per_plane + e];
    const long long vec_per_img = vec_per_plane * Cc;
    const long long copy = vec_per_img * M * (nvec / vec_per_plane);          // vectors of one step: out is [S][B][M][Cc][plane]
    for (int c = 0; c < Cc; ++c) {
        const size_t in = (size_t)b * vec_per_img + (size_t)c * vec_per_plane + e;
        const float4 xv = x[in];
        const float4 bv = base ? base[in] : make_float4(base_const, base_const, base_const, base_const);
#pragma unroll
        for (int m = 0; m < MAX_M; ++m) {
            if (m < M) {
                float4* __restrict__ o = out + ((size_t)b * M + m) * vec_per_img + (size_t)c * vec_per_plane + e;
                for (int st = 0; st < S; ++st) {
                    const int cn = counts[st];
                    const bool ins = insertion != 0;
                    const bool k0 = r[m].x < 0 || (r[m].x < cn) == ins, k1 = r[m].y < 0 || (r[m].y < cn) == ins;
                    const bool k2 = r[m].z < 0 || (r[m].z < cn) == ins, k3 = r[m].w < 0 || (r[m].w < cn) == ins;
                    o[(size_t)st * copy] = make_float4(k0 ? xv.x : bv.x, k1 ? xv.y : bv.y, k2 ? xv.z : bv.z, k3 ? xv.w : bv.w);
                }
            }
        }
    }
}

// grid: (ceil(W / BLUR_TW), ceil(H / BLUR_TH), R) workgroups of NT_BLUR threads
__global__ __launch_bounds__(NT_BLUR) void gauss_blur_kernel(const float* __restrict__ x, const float* __restrict__ taps, int r, int H, int W,
                                                             float* __restrict__ out) {
    __shared__ float in[BLUR_TH + 2 * MAX_RADIUS][BLUR_TW + 2 * MAX_RADIUS];
    __shared__ float mid[BLUR_TH + 2 * MAX_RADIUS][BLUR_TW];
    __shared__ float w[2 * MAX_RADIUS + 1];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * BLUR_TW, y0 = blockIdx.y * BLUR_TH;
    const size_t plane = (size_t)blockIdx.z * H * W;
    const int rows = BLUR_TH + 2 * r, cols = BLUR_TW + 2 * r;
    if (tid < 2 * r + 1) w[tid] = taps[tid];
    for (int i = tid; i < rows * cols; i += NT_BLUR) {
        const int ly = i / cols, lx = i - ly * cols;
        const int gy = y0 - r + ly, gx = x0 - r + lx;
        in[ly][lx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? x[plane + (size_t)gy * W + gx] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < rows * BLUR_TW; i += NT_BLUR) {                     // horizontal: mid[ly][lx] = t[y0 - r + ly][x0 + lx]
        const int ly = i / BLUR_TW, lx = i - ly * BLUR_TW;
        const int gx = x0 + lx;
        float acc = 0.0f;
        for (int d = -r; d <= r; ++d)
            if (gx + d >= 0 && gx + d < W) acc = acc + w[d + r] * in[ly][lx + r + d];
        mid[ly][lx] = acc;
    }
    __syncthreads();
    for (int i = tid; i < BLUR_TH * BLUR_TW; i += NT_BLUR) {                  // vertical
        const int ly = i / BLUR_TW, lx = i - ly * BLUR_TW;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        float acc = 0.0f;
        for (int d = -r; d <= r; ++d)
            if (gy + d >= 0 && gy + d < H) acc = acc + w[d + r] * mid[ly + r + d][lx];
        out[plane + (size_t)gy * W + gx] = acc;
    }
}

int sort_wgs(int R) { return R < SORT_WGS ? R : SORT_WGS; }

}  // namespace

extern "C" {

size_t ppf_pixel_order_scratch_bytes(int R, int n) {
    if (R < 1 || n < 1 || n > MAX_PIXELS) return 0;
    return (size_t)sort_wgs(R) * 4 * (size_t)n * sizeof(uint32_t);
}

int ppf_pixel_order(const float* score, const int* classes, int R, int n, int* rank, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    PPF_CHECK_ARG(R >= 1, PPF_ERR_SHAPE, "ppf_pixel_order: R=%d rows (>= 1)", R);
    PPF_CHECK_ARG(n >= 1 && n <= MAX_PIXELS, PPF_ERR_SHAPE, "ppf_pixel_order: n=%d pixels outside [1, %d]", n, MAX_PIXELS);
    PPF_CHECK_ARG(score && classes && rank && scratch, PPF_ERR_ARG, "ppf_pixel_order: null pointer (score, classes, rank, scratch)");
    const size_t need = ppf_pixel_order_scratch_bytes(R, n);
    PPF_CHECK_ARG(scratch_bytes >= need, PPF_ERR_ARG, "ppf_pixel_order: scratch of %zu bytes, R=%d n=%d needs %zu (ppf_pixel_order_scratch_bytes)",
                  scratch_bytes, R, n, need);
    PPF_CHECK_ARG(((uintptr_t)scratch & 3) == 0, PPF_ERR_ALIGN, "ppf_pixel_order: scratch must be 4-byte aligned");
    return ppf_launch<pixel_order_kernel>(dim3((unsigned)sort_wgs(R)), dim3(NT_SORT), 0, stream, "ppf_pixel_order", score, classes, R, n, rank,
                                          (uint32_t*)scratch);
}

int ppf_pixel_random(const void* image_id_i64, uint64_t seed, int B, int n, float* score, hipStream_t stream) {
    PPF_CHECK_ARG(B >= 1, PPF_ERR_SHAPE, "ppf_pixel_random: B=%d (>= 1)", B);
    PPF_CHECK_ARG(n >= 1 && n <= MAX_PIXELS, PPF_ERR_SHAPE, "ppf_pixel_random: n=%d pixels outside [1, %d]", n, MAX_PIXELS);
    PPF_CHECK_ARG(image_id_i64 && score, PPF_ERR_ARG, "ppf_pixel_random: null pointer");
    const long long total = (long long)B * n, blocks = (total + NT_RANDOM - 1) / NT_RANDOM;
    PPF_CHECK_ARG(blocks <= INT_MAX, PPF_ERR_SHAPE, "ppf_pixel_random: B=%d x n=%d exceeds the grid", B, n);
    return ppf_launch<pixel_random_kernel>(dim3((unsigned)blocks), dim3(NT_RANDOM), 0, stream, "ppf_pixel_random", (const long long*)image_id_i64, seed,
                                           total, n, score);
}

int ppf_pixel_perturb(const float* x, const int* rank, const int* counts, int S, int insertion, const float* baseline, float baseline_const, int B,
                      int M, int Cc, int H, int W, float* out, hipStream_t stream) {
    PPF_CHECK_ARG(B >= 1 && Cc >= 1 && S >= 1, PPF_ERR_SHAPE, "ppf_pixel_perturb: bad shape B=%d Cc=%d S=%d (all >= 1)", B, Cc, S);
    PPF_CHECK_ARG(M >= 1 && M <= MAX_M, PPF_ERR_SHAPE, "ppf_pixel_perturb: M=%d outside [1, %d]", M, MAX_M);
    PPF_CHECK_ARG(H >= 1 && W >= 4 && W % 4 == 0, PPF_ERR_SHAPE, "ppf_pixel_perturb: H=%d W=%d: W must be a multiple of 4 (16-byte vectors)", H, W);
    PPF_CHECK_ARG(insertion == 0 || insertion == 1, PPF_ERR_ARG, "ppf_pixel_perturb: insertion=%d must be 0 (deletion) or 1", insertion);
    PPF_CHECK_ARG(x && rank && counts && out, PPF_ERR_ARG, "ppf_pixel_perturb: null pointer (only baseline may be NULL)");
    PPF_CHECK_ARG((((uintptr_t)x | (uintptr_t)out | (uintptr_t)baseline | (uintptr_t)rank) & 15) == 0, PPF_ERR_ALIGN,
                  "ppf_pixel_perturb: x, baseline, rank and out must be 16-byte aligned");
    const long long vec_per_plane = (long long)H * (W / 4), nvec = vec_per_plane * B, blocks = (nvec + NT_PERTURB - 1) / NT_PERTURB;
    PPF_CHECK_ARG(blocks <= INT_MAX, PPF_ERR_SHAPE, "ppf_pixel_perturb: B=%d x H=%d x W=%d exceeds the grid", B, H, W);
    return ppf_launch<pixel_perturb_kernel>(dim3((unsigned)blocks), dim3(NT_PERTURB), 0, stream, "ppf_pixel_perturb", (const float4*)x,
                                            (const float4*)baseline, baseline_const, (const int4*)rank, counts, S, insertion, M, Cc, vec_per_plane, nvec,
                                            (float4*)out);
}

int ppf_gauss_blur(const float* x, const float* taps, int r, int R, int H, int W, float* out, hipStream_t stream) {
    PPF_CHECK_ARG(r >= 1 && r <= MAX_RADIUS, PPF_ERR_SHAPE, "ppf_gauss_blur: r=%d outside [1, %d]", r, MAX_RADIUS);
    PPF_CHECK_ARG(R >= 1 && H >= 1 && W >= 1, PPF_ERR_SHAPE, "ppf_gauss_blur: bad shape R=%d H=%d W=%d (all >= 1)", R, H, W);
    PPF_CHECK_ARG(x && taps && out, PPF_ERR_ARG, "ppf_gauss_blur: null pointer");
    PPF_CHECK_ARG(x != out, PPF_ERR_ARG, "ppf_gauss_blur: out must not be x (neighbours are read after they would be written)");
    const long long gx = (W + BLUR_TW - 1) / BLUR_TW, gy = (H + BLUR_TH - 1) / BLUR_TH;
    PPF_CHECK_ARG(gy <= 65535 && R <= 65535, PPF_ERR_SHAPE, "ppf_gauss_blur: R=%d planes or H=%d exceed the grid (65535 planes, %d rows)", R, H,
                  65535 * BLUR_TH);
    return ppf_launch<gauss_blur_kernel>(dim3((unsigned)gx, (unsigned)gy, (unsigned)R), dim3(NT_BLUR), 0, stream, "ppf_gauss_blur", x, taps, r, H, W, out);
}

}  // extern "C"
