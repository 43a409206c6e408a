// RISE (Petsiuk et al., 2018): the model-agnostic saliency the deletion / insertion metric was published with.  N random masks per image,
// the class probability of every masked image, saliency = the probability-weighted mean mask.  The masks are integer-exact (the contract
// is in include/ppf_hip.h): a binary grid of L x L nodes, L = s + 2, drawn from Philox keyed by (seed, image id, mask), bilinearly
// up-sampled with node spacing c = ceil(H / s) and shifted by (dy, dx) in [0, c)^2.  The mask value of a pixel is K / c^2 with an integer
// numerator K, so every kernel below and the numpy referees (interpret.rise_*) agree bit for bit.  The reference has no such pass.
//   * rise_nodes_kernel: one thread per Philox call: call k of mask n yields nodes 4k .. 4k+3, the call after the last node word the shift.
//   * rise_apply_kernel: streaming and write-bound, as patch_perturb_kernel.  A workgroup lies inside one image and stages the node rows
//     (one 16-bit word per node row) and shifts of its masks in LDS, in stages of RISE_STAGE masks.  A thread owns one 16-byte vector
//     position (y, x4) in up to three channels: x and the baseline are read once, the mask of the four pixels is computed once per mask
//     (no division in the loop: y / c and x / c are taken once, the shift only carries), and the copies are written from registers.
//     Philox is never run here: the node table is read.
//   * rise_saliency_kernel: a thread owns four pixels of one image and keeps their fp64 sums for all M classes; masks ascending, regenerated
//     from the staged node rows, never stored at pixel resolution; the probabilities are workgroup-uniform loads.
//   * rise_cell_kernel: a thread owns one grid cell of one image and walks the masks in ascending order; the integer mass W of a cell is
//     summed row by row (the sum over x of one node row's interpolation, then the interpolation in y), order-free because it is integer.
// Deterministic: no floating-point atomics, fixed summation order (n ascending).
#include <limits.h>
#include <math.h>

#include "ppf_common.h"
#include "ppf_hip.h"

// The blend of the apply kernel is four roundings, as numpy's.  It is written with plain operators under this pragma: __fmul_rn / __fadd_rn
// are inline functions of the HIP headers, compiled under the default contraction mode, and were fused into an fma after inlining.
#pragma clang fp contract(off)

namespace {

constexpr int NT_RISE = 256;
constexpr int RISE_STAGE = 512;         // masks staged in LDS at a time: 512 * (16 rows * 2 B + 8 B) = 20 KiB
constexpr int RISE_ROWS = 16;           // L = s + 2 <= 16 node rows of <= 16 bits
constexpr int RISE_MAX_S = 14;
constexpr int RISE_MAX_C = 4096;
#ifndef PPF_RISE_CH
#define PPF_RISE_CH 3
#endif
constexpr int RISE_CH = PPF_RISE_CH;    // channels a thread of the apply kernel owns (-DPPF_RISE_CH=1: a measurement build of scripts/bench_rise.py)

// One thread per (image, mask, call): calls 0 .. Q-1 are the node words, call Q is the shift (Philox counter word 0 = 0xFFFFFFFF).
__global__ __launch_bounds__(NT_RISE) void rise_nodes_kernel(const long long* __restrict__ image_id, uint64_t seed, uint32_t thr, int N, int LL, int Q,
                                                             int c, long long total, unsigned char* __restrict__ nodes, int* __restrict__ shift) {
    const long long t = (long long)blockIdx.x * NT_RISE + threadIdx.x;
    if (t >= total) return;
    const int k = (int)(t % (Q + 1));
    const long long bn = t / (Q + 1);                                          // b * N + n
    const int n = (int)(bn % N);
    const uint64_t id = (uint64_t)image_id[bn / N];
    const uint4 w = philox4x32_10(make_uint4(k == Q ? 0xFFFFFFFFu : (uint32_t)k, 1u + (uint32_t)n, (uint32_t)id, (uint32_t)(id >> 32)),
                                  make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
    if (k == Q) {
        shift[bn * 2 + 0] = (int)(((uint64_t)(w.x >> 8) * (uint32_t)c) >> 24);
        shift[bn * 2 + 1] = (int)(((uint64_t)(w.y >> 8) * (uint32_t)c) >> 24);
        return;
    }
    const uint32_t word[4] = {w.x, w.y, w.z, w.w};
    unsigned char* __restrict__ o = nodes + bn * LL;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int q = 4 * k + e;
        if (q < LL) o[q] = (word[e] >> 8) < thr ? 1 : 0;
    }
}

// Stages masks n_begin .. n_begin + count - 1 of one image: rows[k * RISE_ROWS + i] = the nodes of row i as bits (bit j = node (i, j)),
// sh[2k], sh[2k + 1] = (dy, dx) clamped into [0, c) (a table that was not written by rise_nodes_kernel cannot carry an index off the rows).
__device__ __forceinline__ void rise_stage(const unsigned char* __restrict__ nodes_b, const int* __restrict__ shift_b, long long n_begin, int count,
                                           int L, int c, unsigned short* rows, int* sh) {
    for (int e = threadIdx.x; e < count * L; e += NT_RISE) {
        const int k = e / L, i = e - k * L;
        const unsigned char* __restrict__ g = nodes_b + (n_begin + k) * (long long)(L * L) + i * L;
        unsigned bits = 0;
        for (int j = 0; j < L; ++j) bits |= (g[j] ? 1u : 0u) << j;
        rows[k * RISE_ROWS + i] = (unsigned short)bits;
    }
    for (int e = threadIdx.x; e < count * 2; e += NT_RISE) sh[e] = min(max(shift_b[n_begin * 2 + e], 0), c - 1);
}

// The integer numerator K of one pixel: node rows `top` (row i) and `bot` (row i + 1) as bits, column j, remainders ry, rx in [0, c).
__device__ __forceinline__ int rise_k(unsigned top, unsigned bot, int j, int ry, int rx, int c) {
    const unsigned a = top >> j, b = bot >> j;
    const int t = ((a & 1u) ? c - rx : 0) + ((a & 2u) ? rx : 0);
    const int u = ((b & 1u) ? c - rx : 0) + ((b & 2u) ? rx : 0);
    return __mul24(c - ry, t) + __mul24(ry, u);                               // every factor <= c <= 4096
}

// grid: B * groups * blocks_per_img workgroups; a workgroup lies inside one (image, channel group)
__global__ __launch_bounds__(NT_RISE) void rise_apply_kernel(const float4* __restrict__ x, const float4* __restrict__ base, float base_const,
                                                             const unsigned char* __restrict__ nodes, const int* __restrict__ shift, int N, int n0,
                                                             int Nc, int L, int c, float cc, int B, int Cc, int H, int W4, int blocks_per_img, int groups,
                                                             float4* __restrict__ out) {
    __shared__ unsigned short rows[RISE_STAGE * RISE_ROWS];
    __shared__ int sh[RISE_STAGE * 2];
    const int blk = blockIdx.x % blocks_per_img, bg = blockIdx.x / blocks_per_img;
    const int b = bg / groups, ch0 = (bg - b * groups) * RISE_CH;
    const int v = blk * NT_RISE + threadIdx.x;                                 // vector position inside a channel plane
    const int plane = H * W4;
    const bool live = v < plane;
    const int y = live ? v / W4 : 0, x0 = live ? (v - y * W4) * 4 : 0;
    const int iy0 = y / c, ry0 = y - iy0 * c, jx0 = x0 / c, rx0 = x0 - jx0 * c;
    float4 xv[RISE_CH], bv[RISE_CH];
#pragma unroll
    for (int q = 0; q < RISE_CH; ++q) {
        const bool on = live && ch0 + q < Cc;
        const size_t at = ((size_t)b * Cc + ch0 + q) * plane + v;
        xv[q] = on ? x[at] : make_float4(0.f, 0.f, 0.f, 0.f);
        bv[q] = on && base ? base[at] : make_float4(base_const, base_const, base_const, base_const);
    }
    const size_t img = (size_t)Cc * plane, copy = img * B;                     // vectors of one image, of one mask's batch
    for (int s0 = 0; s0 < Nc; s0 += RISE_STAGE) {
        const int count = min(RISE_STAGE, Nc - s0);
        // Measurement builds (scripts/bench_rise.py --variant): -DPPF_RISE_KNOCKOUT=1 keeps the staging and writes a constant mask,
        // =2 drops the staging and its barriers as well.  Neither is a result; the library is built without the switch.
#if !defined(PPF_RISE_KNOCKOUT) || PPF_RISE_KNOCKOUT < 2
        __syncthreads();                                                       // the previous stage has been read
        rise_stage(nodes + (size_t)b * N * (L * L), shift + (size_t)b * N * 2, (long long)n0 + s0, count, L, c, rows, sh);
        __syncthreads();
#endif
        if (!live) continue;
        for (int k = 0; k < count; ++k) {
            float m[4];
#ifdef PPF_RISE_KNOCKOUT
            m[0] = m[1] = m[2] = m[3] = 0.5f;
#else
            int ry = ry0 + sh[2 * k], i = iy0;
            if (ry >= c) { ry -= c; ++i; }
            int rx = rx0 + sh[2 * k + 1], j = jx0;
            if (rx >= c) { rx -= c; ++j; }
            const unsigned top = rows[k * RISE_ROWS + i], bot = rows[k * RISE_ROWS + i + 1];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                m[e] = __fdiv_rn((float)rise_k(top, bot, j, ry, rx, c), cc);
                if (++rx == c) { rx = 0; ++j; }
            }
#endif
            float4* __restrict__ o = out + (size_t)(s0 + k) * copy + (size_t)b * img + (size_t)ch0 * plane + v;
#pragma unroll
            for (int q = 0; q < RISE_CH; ++q) {
                if (ch0 + q >= Cc) break;                                      // workgroup-uniform
                float4 r;
                r.x = m[0] * xv[q].x + (1.0f - m[0]) * bv[q].x;
                r.y = m[1] * xv[q].y + (1.0f - m[1]) * bv[q].y;
                r.z = m[2] * xv[q].z + (1.0f - m[2]) * bv[q].z;
                r.w = m[3] * xv[q].w + (1.0f - m[3]) * bv[q].w;
                o[(size_t)q * plane] = r;
            }
        }
    }
}

// grid: B * blocks_per_img workgroups; a thread owns pixels (y, x0 .. x0 + 3) of image b for all M classes
__global__ __launch_bounds__(NT_RISE) void rise_saliency_kernel(const unsigned char* __restrict__ nodes, const int* __restrict__ shift,
                                                                const float* __restrict__ prob, int B, int N, int M, int L, int c, int H, int W4,
                                                                int blocks_per_img, double norm, float4* __restrict__ sal) {
    __shared__ unsigned short rows[RISE_STAGE * RISE_ROWS];
    __shared__ int sh[RISE_STAGE * 2];
    const int blk = blockIdx.x % blocks_per_img, b = blockIdx.x / blocks_per_img;
    const int v = blk * NT_RISE + threadIdx.x;
    const int plane = H * W4;
    const bool live = v < plane;
    const int y = live ? v / W4 : 0, x0 = live ? (v - y * W4) * 4 : 0;
    const int iy0 = y / c, ry0 = y - iy0 * c, jx0 = x0 / c, rx0 = x0 - jx0 * c;
    double acc[8][4];
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[m][e] = 0.0;
    for (int s0 = 0; s0 < N; s0 += RISE_STAGE) {
        const int count = min(RISE_STAGE, N - s0);
        __syncthreads();
        rise_stage(nodes + (size_t)b * N * (L * L), shift + (size_t)b * N * 2, s0, count, L, c, rows, sh);
        __syncthreads();
        if (!live) continue;
        for (int k = 0; k < count; ++k) {
            int ry = ry0 + sh[2 * k], i = iy0;
            if (ry >= c) { ry -= c; ++i; }
            int rx = rx0 + sh[2 * k + 1], j = jx0;
            if (rx >= c) { rx -= c; ++j; }
            const unsigned top = rows[k * RISE_ROWS + i], bot = rows[k * RISE_ROWS + i + 1];
            double kd[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                kd[e] = (double)rise_k(top, bot, j, ry, rx, c);
                if (++rx == c) { rx = 0; ++j; }
            }
            const float* __restrict__ p = prob + ((size_t)(s0 + k) * B + b) * M;        // workgroup-uniform address
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                if (m >= M) break;
                const double pd = (double)p[m];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[m][e] = fma(pd, kd[e], acc[m][e]);       // the product is exact: K <= 2^24
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        if (m >= M) break;
        sal[((size_t)b * M + m) * plane + v] = make_float4((float)(acc[m][0] / norm), (float)(acc[m][1] / norm), (float)(acc[m][2] / norm),
                                                           (float)(acc[m][3] / norm));
    }
}

// grid: B workgroups; a thread owns the cells g = tid, tid + NT_RISE, ... of image b, one after the other
__global__ __launch_bounds__(NT_RISE) void rise_cell_kernel(const unsigned char* __restrict__ nodes, const int* __restrict__ shift,
                                                            const float* __restrict__ prob, int B, int N, int M, int L, int c, int G, int side, int patch,
                                                            double norm_cell, float* __restrict__ cell) {
    __shared__ unsigned short rows[RISE_STAGE * RISE_ROWS];
    __shared__ int sh[RISE_STAGE * 2];
    const int b = blockIdx.x;
    for (int g0 = 0; g0 < G; g0 += NT_RISE) {                                  // workgroup-uniform trip count
        const int g = g0 + threadIdx.x;
        const bool live = g < G;
        const int gy = live ? g / side : 0, gx = live ? g - gy * side : 0;
        const int y0 = gy * patch, x0 = gx * patch;
        const int iy0 = y0 / c, ry0 = y0 - iy0 * c, jx0 = x0 / c, rx0 = x0 - jx0 * c;
        double acc[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) acc[m] = 0.0;
        for (int s0 = 0; s0 < N; s0 += RISE_STAGE) {
            const int count = min(RISE_STAGE, N - s0);
            __syncthreads();
            rise_stage(nodes + (size_t)b * N * (L * L), shift + (size_t)b * N * 2, s0, count, L, c, rows, sh);
            __syncthreads();
            if (!live) continue;
            for (int k = 0; k < count; ++k) {
                int ry = ry0 + sh[2 * k], i = iy0;
                if (ry >= c) { ry -= c; ++i; }
                int rxs = rx0 + sh[2 * k + 1], js = jx0;
                if (rxs >= c) { rxs -= c; ++js; }
                // rowsum(r) = the sum over the cell's columns of node row r's interpolation in x
                auto rowsum = [&](unsigned bits) {
                    int rx = rxs, j = js, sum = 0;
                    for (int e = 0; e < patch; ++e) {
                        const unsigned a = bits >> j;
                        sum += ((a & 1u) ? c - rx : 0) + ((a & 2u) ? rx : 0);
                        if (++rx == c) { rx = 0; ++j; }
                    }
                    return sum;                                               // <= patch * c
                };
                int top = rowsum(rows[k * RISE_ROWS + i]), bot = rowsum(rows[k * RISE_ROWS + i + 1]);
                int w = 0;                                                    // <= patch^2 * c^2 <= 2^29 (checked by the host)
                for (int e = 0; e < patch; ++e) {
                    w += (c - ry) * top + ry * bot;
                    if (++ry == c) {
                        ry = 0; ++i;
                        top = bot;
                        bot = e + 1 < patch ? rowsum(rows[k * RISE_ROWS + i + 1]) : 0;
                    }
                }
                const double wd = (double)w;
                const float* __restrict__ p = prob + ((size_t)(s0 + k) * B + b) * M;
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    if (m >= M) break;
                    acc[m] = fma((double)p[m], wd, acc[m]);                   // exact product: 24 + 29 bits
                }
            }
        }
        if (!live) continue;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            if (m >= M) break;
            cell[((size_t)b * M + m) * G + g] = (float)(acc[m] / norm_cell);
        }
    }
}

// The shape rules the three entry points share; c = ceil(H / s) on success.
int rise_shape(const char* who, int H, int s, int N, int* c) {
    PPF_CHECK_ARG(s >= 1 && s <= RISE_MAX_S, PPF_ERR_SHAPE, "%s: s=%d low-resolution cells per side outside [1, %d]", who, s, RISE_MAX_S);
    PPF_CHECK_ARG(H >= 4 && H % 4 == 0, PPF_ERR_SHAPE, "%s: H=%d must be a positive multiple of 4", who, H);
    *c = (H + s - 1) / s;
    PPF_CHECK_ARG(*c <= RISE_MAX_C, PPF_ERR_SHAPE, "%s: node spacing c=%d = ceil(H=%d / s=%d) exceeds %d", who, *c, H, s, RISE_MAX_C);
    PPF_CHECK_ARG(N >= 1 && N <= INT_MAX - 1, PPF_ERR_SHAPE, "%s: N=%d masks outside [1, 2^31 - 2]", who, N);
    return 0;
}

}  // namespace

extern "C" {

int ppf_rise_nodes(const void* image_id_i64, uint64_t seed, int thr, int B, int N, int s, int H, void* nodes_u8, int* shift, hipStream_t stream) {
    int c = 0;
    if (int rc = rise_shape("ppf_rise_nodes", H, s, N, &c)) return rc;
    PPF_CHECK_ARG(B >= 1, PPF_ERR_SHAPE, "ppf_rise_nodes: B=%d (>= 1)", B);
    PPF_CHECK_ARG(thr >= 1 && thr <= (1 << 24), PPF_ERR_ARG, "ppf_rise_nodes: thr=%d outside [1, 2^24] (keep probability thr / 2^24)", thr);
    PPF_CHECK_ARG(image_id_i64 && nodes_u8 && shift, PPF_ERR_ARG, "ppf_rise_nodes: null pointer (image_id, nodes, shift)");
    const int L = s + 2, LL = L * L, Q = (LL + 3) / 4;
    PPF_CHECK_ARG((long long)B * N <= (long long)INT_MAX * NT_RISE / (Q + 1) - 1, PPF_ERR_SHAPE, "ppf_rise_nodes: B=%d x N=%d masks exceed the grid", B, N);
    const long long total = (long long)B * N * (Q + 1), blocks = (total + NT_RISE - 1) / NT_RISE;
    return ppf_launch<rise_nodes_kernel>(dim3((unsigned)blocks), dim3(NT_RISE), 0, stream, "ppf_rise_nodes", (const long long*)image_id_i64, seed,
                                         (uint32_t)thr, N, LL, Q, c, total, (unsigned char*)nodes_u8, shift);
}

int ppf_rise_apply(const float* x, const void* nodes_u8, const int* shift, int N, int n0, int Nc, int s, const float* baseline, float baseline_const,
                   int B, int Cc, int H, int W, float* out, hipStream_t stream) {
    PPF_CHECK_ARG(H == W, PPF_ERR_SHAPE, "ppf_rise_apply: H=%d W=%d (square images only)", H, W);
    PPF_CHECK_ARG(W >= 4 && W % 4 == 0, PPF_ERR_SHAPE, "ppf_rise_apply: W=%d is not a positive multiple of 4 (16-byte vectors)", W);
    int c = 0;
    if (int rc = rise_shape("ppf_rise_apply", H, s, N, &c)) return rc;
    PPF_CHECK_ARG(B >= 1 && Cc >= 1, PPF_ERR_SHAPE, "ppf_rise_apply: bad shape B=%d Cc=%d (both >= 1)", B, Cc);
    PPF_CHECK_ARG(n0 >= 0 && Nc >= 1 && (long long)n0 + Nc <= N, PPF_ERR_SHAPE, "ppf_rise_apply: masks n0=%d .. n0 + Nc=%d - 1 outside [0, N=%d)", n0, Nc,
                  N);
    PPF_CHECK_ARG(x && nodes_u8 && shift && out, PPF_ERR_ARG, "ppf_rise_apply: null pointer (only baseline may be NULL)");
    PPF_CHECK_ARG((((uintptr_t)x | (uintptr_t)out | (uintptr_t)baseline) & 15) == 0, PPF_ERR_ALIGN,
                  "ppf_rise_apply: x, baseline and out must be 16-byte aligned");
    const int W4 = W / 4, blocks_per_img = (H * W4 + NT_RISE - 1) / NT_RISE, groups = Cc / RISE_CH + (Cc % RISE_CH != 0);
    const long long per_img = (long long)groups * blocks_per_img, blocks = per_img <= INT_MAX ? per_img * B : per_img;     // no overflow: both < 2^31
    PPF_CHECK_ARG(blocks <= INT_MAX, PPF_ERR_SHAPE, "ppf_rise_apply: B=%d x Cc=%d x H=%d x W=%d exceeds the grid", B, Cc, H, W);
    return ppf_launch<rise_apply_kernel>(dim3((unsigned)blocks), dim3(NT_RISE), 0, stream, "ppf_rise_apply", (const float4*)x, (const float4*)baseline,
                                         baseline_const, (const unsigned char*)nodes_u8, shift, N, n0, Nc, s + 2, c, (float)(c * c), B, Cc, H, W4,
                                         blocks_per_img, groups, (float4*)out);
}

int ppf_rise_accumulate(const void* nodes_u8, const int* shift, const float* prob, int B, int N, int M, int s, int thr, int H, int W, int G, float* sal,
                        float* cell, hipStream_t stream) {
    PPF_CHECK_ARG(H == W, PPF_ERR_SHAPE, "ppf_rise_accumulate: H=%d W=%d (square images only)", H, W);
    int c = 0;
    if (int rc = rise_shape("ppf_rise_accumulate", H, s, N, &c)) return rc;
    PPF_CHECK_ARG(B >= 1, PPF_ERR_SHAPE, "ppf_rise_accumulate: B=%d (>= 1)", B);
    PPF_CHECK_ARG(M >= 1 && M <= 8, PPF_ERR_SHAPE, "ppf_rise_accumulate: M=%d outside [1, 8]", M);
    PPF_CHECK_ARG(thr >= 1 && thr <= (1 << 24), PPF_ERR_ARG, "ppf_rise_accumulate: thr=%d outside [1, 2^24] (keep probability thr / 2^24)", thr);
    PPF_CHECK_ARG(G >= 1 && G <= 1024, PPF_ERR_SHAPE, "ppf_rise_accumulate: G=%d grid cells outside [1, 1024]", G);
    const int side = (int)lround(sqrt((double)G));
    PPF_CHECK_ARG(side * side == G, PPF_ERR_SHAPE, "ppf_rise_accumulate: G=%d is not a square grid", G);
    PPF_CHECK_ARG(H % side == 0, PPF_ERR_SHAPE, "ppf_rise_accumulate: the grid side %d (G=%d) does not divide H=%d", side, G, H);
    const int patch = H / side;
    PPF_CHECK_ARG((long long)patch * patch * c * c <= (1LL << 29), PPF_ERR_SHAPE,
                  "ppf_rise_accumulate: cell mass patch^2 * c^2 = %lld (patch=%d, c=%d) exceeds 2^29 (exact fp64 products)",
                  (long long)patch * patch * c * c, patch, c);
    PPF_CHECK_ARG(nodes_u8 && shift && prob && sal && cell, PPF_ERR_ARG, "ppf_rise_accumulate: null pointer");
    PPF_CHECK_ARG(((uintptr_t)sal & 15) == 0, PPF_ERR_ALIGN, "ppf_rise_accumulate: sal must be 16-byte aligned");
    const int W4 = W / 4, blocks_per_img = (H * W4 + NT_RISE - 1) / NT_RISE;
    PPF_CHECK_ARG((long long)B * blocks_per_img <= INT_MAX, PPF_ERR_SHAPE, "ppf_rise_accumulate: B=%d x H=%d x W=%d exceeds the grid", B, H, W);
    const double norm = (double)N * ((double)thr / 16777216.0) * (double)(c * c);
    if (int rc = ppf_launch<rise_saliency_kernel>(dim3((unsigned)(B * blocks_per_img)), dim3(NT_RISE), 0, stream, "ppf_rise_accumulate",
                                                  (const unsigned char*)nodes_u8, shift, prob, B, N, M, s + 2, c, H, W4, blocks_per_img, norm, (float4*)sal))
        return rc;
    return ppf_launch<rise_cell_kernel>(dim3((unsigned)B), dim3(NT_RISE), 0, stream, "ppf_rise_accumulate", (const unsigned char*)nodes_u8, shift, prob, B,
                                        N, M, s + 2, c, G, side, patch, norm * (double)(patch * patch), cell);
}

}  // extern "C"
