// "This looks like that, because ..." (Nauta et al., 2021): which visual characteristic of a patch makes it look like a prototype?  One
// characteristic of the image is suppressed -- hue, saturation, contrast (a colour transform), texture (an edge-preserving filter) or
// shape (a smooth warp) --, the model runs again, and the prototype's similarity at the same grid cell is read off the perturbed forward.
// The forwards in between are the caller's.  The arithmetic of every kernel is a written contract (include/ppf_hip.h), repeated here
// operation for operation, so the numpy referees (interpret.color_affine, gray_sum, bilateral, warp_*, because_score) agree bit for bit:
// plain fp32, every operation rounded once, no contraction, correctly rounded division, no transcendental function on the device (the
// Gaussian tables and the hue matrix are computed by the host in fp64 and passed in).  The reference has no such pass.
//   * color_affine_kernel, gray_sum_kernel: streaming; a thread owns V = 4 consecutive pixels of a row in all three channels (16-byte
//     accesses) when W % 4 == 0 and the pointers are aligned, else V = 1.
//   * warp_apply_kernel: a gather; the lanes of a wave own consecutive pixels and a thread four of them a workgroup apart (see there).
//   * contrast_offset_kernel: the contrast offsets from the integer grey sums, on the device (no host read in between).
//   * bilateral_kernel: a workgroup of 256 threads owns a tile of BIL_TW x BIL_TH = 32 x 16 pixels and stages the tile plus its halo of r
//     pixels ONCE in LDS, one 16-byte slot per pixel: (r, g, b, q8) -- the three clamped de-normalised channels and the 8-bit luma, -512
//     outside the image.  A tap is then one ds_read_b128 (lanes of a wave read consecutive slots: conflict-free) and one look-up in the
//     range table, which is staged too, as is the spatial table (a broadcast read).  A thread owns the pixels (ty, tx) and (ty + 8, tx).
//     LDS: (32 + 2r)(16 + 2r) * 16 + 4096 + (2r + 1)^2 * 4 bytes = 29.1 KiB at r = 8, 13.4 KiB at r = 1: five workgroups (20 waves) per
//     compute unit at the widest window, the eight the wave slots admit up to r = 3.
//   * warp_nodes_kernel: one thread per node, one Philox call each (the library's generator, ppf_common.h).
//   * because_score_kernel: one wave per (image, prototype) row, one wave per workgroup, as explain_topk_kernel.
// Deterministic: integer atomics only (gray sums), fixed summation order everywhere else.
#include <limits.h>
#include <math.h>

#include "ppf_common.h"
#include "ppf_hip.h"

// every operation below is rounded once, as numpy's: see rise.hip for why this is the pragma and not __fmul_rn / __fadd_rn
#pragma clang fp contract(off)

namespace {

constexpr int NT_BEC = 256;
constexpr int BIL_TW = 32, BIL_TH = 16;     // the bilateral tile: 256 threads, two pixels each
constexpr int BIL_MAX_R = 8;
constexpr int BIL_OUT = -512, BIL_WR = 1024;  // the q8 of a tap outside the image; entries of the staged range table (bilateral_kernel)
constexpr int WARP_MAX_S = 16;
constexpr int WARP_MAX_C = 2048;            // H * W <= 2^22 and H == W: never reached; the warp's 24-bit products rest on it
constexpr int WARP_MAX_A = 1 << 15;         // 128 pixels in 1/256 units

struct Norm3 { float mean[3], std[3]; };
struct ColorParams { float m[9]; Norm3 n; };
struct BilateralParams { float ws[(2 * BIL_MAX_R + 1) * (2 * BIL_MAX_R + 1)]; float wr[256]; Norm3 n; };

// clamp to [0, 1]; NaN becomes 0 (both comparisons are false for it), as the referee's np.where
__device__ __forceinline__ float clamp01(float v) { return v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f; }
// v = clamp(fl(fl(x * std) + mean))
__device__ __forceinline__ float denorm(float x, float mean, float std) { const float t = x * std; return clamp01(t + mean); }
// fl(fl(v - mean) / std), the division correctly rounded
__device__ __forceinline__ float renorm(float v, float mean, float std) { const float t = v - mean; return __fdiv_rn(t, std); }
// y = fl(fl(fl(0.299 r) + fl(0.587 g)) + fl(0.114 b));  q8 = min(max((int)floor(fl(fl(255 y) + 0.5)), 0), 255)
__device__ __forceinline__ int luma_q8(float r, float g, float b) {
    const float a = 0.299f * r, c = 0.587f * g, d = 0.114f * b;
    const float s = a + c;
    const float y = s + d;
    const float t = 255.0f * y;
    const int q = (int)floorf(t + 0.5f);
    return min(max(q, 0), 255);
}

template <int V> struct Vec;
template <> struct Vec<1> { typedef float type; };
template <> struct Vec<4> { typedef float4 type; };
template <int V> __device__ __forceinline__ void load_v(const float* p, float (&v)[V]) {
    const typename Vec<V>::type t = *reinterpret_cast<const typename Vec<V>::type*>(p);
    __builtin_memcpy(v, &t, sizeof(t));
}
template <int V> __device__ __forceinline__ void store_v(float* p, const float (&v)[V]) {
    typename Vec<V>::type t;
    __builtin_memcpy(&t, v, sizeof(t));
    *reinterpret_cast<typename Vec<V>::type*>(p) = t;
}

// grid: (ceil(plane / V / NT_BEC), B); a thread owns V consecutive pixels of image b in the three channels
template <int V>
__global__ __launch_bounds__(NT_BEC) void color_affine_kernel(const float* __restrict__ x, const float* __restrict__ off, ColorParams p, int plane,
                                                              float* __restrict__ out) {
    const int b = blockIdx.y;
    const int at = (blockIdx.x * NT_BEC + threadIdx.x) * V;
    if (at >= plane) return;
    const size_t base = (size_t)b * 3 * plane + at;
    float ch[3][V], res[3][V];
#pragma unroll
    for (int k = 0; k < 3; ++k) load_v<V>(x + base + (size_t)k * plane, ch[k]);
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const float r = denorm(ch[0][e], p.n.mean[0], p.n.std[0]), g = denorm(ch[1][e], p.n.mean[1], p.n.std[1]),
                    bl = denorm(ch[2][e], p.n.mean[2], p.n.std[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float a = p.m[3 * k + 0] * r, c = p.m[3 * k + 1] * g, d = p.m[3 * k + 2] * bl;
            const float s = a + c;
            float t = s + d;
            if (off) t = t + off[b * 3 + k];
            res[k][e] = renorm(clamp01(t), p.n.mean[k], p.n.std[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) store_v<V>(out + base + (size_t)k * plane, res[k]);
}

// grid: (blocks, B); sum[b] += the q8 of the pixels this workgroup walks (integer atomics: exact at any launch shape)
template <int V>
__global__ __launch_bounds__(NT_BEC) void gray_sum_kernel(const float* __restrict__ x, Norm3 n, int plane, int* __restrict__ sum) {
    const int b = blockIdx.y;
    const float* __restrict__ xb = x + (size_t)b * 3 * plane;
    int acc = 0;
    for (long long at = ((long long)blockIdx.x * NT_BEC + threadIdx.x) * V; at < plane; at += (long long)gridDim.x * NT_BEC * V) {
        float ch[3][V];
#pragma unroll
        for (int k = 0; k < 3; ++k) load_v<V>(xb + (size_t)k * plane + at, ch[k]);
#pragma unroll
        for (int e = 0; e < V; ++e)
            acc += luma_q8(denorm(ch[0][e], n.mean[0], n.std[0]), denorm(ch[1][e], n.mean[1], n.std[1]), denorm(ch[2][e], n.mean[2], n.std[2]));
    }
    acc = wave_sum_i32(acc);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(sum + b, acc);
}

// off[b][k] = fl(g * fl(fl((float)sum[b] / (float)plane) / 255)), k = 0 .. 2
__global__ __launch_bounds__(NT_BEC) void contrast_offset_kernel(const int* __restrict__ sum, int B, float plane_f, float g, float* __restrict__ off) {
    const int b = blockIdx.x * NT_BEC + threadIdx.x;
    if (b >= B) return;
    const float mean_q = __fdiv_rn((float)sum[b], plane_f);
    const float m = __fdiv_rn(mean_q, 255.0f);
    const float o = g * m;
    off[b * 3 + 0] = o; off[b * 3 + 1] = o; off[b * 3 + 2] = o;
}

// grid: (ceil(W / 32), ceil(H / 16), B); dynamic LDS: the padded tile, then wr_s[BIL_WR], then ws[(2r + 1)^2]
__global__ __launch_bounds__(NT_BEC) void bilateral_kernel(const float* __restrict__ x, BilateralParams p, int r, int H, int W, float* __restrict__ out) {
    extern __shared__ float4 tile[];
    const int PW = BIL_TW + 2 * r, PH = BIL_TH + 2 * r, D = 2 * r + 1;
    float* __restrict__ wr_s = reinterpret_cast<float*>(tile + PW * PH);
    float* __restrict__ ws_s = wr_s + BIL_WR;
    const int tid = threadIdx.x, b = blockIdx.z;
    const int plane = H * W;
    const float* __restrict__ xb = x + (size_t)b * 3 * plane;
    const int x0 = blockIdx.x * BIL_TW - r, y0 = blockIdx.y * BIL_TH - r;
    for (int e = tid; e < PW * PH; e += NT_BEC) {
        const int ly = e / PW, lx = e - ly * PW;
        const int gy = y0 + ly, gx = x0 + lx;
        float4 t = make_float4(0.f, 0.f, 0.f, __int_as_float(BIL_OUT));           // a tap outside the image: skipped (weight 0)
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const int at = gy * W + gx;
            t.x = denorm(xb[at], p.n.mean[0], p.n.std[0]);
            t.y = denorm(xb[plane + at], p.n.mean[1], p.n.std[1]);
            t.z = denorm(xb[2 * plane + at], p.n.mean[2], p.n.std[2]);
            t.w = __int_as_float(luma_q8(t.x, t.y, t.z));
        }
        tile[e] = t;
    }
    // The range table is staged by signed difference, wr_s[255 + d] = wr[|d|] for |d| <= 255, and zero from there to BIL_WR: a tap
    // outside the image carries q = BIL_OUT = -512, so its index 255 + q(p) + 512 falls into the zeros and its weight is fl(ws * 0) = 0
    // without a test (the inner loop is bound by its VALU work: abs, clamp, compare and select were five of fifteen instructions).
    for (int e = tid; e < BIL_WR; e += NT_BEC) {
        const int d = abs(e - 255);
        wr_s[e] = d < 256 ? p.wr[d] : 0.0f;
    }
    for (int e = tid; e < D * D; e += NT_BEC) ws_s[e] = p.ws[e];
    __syncthreads();

    const int tx = tid & (BIL_TW - 1), ty = tid / BIL_TW;                          // ty in [0, 8): the pixels (ty, tx) and (ty + 8, tx)
    const int gx = blockIdx.x * BIL_TW + tx;
    const float4* __restrict__ c0 = tile + (ty + r) * PW + tx + r;
    const float4* __restrict__ c1 = c0 + (BIL_TH / 2) * PW;
    // the table index of a tap is q(p) + 255 - q(tap); a thread whose own pixel lies outside the image takes q(p) = 0
    const int q0 = max(__float_as_int(c0->w), 0) + 255, q1 = max(__float_as_int(c1->w), 0) + 255;
    float sw0 = 0.f, sr0 = 0.f, sg0 = 0.f, sb0 = 0.f, sw1 = 0.f, sr1 = 0.f, sg1 = 0.f, sb1 = 0.f;
    for (int dy = 0; dy < D; ++dy) {                                               // row-major window order: the order is the contract
        const float4* __restrict__ row0 = tile + (ty + dy) * PW + tx;
        const float4* __restrict__ row1 = row0 + (BIL_TH / 2) * PW;
        const float* __restrict__ wrow = ws_s + dy * D;
#pragma unroll 3
        for (int dx = 0; dx < D; ++dx) {                                           // D = 2r + 1 >= 3
            const float s = wrow[dx];
            const float4 a = row0[dx], c = row1[dx];
            const int qa = __float_as_int(a.w), qc = __float_as_int(c.w);
            const float wa = s * wr_s[q0 - qa], wc = s * wr_s[q1 - qc];             // no branch, no clamp: see the staging of wr_s
            sw0 = sw0 + wa;
            const float ar = wa * a.x, ag = wa * a.y, ab = wa * a.z;
            sr0 = sr0 + ar; sg0 = sg0 + ag; sb0 = sb0 + ab;
            sw1 = sw1 + wc;
            const float cr = wc * c.x, cg = wc * c.y, cb = wc * c.z;
            sr1 = sr1 + cr; sg1 = sg1 + cg; sb1 = sb1 + cb;
        }
    }
    if (gx >= W) return;
    float* __restrict__ ob = out + (size_t)b * 3 * plane;
    const int gy0 = blockIdx.y * BIL_TH + ty, gy1 = gy0 + BIL_TH / 2;
    if (gy0 < H) {
        const int at = gy0 * W + gx;
        ob[at] = renorm(clamp01(__fdiv_rn(sr0, sw0)), p.n.mean[0], p.n.std[0]);
        ob[plane + at] = renorm(clamp01(__fdiv_rn(sg0, sw0)), p.n.mean[1], p.n.std[1]);
        ob[2 * plane + at] = renorm(clamp01(__fdiv_rn(sb0, sw0)), p.n.mean[2], p.n.std[2]);
    }
    if (gy1 < H) {
        const int at = gy1 * W + gx;
        ob[at] = renorm(clamp01(__fdiv_rn(sr1, sw1)), p.n.mean[0], p.n.std[0]);
        ob[plane + at] = renorm(clamp01(__fdiv_rn(sg1, sw1)), p.n.mean[1], p.n.std[1]);
        ob[2 * plane + at] = renorm(clamp01(__fdiv_rn(sb1, sw1)), p.n.mean[2], p.n.std[2]);
    }
}

// One thread per (image, node): nodes[b][q] = (dy, dx), each ((draw >> 8) * (2A + 1) >> 24) - A in [-A, A]
__global__ __launch_bounds__(NT_BEC) void warp_nodes_kernel(const long long* __restrict__ image_id, uint64_t seed, int Q, int A, long long total,
                                                            int* __restrict__ nodes) {
    const long long t = (long long)blockIdx.x * NT_BEC + threadIdx.x;
    if (t >= total) return;
    const int q = (int)(t % Q);
    const uint64_t id = (uint64_t)image_id[t / Q];
    const uint4 w = philox4x32_10(make_uint4((uint32_t)q, 0x80000000u, (uint32_t)id, (uint32_t)(id >> 32)),
                                  make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
    const uint64_t span = (uint64_t)(2 * A + 1);
    nodes[t * 2 + 0] = (int)(((uint64_t)(w.x >> 8) * span) >> 24) - A;
    nodes[t * 2 + 1] = (int)(((uint64_t)(w.y >> 8) * span) >> 24) - A;
}

// floor(a / d) for |a| <= d * 2^15 and d <= 2^24, without an integer division: inv = 1.0 / d in fp64.  |a * inv - a / d| <= 2^-37; a
// quotient that is no integer lies at least 1 / d >= 2^-24 from the next one, an integer one is lifted off the edge by the 2^-26.
__device__ __forceinline__ int floor_div(int a, double inv) { return (int)floor((double)a * inv + 0x1p-26); }

// n / d for 0 <= n < 2^22 and d >= 1 with inv = fl(1 / (float)d), exactly: the fp32 product is within one of the quotient, the remainder
// says which way.  (The kernel below is bound by its VALU work; an integer division is some forty instructions.)
__device__ __forceinline__ int div_small(int n, int d, float inv) {                // d <= 2^11 here: the product fits 24 x 24 bits
    const int q = (int)((float)n * inv);
    const int r = n - __mul24(q, d);
    return r < 0 ? q - 1 : (r >= d ? q + 1 : q);
}

constexpr int WARP_U = 4;                   // pixels per thread (1, 2 and 4 were measured within 3 % of each other)

// grid: (ceil(H * W / (U * NT_BEC)), B); a thread owns the pixels at0 + e * NT_BEC, e < U, in all channels (CC = 3, or CC = 0: Cc of
// them): the lanes of a wave lie on consecutive pixels, so its gathers touch few cache lines each, and the U pixels keep 4 U node loads
// and then 4 U CC pixel loads in flight.  (Four CONSECUTIVE pixels per thread and 16-byte stores were measured 1.3 x slower at batch
// 256: every gather then strides 16 bytes across the lanes.  The figures are in profiles/because_cost.txt.)
template <int U, int CC>
__global__ __launch_bounds__(NT_BEC) void warp_apply_kernel(const float* __restrict__ x, const int* __restrict__ nodes, int s, int c, double inv_cc, float inv_c,
                                                            float inv_w, int A, int Cc, int H, int W, float* __restrict__ out) {
    const int b = blockIdx.y, plane = H * W;
    const int at0 = blockIdx.x * (NT_BEC * U) + threadIdx.x;
    if (at0 >= plane) return;
    const int L = s + 1;
    const int2* __restrict__ nb = reinterpret_cast<const int2*>(nodes) + (size_t)b * L * L;               // (dy, dx) of a node: one 8-byte load
    int2 nd[4][U];
    int yy[U], xx[U], ry[U], rx[U];
#pragma unroll
    for (int e = 0; e < U; ++e) {
        const int at = min(at0 + e * NT_BEC, plane - 1);                           // past the plane: the last pixel again, not stored
        yy[e] = div_small(at, W, inv_w); xx[e] = at - __mul24(yy[e], W);
        const int i = div_small(yy[e], c, inv_c), j = div_small(xx[e], c, inv_c);          // i + 1 <= s: y <= H - 1 <= s * c - 1; likewise j
        ry[e] = yy[e] - __mul24(i, c); rx[e] = xx[e] - __mul24(j, c);
        const int2* __restrict__ n0 = nb + __mul24(i, L) + j;
        nd[0][e] = n0[0]; nd[1][e] = n0[1]; nd[2][e] = n0[L]; nd[3][e] = n0[L + 1];
    }
    int src[4][U];                                                                 // the four source offsets inside a plane
    float wx1[U], wy1[U];                                                          // the weights of the right / lower source, n / 256: exact
    bool bx[U], by[U];
#pragma unroll
    for (int e = 0; e < U; ++e) {
        // every factor fits 24 bits (c <= 2^11, so K <= 2^22; |node| <= 2^15): v_mul_i32_i24 runs at four times the rate of a 32-bit product
        const int k00 = __mul24(c - ry[e], c - rx[e]), k01 = __mul24(c - ry[e], rx[e]), k10 = __mul24(ry[e], c - rx[e]), k11 = __mul24(ry[e], rx[e]);
        auto cl = [&](int v) { return min(max(v, -A), A); };                       // a foreign table cannot overflow the sum
        const int dy = floor_div(__mul24(k00, cl(nd[0][e].x)) + __mul24(k01, cl(nd[1][e].x)) + __mul24(k10, cl(nd[2][e].x)) + __mul24(k11, cl(nd[3][e].x)), inv_cc);
        const int dx = floor_div(__mul24(k00, cl(nd[0][e].y)) + __mul24(k01, cl(nd[1][e].y)) + __mul24(k10, cl(nd[2][e].y)) + __mul24(k11, cl(nd[3][e].y)), inv_cc);
        const int Y = min(max(256 * yy[e] + dy, 0), 256 * (H - 1)), X = min(max(256 * xx[e] + dx, 0), 256 * (W - 1));
        const int sy = Y >> 8, fy = Y & 255, sx = X >> 8, fx = X & 255;
        const int sy1 = min(sy + 1, H - 1), sx1 = min(sx + 1, W - 1);
        const int r0 = __mul24(sy, W), r1 = __mul24(sy1, W);
        src[0][e] = r0 + sx; src[1][e] = r0 + sx1; src[2][e] = r1 + sx; src[3][e] = r1 + sx1;
        wx1[e] = (float)fx * 0.00390625f; wy1[e] = (float)fy * 0.00390625f;
        bx[e] = fx != 0; by[e] = fy != 0;
    }
    auto channel = [&](int k) {
        const float* __restrict__ xp = x + ((size_t)b * Cc + k) * plane;
        float* __restrict__ op = out + ((size_t)b * Cc + k) * plane;
        float v[4][U];
#pragma unroll
        for (int e = 0; e < U; ++e)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q][e] = xp[src[q][e]];                   // all loads in flight; the addresses are always inside the plane
#pragma unroll
        for (int e = 0; e < U; ++e) {
            // a zero weight's term is skipped, not multiplied: amplitude 0 copies the input bit for bit (-0, inf and NaN included)
            const float ta = (1.0f - wx1[e]) * v[0][e], tb = wx1[e] * v[1][e];
            const float top = bx[e] ? ta + tb : v[0][e];
            const float ba = (1.0f - wx1[e]) * v[2][e], bb = wx1[e] * v[3][e];
            const float bot = bx[e] ? ba + bb : v[2][e];
            const float oa = (1.0f - wy1[e]) * top, ob = wy1[e] * bot;
            if (at0 + e * NT_BEC < plane) op[at0 + e * NT_BEC] = by[e] ? oa + ob : top;
        }
    };
    if (CC) {
#pragma unroll
        for (int k = 0; k < CC; ++k) channel(k);
    } else {
        for (int k = 0; k < Cc; ++k) channel(k);
    }
}

// grid: B * K workgroups of one wave: row (b, k) of prototype protos[b][k] and cell cells[b][k]
__global__ __launch_bounds__(64) void because_score_kernel(const float* __restrict__ act_full, const int* __restrict__ idx, const float* __restrict__ act_max,
                                                           const int* __restrict__ protos, const int* __restrict__ cells, int P, int T, int G, int K,
                                                           float* __restrict__ same, float* __restrict__ best, int* __restrict__ lost) {
    const int row = blockIdx.x, b = row / K, lane = threadIdx.x;
    const int p = protos[row];
    const bool valid = p >= 0 && p < P;
    if (lane == 0) best[row] = valid ? act_max[(size_t)b * P + p] : __int_as_float(0x7fc00000);
    if (!idx) return;                                                              // the global branch has no cells
    const int c = cells[row];
    int found = INT_MAX;                                                           // the smallest t with idx[b][t] == c
    if (valid && c >= 0 && c < G)                                                  // so an idx entry outside the grid never matches
        for (int t = lane; t < T; t += 64)
            if (idx[(size_t)b * T + t] == c) { found = t; break; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) found = min(found, __shfl_xor(found, o, 64));
    if (lane == 0) {
        const bool kept = found != INT_MAX;
        same[row] = kept ? act_full[((size_t)b * P + p) * T + found] : 0.0f;       // a NaN activation is written as it is
        lost[row] = kept ? 0 : 1;
    }
}

int norm_check(const char* who, const float* mean3, const float* std3, Norm3* n) {
    PPF_CHECK_ARG(mean3 && std3, PPF_ERR_ARG, "%s: null pointer (mean3, std3: host pointers)", who);
    for (int k = 0; k < 3; ++k) {
        PPF_CHECK_ARG(isfinite(mean3[k]) && isfinite(std3[k]) && std3[k] > 0.f, PPF_ERR_ARG, "%s: mean3[%d]=%g std3[%d]=%g (finite, std > 0)", who, k,
                      (double)mean3[k], k, (double)std3[k]);
        n->mean[k] = mean3[k]; n->std[k] = std3[k];
    }
    return 0;
}

// B, H, W of a three-channel image batch; plane = H * W <= 2^22
int image_check(const char* who, int B, int H, int W) {
    PPF_CHECK_ARG(B >= 1 && B <= 65535, PPF_ERR_SHAPE, "%s: B=%d outside [1, 65535]", who, B);
    PPF_CHECK_ARG(H >= 1 && W >= 1 && (long long)H * W <= (1 << 22), PPF_ERR_SHAPE, "%s: H=%d W=%d (both >= 1, H * W <= 2^22)", who, H, W);
    return 0;
}

bool vec_ok(int W, const void* a, const void* b) { return W % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

}  // namespace

extern "C" {

int ppf_color_affine(const float* x, const float* matrix9, const float* offset, const float* mean3, const float* std3, int B, int H, int W, float* out,
                     hipStream_t stream) {
    const char* who = "ppf_color_affine";
    if (int rc = image_check(who, B, H, W)) return rc;
    PPF_CHECK_ARG(x && matrix9 && out, PPF_ERR_ARG, "%s: null pointer (only offset may be NULL)", who);
    ColorParams p;
    if (int rc = norm_check(who, mean3, std3, &p.n)) return rc;
    for (int k = 0; k < 9; ++k) {
        PPF_CHECK_ARG(isfinite(matrix9[k]), PPF_ERR_ARG, "%s: matrix9[%d] is not finite", who, k);
        p.m[k] = matrix9[k];
    }
    const int plane = H * W;
    if (vec_ok(W, x, out))
        return ppf_launch<color_affine_kernel<4>>(dim3((plane / 4 + NT_BEC - 1) / NT_BEC, B), dim3(NT_BEC), 0, stream, who, x, offset, p, plane, out);
    return ppf_launch<color_affine_kernel<1>>(dim3((plane + NT_BEC - 1) / NT_BEC, B), dim3(NT_BEC), 0, stream, who, x, offset, p, plane, out);
}

int ppf_gray_sum(const float* x, const float* mean3, const float* std3, int B, int H, int W, int* sum, hipStream_t stream) {
    const char* who = "ppf_gray_sum";
    if (int rc = image_check(who, B, H, W)) return rc;
    PPF_CHECK_ARG(x && sum, PPF_ERR_ARG, "%s: null pointer", who);
    Norm3 n;
    if (int rc = norm_check(who, mean3, std3, &n)) return rc;
    if (hipError_t e = ppf_memset_async(sum, 0, (size_t)B * sizeof(int), stream)) {
        ppf_set_error("%s: zeroing the sums: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    const int plane = H * W;
    // 16 pixels per thread and trip where the image is large enough: a few atomics per image
    if (vec_ok(W, x, x))
        return ppf_launch<gray_sum_kernel<4>>(dim3(min(max(plane / (NT_BEC * 16), 1), 64), B), dim3(NT_BEC), 0, stream, who, x, n, plane, sum);
    return ppf_launch<gray_sum_kernel<1>>(dim3(min(max(plane / (NT_BEC * 16), 1), 64), B), dim3(NT_BEC), 0, stream, who, x, n, plane, sum);
}

int ppf_contrast_offset(const int* gray_sum, int B, int H, int W, float one_minus_f, float* offset, hipStream_t stream) {
    const char* who = "ppf_contrast_offset";
    if (int rc = image_check(who, B, H, W)) return rc;
    PPF_CHECK_ARG(gray_sum && offset, PPF_ERR_ARG, "%s: null pointer", who);
    PPF_CHECK_ARG(isfinite(one_minus_f), PPF_ERR_ARG, "%s: one_minus_f is not finite", who);
    return ppf_launch<contrast_offset_kernel>(dim3((B + NT_BEC - 1) / NT_BEC), dim3(NT_BEC), 0, stream, who, gray_sum, B, (float)(H * W), one_minus_f,
                                              offset);
}

int ppf_bilateral(const float* x, const float* ws, const float* wr256, int r, const float* mean3, const float* std3, int B, int H, int W, float* out,
                  hipStream_t stream) {
    const char* who = "ppf_bilateral";
    if (int rc = image_check(who, B, H, W)) return rc;
    PPF_CHECK_ARG(r >= 1 && r <= BIL_MAX_R, PPF_ERR_SHAPE, "%s: window radius r=%d outside [1, %d]", who, r, BIL_MAX_R);
    PPF_CHECK_ARG(x && ws && wr256 && out, PPF_ERR_ARG, "%s: null pointer (ws, wr256: host pointers)", who);
    PPF_CHECK_ARG(x != out, PPF_ERR_ARG, "%s: out must not be x (a tile reads its neighbours' pixels)", who);
    BilateralParams p;
    if (int rc = norm_check(who, mean3, std3, &p.n)) return rc;
    const int D = 2 * r + 1;
    for (int k = 0; k < D * D; ++k) {
        PPF_CHECK_ARG(isfinite(ws[k]) && ws[k] >= 0.f, PPF_ERR_ARG, "%s: ws[%d] must be finite and >= 0", who, k);
        p.ws[k] = ws[k];
    }
    for (int k = D * D; k < (int)(sizeof(p.ws) / sizeof(float)); ++k) p.ws[k] = 0.f;
    for (int k = 0; k < 256; ++k) {
        PPF_CHECK_ARG(isfinite(wr256[k]) && wr256[k] >= 0.f, PPF_ERR_ARG, "%s: wr256[%d] must be finite and >= 0", who, k);
        p.wr[k] = wr256[k];
    }
    const int tiles_x = (W + BIL_TW - 1) / BIL_TW, tiles_y = (H + BIL_TH - 1) / BIL_TH;
    PPF_CHECK_ARG(tiles_y <= 65535, PPF_ERR_SHAPE, "%s: H=%d exceeds the grid", who, H);
    const size_t lds = (size_t)(BIL_TW + 2 * r) * (BIL_TH + 2 * r) * sizeof(float4) + BIL_WR * sizeof(float) + (size_t)D * D * sizeof(float);
    return ppf_launch<bilateral_kernel>(dim3(tiles_x, tiles_y, B), dim3(NT_BEC), lds, stream, who, x, p, r, H, W, out);
}

int ppf_warp_nodes(const void* image_id_i64, uint64_t seed, int B, int s, int amp256, int* nodes, hipStream_t stream) {
    const char* who = "ppf_warp_nodes";
    PPF_CHECK_ARG(B >= 1, PPF_ERR_SHAPE, "%s: B=%d (>= 1)", who, B);
    PPF_CHECK_ARG(s >= 1 && s <= WARP_MAX_S, PPF_ERR_SHAPE, "%s: s=%d grid cells per side outside [1, %d]", who, s, WARP_MAX_S);
    PPF_CHECK_ARG(amp256 >= 0 && amp256 <= WARP_MAX_A, PPF_ERR_ARG, "%s: amplitude %d / 256 pixels outside [0, %d / 256]", who, amp256, WARP_MAX_A);
    PPF_CHECK_ARG(image_id_i64 && nodes, PPF_ERR_ARG, "%s: null pointer", who);
    const int Q = (s + 1) * (s + 1);
    const long long total = (long long)B * Q, blocks = (total + NT_BEC - 1) / NT_BEC;
    PPF_CHECK_ARG(blocks <= INT_MAX, PPF_ERR_SHAPE, "%s: B=%d exceeds the grid", who, B);
    return ppf_launch<warp_nodes_kernel>(dim3((unsigned)blocks), dim3(NT_BEC), 0, stream, who, (const long long*)image_id_i64, seed, Q, amp256, total,
                                         nodes);
}

int ppf_warp_apply(const float* x, const int* nodes, int s, int amp256, int B, int Cc, int H, int W, float* out, hipStream_t stream) {
    const char* who = "ppf_warp_apply";
    if (int rc = image_check(who, B, H, W)) return rc;
    PPF_CHECK_ARG(H == W, PPF_ERR_SHAPE, "%s: H=%d W=%d (square images only)", who, H, W);
    PPF_CHECK_ARG(Cc >= 1 && Cc <= 64, PPF_ERR_SHAPE, "%s: Cc=%d outside [1, 64]", who, Cc);
    PPF_CHECK_ARG(s >= 1 && s <= WARP_MAX_S, PPF_ERR_SHAPE, "%s: s=%d grid cells per side outside [1, %d]", who, s, WARP_MAX_S);
    PPF_CHECK_ARG(amp256 >= 0 && amp256 <= WARP_MAX_A, PPF_ERR_ARG, "%s: amplitude %d / 256 pixels outside [0, %d / 256]", who, amp256, WARP_MAX_A);
    const int c = (H + s - 1) / s;
    PPF_CHECK_ARG(c <= WARP_MAX_C && (long long)c * c * max(amp256, 1) <= INT_MAX, PPF_ERR_SHAPE,
                  "%s: node spacing c=%d = ceil(H=%d / s=%d): c <= %d and c^2 * amplitude <= 2^31 - 1 (int32 interpolation)", who, c, H, s, WARP_MAX_C);
    PPF_CHECK_ARG(x && nodes && out, PPF_ERR_ARG, "%s: null pointer", who);
    PPF_CHECK_ARG(x != out, PPF_ERR_ARG, "%s: out must not be x (a pixel reads its neighbours)", who);
    PPF_CHECK_ARG(((uintptr_t)nodes & 7) == 0, PPF_ERR_ALIGN, "%s: nodes must be 8-byte aligned (a node is one 8-byte load)", who);
    const int plane = H * W;
    const double inv_cc = 1.0 / (double)(c * c);
    const float inv_c = 1.0f / (float)c, inv_w = 1.0f / (float)W;
    const dim3 grid((plane + NT_BEC * WARP_U - 1) / (NT_BEC * WARP_U), B);
    if (Cc == 3) return ppf_launch<warp_apply_kernel<WARP_U, 3>>(grid, dim3(NT_BEC), 0, stream, who, x, nodes, s, c, inv_cc, inv_c, inv_w, amp256, Cc, H, W,
                                                                 out);
    return ppf_launch<warp_apply_kernel<WARP_U, 0>>(grid, dim3(NT_BEC), 0, stream, who, x, nodes, s, c, inv_cc, inv_c, inv_w, amp256, Cc, H, W, out);
}

int ppf_because_score(const float* act_full, const int* idx, const float* act_max, const int* protos, const int* cells, int B, int P, int T, int G, int K,
                      float* same, float* best, int* lost, hipStream_t stream) {
    const char* who = "ppf_because_score";
    PPF_CHECK_ARG(B >= 1 && P >= 1 && K >= 1 && (long long)B * K <= INT_MAX, PPF_ERR_SHAPE, "%s: bad shape B=%d P=%d K=%d", who, B, P, K);
    PPF_CHECK_ARG(act_max && protos && best, PPF_ERR_ARG, "%s: null pointer (act_max, protos, best)", who);
    if (idx) {
        PPF_CHECK_ARG(T >= 1 && G >= 1, PPF_ERR_SHAPE, "%s: T=%d G=%d (both >= 1 on the local branch)", who, T, G);
        PPF_CHECK_ARG(act_full && cells && same && lost, PPF_ERR_ARG, "%s: null pointer (act_full, cells, same, lost go with idx)", who);
    }
    return ppf_launch<because_score_kernel>(dim3((unsigned)(B * K)), dim3(64), 0, stream, who, act_full, idx, act_max, protos, cells, P, T, G, K, same, best,
                                            lost);
}

}  // extern "C"
