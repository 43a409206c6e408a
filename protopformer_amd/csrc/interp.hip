// Interpretability post-processing on the device (interpret.py: resize_cubic, prototype_part_table, find_high_activation_crop; reference
// eval_interpretability.py:206-226, main_visualize.py:44-66,381-398): the g x g activation map of an (image, prototype) pair is
// up-sampled to S x S with the bicubic kernel cv2.INTER_CUBIC uses (Keys, a = -0.75, half-pixel centres, replicated border) and then
// scanned for its peak or for the bounding box of its top entries.
//
//   * The arithmetic is interpret.resize_cubic's, operation for operation, in fp64 with floating-point contraction OFF for this whole
//     file: source coordinate (j + 0.5) * (g / S) - 0.5 (the ratio is divided on the host and passed in, so no kernel here holds a
//     division), the weights by _cubic_weights' expressions with the fourth as 1 - w0 - w1 - w2, axis 0 first and then axis 1, the four
//     taps multiplied and added in index order, one cast to fp32 at the end.  The peak of a map with a symmetric blob is an exact tie;
//     which pixel wins is only defined when the values are the host's, bit for bit.
//   * LDS (dynamic) holds the g x g source as fp64, ONE table of S x 4 weights and S first-tap indices (maps and outputs are square: the
//     row table and the column table are the same table), and the axis-0 result of a band of BAND output rows.  A thread owns four
//     consecutive output columns for the whole launch: their 16 weights and tap indices stay in registers, a row of the band costs it
//     16 LDS reads, and ppf_act_upsample stores the four values as one 16-byte store (consecutive threads, consecutive 16 bytes).
//   * act_upsample_kernel: one workgroup per (map, band).  The other kernels walk all bands of ONE map per workgroup and never write the
//     map: act_peak_kernel keeps (max, first flat index) per thread, reduces by wavefront shuffles and then across the four waves
//     through LDS (equal values resolve to the smaller flat index = np.where(up == up.max())[..][0]), and optionally finishes with the
//     part table of prototype_part_table (fused: the workgroup that found the peak tests it against its image's part list);
//     act_box_kernel reduces the row / column extent of up >= thr; act_order_stats_kernel selects order statistics of the S*S fp32
//     values exactly -- the 4-pass 8-bit radix select over order-preserving keys of rollout.hip (pass steps: ppf_select.h), the map
//     recomputed in every pass instead of being held (S*S values do not fit the registers), integer LDS atomics only.
//   * Foreground focus (interpret.foreground_focus): act_focus_kernel is act_peak_kernel's walk with an object box per image: the same
//     peak, whether it lies in the box, and the fp64 sums of max(v, 0) over the box and over the map; focus_box_terms_kernel and
//     reserve_focus_kernel are the integer kernels around it (box overlap areas; the reserved cells and the rollout scores against the box).
//   * The stability score's two kernels live here too: gauss_noise_kernel adds N(0, sigma^2) noise that is a function of (seed, image id,
//     element) alone (Philox4x32-10 + Box-Muller, accurate logf / sincospif), and part_meter_kernel adds a batch's part tables, and the
//     row equality of a clean and a noisy table, into per-class int32 accumulators (interpret.PartMeter).
// Everything is deterministic: no floating-point atomics, fixed summation order.  A NaN never wins a comparison (a map of NaNs reports
// the peak (0, 0) with value -inf).
#include <limits.h>
#include <math.h>

#include "ppf_common.h"
#include "ppf_hip.h"
#include "ppf_select.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;          // threads per workgroup (4 waves)
constexpr int BAND = 32;         // output rows per band
constexpr int MAX_G = 64, MAX_S = 1024;
constexpr int MAX_LDS = 48 << 10;   // dynamic LDS of a launch; with the 8 KiB of static histograms of the selection it stays inside 64 KiB
constexpr int HCOPIES = 8;      // histogram replicas of the radix select (ppf_select.h)

struct Lds {
    double* src;     // [g][g]
    double* wt;      // [S][4]
    double* tmp;     // [BAND][g]: axis 0 done
    int* i0;         // [S] floor of the source coordinate
};

__host__ __device__ inline size_t act_lds_bytes(int g, int S) { return ((size_t)g * g + 4 * (size_t)S + (size_t)BAND * g) * 8 + (size_t)S * 4; }

__device__ __forceinline__ Lds act_carve(unsigned char* base, int g, int S) {
    Lds L;
    L.src = reinterpret_cast<double*>(base);
    L.wt = L.src + g * g;
    L.tmp = L.wt + 4 * S;
    L.i0 = reinterpret_cast<int*>(L.tmp + BAND * g);
    return L;
}

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

// the source map as fp64 and the weight table (interpret._resize_axis / _cubic_weights)
__device__ void act_stage(const float* __restrict__ grid, const Lds& L, int g, int S, double ratio) {
    for (int i = threadIdx.x; i < g * g; i += NT) L.src[i] = (double)grid[i];
    for (int j = threadIdx.x; j < S; j += NT) {
        const double s = ((double)j + 0.5) * ratio - 0.5;
        const double fl = floor(s);
        const double f = s - fl;
        const double a = -0.75;
        const double t = f + 1.0, u = 1.0 - f;
        const double w0 = ((a * t - 5.0 * a) * t + 8.0 * a) * t - 4.0 * a;
        const double w1 = ((a + 2.0) * f - (a + 3.0)) * f * f + 1.0;
        const double w2 = ((a + 2.0) * u - (a + 3.0)) * u * u + 1.0;
        L.wt[4 * j + 0] = w0;
        L.wt[4 * j + 1] = w1;
        L.wt[4 * j + 2] = w2;
        L.wt[4 * j + 3] = 1.0 - w0 - w1 - w2;
        L.i0[j] = (int)fl;
    }
    __syncthreads();
}

// a thread's four output columns: weights and clamped tap indices, loaded once
struct ColTaps {
    double w[4][4];
    int ix[4][4];
    int col0, nvalid;      // nvalid: columns of the group inside the map (4 except in the last group of an S that is no multiple of 4)
    int rl, rows_par;      // the thread's row lane and the number of row lanes; rl >= rows_par: no work
};

__device__ __forceinline__ void act_taps(ColTaps& T, const Lds& L, int g, int S) {
    const int ncg = (S + 3) >> 2;
    const int cg = threadIdx.x % ncg;
    T.rl = threadIdx.x / ncg;
    T.rows_par = NT / ncg;
    T.col0 = 4 * cg;
    T.nvalid = min(4, S - T.col0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = min(T.col0 + q, S - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            T.w[q][k] = L.wt[4 * j + k];
            T.ix[q][k] = clampi(L.i0[j] + k - 1, g - 1);
        }
    }
}

// Output rows [r0, r0 + rows) of the map: axis 0 into L.tmp, then axis 1 from it.  EVERY thread calls f(row, col0, v, n) the same
// number of times (n = 0: nothing of this call is valid), so f may use wave-wide operations; a thread sees its elements in increasing
// flat index.
template <class F>
__device__ __forceinline__ void act_band(const Lds& L, const ColTaps& T, int g, int S, int r0, int rows, F&& f) {
    for (int it = threadIdx.x; it < rows * g; it += NT) {
        const int r = it / g, c = it - r * g;
        const int j = r0 + r, b = L.i0[j];
        const double* w = L.wt + 4 * j;
        double acc = L.src[clampi(b - 1, g - 1) * g + c] * w[0];
        acc = acc + L.src[clampi(b, g - 1) * g + c] * w[1];
        acc = acc + L.src[clampi(b + 1, g - 1) * g + c] * w[2];
        acc = acc + L.src[clampi(b + 2, g - 1) * g + c] * w[3];
        L.tmp[it] = acc;
    }
    __syncthreads();
    for (int rb = 0; rb < rows; rb += T.rows_par) {
        const int r = rb + T.rl;
        const bool ok = T.rl < T.rows_par && r < rows;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (ok) {
            const double* trow = L.tmp + r * g;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double acc = trow[T.ix[q][0]] * T.w[q][0];
                acc = acc + trow[T.ix[q][1]] * T.w[q][1];
                acc = acc + trow[T.ix[q][2]] * T.w[q][2];
                acc = acc + trow[T.ix[q][3]] * T.w[q][3];
                v[q] = (float)acc;
            }
        }
        f(r0 + r, T.col0, v, ok ? T.nvalid : 0);
    }
    __syncthreads();
}

// ---- 1. the map itself
// VEC: S % 4 == 0 and a 16-byte aligned output, every group of four is one 16-byte store (a template parameter, not a run-time flag: with
// both forms in one function the compiler merges their tails and splits the 16-byte store into 12 + 4)
template <bool VEC>
__global__ __launch_bounds__(NT) void act_upsample_kernel(const float* __restrict__ grids, float* __restrict__ out, int g, int S, double ratio,
                                                          int bands) {
    extern __shared__ __align__(16) unsigned char act_smem[];
    const int m = blockIdx.x / bands, band = blockIdx.x - m * bands;
    const Lds L = act_carve(act_smem, g, S);
    act_stage(grids + (size_t)m * g * g, L, g, S, ratio);
    ColTaps T;
    act_taps(T, L, g, S);
    float* o = out + (size_t)m * S * S;
    const int r0 = band * BAND;
    act_band(L, T, g, S, r0, min(BAND, S - r0), [&](int row, int col0, const float (&v)[4], int n) {
        if (n == 0) return;
        float* p = o + (size_t)row * S + col0;
        if (VEC) {                                        // n == 4
            *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < n) p[q] = v[q];
        }
    });
}

// ---- 2. / 3. peak (+ part table)
// is part p of the image inside the box of half-width `half` around the peak (y, x)?  interpret.in_bbox: inclusive on both ends, the box
// clipped to [0, S]
__device__ __forceinline__ unsigned char part_hit(const int* __restrict__ parts_img, int p, int y, int x, int half, int S) {
    const int valid = parts_img[3 * p], px = parts_img[3 * p + 1], py = parts_img[3 * p + 2];
    const int y0 = max(0, y - half), y1 = min(S, y + half), x0 = max(0, x - half), x1 = min(S, x + half);
    return (valid != 0 && y0 <= py && py <= y1 && x0 <= px && px <= x1) ? 1 : 0;
}

__global__ __launch_bounds__(NT) void act_peak_kernel(const float* __restrict__ grids, int g, int S, double ratio, float* __restrict__ peak_val,
                                                      int* __restrict__ peak_yx, const int* __restrict__ parts, int maps_per_img, int n_parts,
                                                      int half, unsigned char* __restrict__ table) {
    extern __shared__ __align__(16) unsigned char act_smem[];
    __shared__ float red_v[NT / 64];
    __shared__ int red_i[NT / 64];
    __shared__ int peak_s[2];
    const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Lds L = act_carve(act_smem, g, S);
    act_stage(grids + (size_t)m * g * g, L, g, S, ratio);
    ColTaps T;
    act_taps(T, L, g, S);
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int r0 = 0; r0 < S; r0 += BAND)
        act_band(L, T, g, S, r0, min(BAND, S - r0), [&](int row, int col0, const float (&v)[4], int n) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = row * S + col0 + q;
                if (q < n && comes_before(v[q], i, bv, bi)) { bv = v[q]; bi = i; }
            }
        });
    wave_first(bv, bi);
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < NT / 64; ++w)
            if (comes_before(red_v[w], red_i[w], bv, bi)) { bv = red_v[w]; bi = red_i[w]; }
        if (bi == INT_MAX) bi = 0;                        // nothing compared (NaNs only)
        const int y = bi / S, x = bi - y * S;
        peak_val[m] = bv;
        peak_yx[2 * (size_t)m] = y;
        peak_yx[2 * (size_t)m + 1] = x;
        peak_s[0] = y;
        peak_s[1] = x;
    }
    if (table == nullptr) return;                         // uniform
    __syncthreads();
    const int* parts_img = parts + (size_t)(m / maps_per_img) * n_parts * 3;
    for (int p = threadIdx.x; p < n_parts; p += NT) table[(size_t)m * n_parts + p] = part_hit(parts_img, p, peak_s[0], peak_s[1], half, S);
}

__global__ __launch_bounds__(NT) void act_part_table_kernel(const int* __restrict__ peak_yx, long long total, int S, const int* __restrict__ parts,
                                                            int maps_per_img, int n_parts, int half, unsigned char* __restrict__ table) {
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e >= total) return;
    const long long m = e / n_parts;
    const int p = (int)(e - m * n_parts);
    table[e] = part_hit(parts + (size_t)(m / maps_per_img) * n_parts * 3, p, peak_yx[2 * m], peak_yx[2 * m + 1], half, S);
}

// ---- 4. bounding box of up >= thr
__global__ __launch_bounds__(NT) void act_box_kernel(const float* __restrict__ grids, const double* __restrict__ thr, int g, int S, double ratio,
                                                     int* __restrict__ box) {
    extern __shared__ __align__(16) unsigned char act_smem[];
    __shared__ int red[NT / 64][4];
    const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Lds L = act_carve(act_smem, g, S);
    act_stage(grids + (size_t)m * g * g, L, g, S, ratio);
    ColTaps T;
    act_taps(T, L, g, S);
    const double t = thr[m];
    int e[4] = {INT_MAX, -1, INT_MAX, -1};                // min row, max row, min column, max column
    for (int r0 = 0; r0 < S; r0 += BAND)
        act_band(L, T, g, S, r0, min(BAND, S - r0), [&](int row, int col0, const float (&v)[4], int n) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < n && (double)v[q] >= t) {
                    e[0] = min(e[0], row); e[1] = max(e[1], row);
                    e[2] = min(e[2], col0 + q); e[3] = max(e[3], col0 + q);
                }
        });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        e[0] = min(e[0], __shfl_xor(e[0], o, 64)); e[1] = max(e[1], __shfl_xor(e[1], o, 64));
        e[2] = min(e[2], __shfl_xor(e[2], o, 64)); e[3] = max(e[3], __shfl_xor(e[3], o, 64));
    }
    if (lane == 0) { red[wave][0] = e[0]; red[wave][1] = e[1]; red[wave][2] = e[2]; red[wave][3] = e[3]; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) {
            e[0] = min(e[0], red[w][0]); e[1] = max(e[1], red[w][1]);
            e[2] = min(e[2], red[w][2]); e[3] = max(e[3], red[w][3]);
        }
        int* b = box + 4 * (size_t)m;
        if (e[1] < 0) { b[0] = 0; b[1] = 1; b[2] = 0; b[3] = 1; }          // nothing passes: find_high_activation_crop's (0, 1, 0, 1)
        else { b[0] = e[0]; b[1] = e[1] + 1; b[2] = e[2]; b[3] = e[3] + 1; }
    }
}

// ---- 5. foreground focus: the peak, and the positive mass of the map inside / outside an object box
// an object box (y0, y1, x0, x1), half-open, clipped to [0, S]; empty: the upper end is not above the lower one
struct ObjBox { int y0, y1, x0, x1; };
__device__ __forceinline__ ObjBox obj_clip(const int* __restrict__ o, int S) {
    return ObjBox{clampi(o[0], S), clampi(o[1], S), clampi(o[2], S), clampi(o[3], S)};
}

// act_peak_kernel's walk and its peak, element for element, plus two fp64 sums per thread: max(v, 0) of the finite values over the map and
// over the box.  A thread's columns never change, so their box test is made once; the row's is uniform over a call.  The sums are
// reduced by wavefront shuffles and then over the four waves in index order: a fixed order, no atomics.
__global__ __launch_bounds__(NT) void act_focus_kernel(const float* __restrict__ grids, const int* __restrict__ obj, int g, int S, double ratio,
                                                       int maps_per_img, float* __restrict__ peak_val, int* __restrict__ peak_yx, int* __restrict__ hit,
                                                       double* __restrict__ inside, double* __restrict__ total, int* __restrict__ nonfinite) {
    extern __shared__ __align__(16) unsigned char act_smem[];
    __shared__ float red_v[NT / 64];
    __shared__ int red_i[NT / 64], red_n[NT / 64];
    __shared__ double red_in[NT / 64], red_tot[NT / 64];
    const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Lds L = act_carve(act_smem, g, S);
    act_stage(grids + (size_t)m * g * g, L, g, S, ratio);
    ColTaps T;
    act_taps(T, L, g, S);
    const ObjBox ob = obj_clip(obj + 4 * (size_t)(m / maps_per_img), S);
    bool cin[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) cin[q] = T.col0 + q >= ob.x0 && T.col0 + q < ob.x1;
    float bv = -INFINITY;
    int bi = INT_MAX, nf = 0;
    double s_in = 0.0, s_tot = 0.0;
    for (int r0 = 0; r0 < S; r0 += BAND)
        act_band(L, T, g, S, r0, min(BAND, S - r0), [&](int row, int col0, const float (&v)[4], int n) {
            const bool rin = row >= ob.y0 && row < ob.y1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = row * S + col0 + q;
                if (q < n && comes_before(v[q], i, bv, bi)) { bv = v[q]; bi = i; }
                const bool fin = fabsf(v[q]) < INFINITY;                      // false for NaN and +-inf
                const double pos = (q < n && fin && v[q] > 0.0f) ? (double)v[q] : 0.0;
                nf += (q < n && !fin) ? 1 : 0;
                s_tot += pos;
                s_in += (rin && cin[q]) ? pos : 0.0;
            }
        });
    wave_first(bv, bi);
    s_in = wave_sum_f64(s_in);
    s_tot = wave_sum_f64(s_tot);
    nf = wave_sum_i32(nf);
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; red_in[wave] = s_in; red_tot[wave] = s_tot; red_n[wave] = nf; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) {
            if (comes_before(red_v[w], red_i[w], bv, bi)) { bv = red_v[w]; bi = red_i[w]; }
            s_in += red_in[w];
            s_tot += red_tot[w];
            nf += red_n[w];
        }
        if (bi == INT_MAX) bi = 0;                        // nothing compared (NaNs only)
        const int y = bi / S, x = bi - y * S;
        peak_val[m] = bv;
        peak_yx[2 * (size_t)m] = y;
        peak_yx[2 * (size_t)m + 1] = x;
        hit[m] = (y >= ob.y0 && y < ob.y1 && x >= ob.x0 && x < ob.x1) ? 1 : 0;
        inside[m] = s_in;
        total[m] = s_tot;
        if (nonfinite) nonfinite[m] = nf;
    }
}

// (intersection, box, object, union) areas of the clipped boxes: integers only, one thread per map
__global__ __launch_bounds__(NT) void focus_box_terms_kernel(const int* __restrict__ box, const int* __restrict__ obj, int M, int maps_per_img, int S,
                                                             int* __restrict__ terms) {
    const int m = blockIdx.x * NT + threadIdx.x;
    if (m >= M) return;
    const ObjBox a = obj_clip(box + 4 * (size_t)m, S), o = obj_clip(obj + 4 * (size_t)(m / maps_per_img), S);
    const int abox = max(a.y1 - a.y0, 0) * max(a.x1 - a.x0, 0), aobj = max(o.y1 - o.y0, 0) * max(o.x1 - o.x0, 0);
    const int inter = (abox > 0 && aobj > 0) ? max(min(a.y1, o.y1) - max(a.y0, o.y0), 0) * max(min(a.x1, o.x1) - max(a.x0, o.x0), 0) : 0;
    int* t = terms + 4 * (size_t)m;
    t[0] = inter; t[1] = abox; t[2] = aobj; t[3] = abox + aobj - inter;
}

// is the centre pixel of grid cell c inside the (clipped) box?
__device__ __forceinline__ bool cell_centre_in(int c, int g, int patch, const ObjBox& ob) {
    const int cy = c / g, cx = c - cy * g;
    const int py = cy * patch + patch / 2, px = cx * patch + patch / 2;
    return py >= ob.y0 && py < ob.y1 && px >= ob.x0 && px < ob.x1;
}

// One workgroup per image: the reserved cells against the box (integers), and the rollout scores over the cells whose centre is inside
// (fp64, a thread's cells in ascending order, then shuffles, then the waves in index order).
__global__ __launch_bounds__(NT) void reserve_focus_kernel(const int* __restrict__ idx, const int* __restrict__ obj, const float* __restrict__ token_attn,
                                                           int T, int g, int patch, int* __restrict__ out, double* __restrict__ attn) {
    __shared__ int red_i[NT / 64][4];
    __shared__ double red_d[NT / 64][2];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, G = g * g;
    const ObjBox ob = obj_clip(obj + 4 * (size_t)b, g * patch);
    int e[4] = {0, 0, 0, 0};
    for (int t = threadIdx.x; t < T; t += NT) {
        const int c = idx[(size_t)b * T + t];
        if (c < 0 || c >= G) continue;
        const int cy = c / g, cx = c - cy * g;
        const int oy = max(min((cy + 1) * patch, ob.y1) - max(cy * patch, ob.y0), 0), ox = max(min((cx + 1) * patch, ob.x1) - max(cx * patch, ob.x0), 0);
        e[0] += oy * ox;
        e[1] += cell_centre_in(c, g, patch, ob) ? 1 : 0;
        e[3] += 1;
    }
    double a_in = 0.0, a_all = 0.0;
    for (int c = threadIdx.x; c < G; c += NT) {
        const bool in = cell_centre_in(c, g, patch, ob);
        e[2] += in ? 1 : 0;
        if (token_attn) {
            const float v = token_attn[(size_t)b * G + c];
            const double d = fabsf(v) < INFINITY ? (double)v : 0.0;
            a_all += d;
            a_in += in ? d : 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = wave_sum_i32(e[k]);
    a_in = wave_sum_f64(a_in);
    a_all = wave_sum_f64(a_all);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red_i[wave][k] = e[k];
        red_d[wave][0] = a_in; red_d[wave][1] = a_all;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) {
#pragma unroll
            for (int k = 0; k < 4; ++k) e[k] += red_i[w][k];
            a_in += red_d[w][0]; a_all += red_d[w][1];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) out[4 * (size_t)b + k] = e[k];
        if (token_attn) { attn[2 * (size_t)b] = a_in; attn[2 * (size_t)b + 1] = a_all; }
    }
}

// ---- order statistics of the S*S fp32 values
// ranks are 0-based in ascending order, k_lo <= k_hi <= k_lo + 1
__global__ __launch_bounds__(NT) void act_order_stats_kernel(const float* __restrict__ grids, int g, int S, double ratio, int k_lo, int k_hi,
                                                             float* __restrict__ stats) {
    extern __shared__ __align__(16) unsigned char act_smem[];
    __shared__ uint32_t hist[HCOPIES * RADIX_HSTRIDE];
    __shared__ uint32_t misc[16];
    const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Lds L = act_carve(act_smem, g, S);
    act_stage(grids + (size_t)m * g * g, L, g, S, ratio);
    ColTaps T;
    act_taps(T, L, g, S);
    uint32_t prefix = 0;
    int remaining = k_lo + 1;                             // 1-based rank among the keys that share the prefix
    const int hcopy = radix_replica<HCOPIES>();
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        radix_clear<HCOPIES>(hist, NT);
        for (int r0 = 0; r0 < S; r0 += BAND)
            act_band(L, T, g, S, r0, min(BAND, S - r0), [&](int, int, const float (&v)[4], int n) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t key = order_key(v[q]);
                    const bool in = q < n && (pass == 0 || (key >> (shift + 8)) == prefix);
                    const uint32_t bin = (key >> shift) & 255u;
                    // activation maps are mostly one value: when the wave's keys share a bin, one lane adds their count
                    const unsigned long long mm = __ballot(in);
                    if (mm == 0) continue;                                   // wave-uniform
                    const int leader = __ffsll((long long)mm) - 1;
                    const uint32_t b0 = __shfl(bin, leader, 64);
                    const unsigned long long eq = __ballot(in && bin == b0);
                    if (eq == mm) {
                        if (lane == leader) atomicAdd(&hist[hcopy + b0], (uint32_t)__popcll(mm));
                    } else if (in) {
                        atomicAdd(&hist[hcopy + bin], 1u);
                    }
                }
            });
        // The pass's closing scan, this kernel's own (every thread scans, a barrier behind the misc reads): through radix_close of
        // ppf_select.h the kernel measured +1.3 % on near-constant maps against a parent spread of 0.7 % (MEASUREMENTS.md 5l).
        uint32_t cnt = 0;
#pragma unroll
        for (int c = 0; c < HCOPIES; ++c) cnt += hist[c * RADIX_HSTRIDE + threadIdx.x];
        uint32_t cum = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t nb = __shfl_up(cum, o, 64);
            if (lane >= o) cum += nb;
        }
        if (lane == 63) misc[wave] = cum;
        __syncthreads();
        for (int w = 0; w < wave; ++w) cum += misc[w];
        const uint32_t before = cum - cnt;
        if ((uint32_t)remaining > before && (uint32_t)remaining <= cum) { misc[8] = threadIdx.x; misc[9] = before; misc[10] = cnt; }
        __syncthreads();
        prefix = (prefix << 8) | misc[8];
        remaining -= (int)misc[9];
        __syncthreads();
    }
    // prefix = the key of rank k_lo; remaining - 1 keys equal to it come before that rank, misc[10] keys equal it in all
    const int n_le = (k_lo + 1 - remaining) + (int)misc[10];      // keys <= prefix
    uint32_t key_hi = prefix;
    if (k_hi > k_lo && n_le < k_hi + 1) {                 // uniform: the next rank is the smallest key above
        if (threadIdx.x == 0) misc[11] = 0xFFFFFFFFu;
        __syncthreads();
        uint32_t mn = 0xFFFFFFFFu;
        for (int r0 = 0; r0 < S; r0 += BAND)
            act_band(L, T, g, S, r0, min(BAND, S - r0), [&](int, int, const float (&v)[4], int n) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t key = order_key(v[q]);
                    if (q < n && key > prefix) mn = min(mn, key);
                }
            });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
        if (lane == 0) atomicMin(&misc[11], mn);
        __syncthreads();
        key_hi = misc[11];
    }
    if (threadIdx.x == 0) {
        stats[2 * (size_t)m] = key_value(prefix);
        stats[2 * (size_t)m + 1] = key_value(key_hi);
    }
}

// ---- stability score: Gaussian input noise per image, and the per-class accumulators of both scores
// Four standard normals of elements 4q .. 4q+3 of image `id`: one Philox4x32-10 call, counter (q, image id), key = seed, two Box-Muller
// pairs.  Uniforms on the 24-bit grid as the input finisher builds them (u0, u2 in (0, 1): the logarithm is finite; u1, u3 in [0, 1)).
// logf / sincospif are the accurate library functions: 2 * u is exact in fp32, so the argument of sincospif carries no rounding error.
// PPF_NOISE_KO: measurement builds only (scripts/bench_stability.py --knockouts; the noise they make is wrong on purpose): 1 = a counter hash
// in place of Philox, 2 = the fast logarithm, 3 = the fast sine / cosine.
#ifndef PPF_NOISE_KO
#define PPF_NOISE_KO 0
#endif
__device__ __forceinline__ void gauss4(uint64_t seed, uint64_t id, uint64_t q, float (&n)[4]) {
#if PPF_NOISE_KO == 1
    const uint32_t h = ((uint32_t)q * 0x9E3779B9u) ^ (uint32_t)id ^ (uint32_t)seed;
    const uint4 r = make_uint4(h, h * 0x85EBCA6Bu, h ^ 0xC2B2AE35u, h * 0x27D4EB2Fu);
#else
    const uint4 r = philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)id, (uint32_t)(id >> 32)),
                                  make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
#endif
    const float u0 = ((float)(r.x >> 8) + 0.5f) * (1.0f / 16777216.0f), u1 = (float)(r.y >> 8) * (1.0f / 16777216.0f);
    const float u2 = ((float)(r.z >> 8) + 0.5f) * (1.0f / 16777216.0f), u3 = (float)(r.w >> 8) * (1.0f / 16777216.0f);
#if PPF_NOISE_KO == 2
    const float m0 = sqrtf(-2.0f * __logf(u0)), m1 = sqrtf(-2.0f * __logf(u2));
#else
    const float m0 = sqrtf(-2.0f * logf(u0)), m1 = sqrtf(-2.0f * logf(u2));
#endif
    float s0, c0, s1, c1;
#if PPF_NOISE_KO == 3
    s0 = __sinf(6.283185307f * u1); c0 = __cosf(6.283185307f * u1); s1 = __sinf(6.283185307f * u3); c1 = __cosf(6.283185307f * u3);
#else
    sincospif(2.0f * u1, &s0, &c0);
    sincospif(2.0f * u3, &s1, &c1);
#endif
    n[0] = m0 * c0; n[1] = m0 * s0; n[2] = m1 * c1; n[3] = m1 * s1;
}

// out[b][e] = fmaf(sigma, n(seed, id[b], e), x[b][e]); a lane owns one group of four elements of one image per iteration.  x and out may
// be the same buffer (no __restrict__): a lane reads its group before it writes it and no other lane touches it.  blockIdx.y strides over
// the images and blockIdx.x over an image's groups, so no index is divided.
// VEC: n_per_img % 4 == 0 and both pointers 16-byte aligned, every group is one 16-byte load and one 16-byte store (a template
// parameter for the reason given at act_upsample_kernel).
template <bool VEC>
__global__ __launch_bounds__(NT) void gauss_noise_kernel(const float* x, float* out, const long long* __restrict__ image_id, int B, int groups_per_img,
                                                         long long n_per_img, float sigma, uint64_t seed) {
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const uint64_t id = (uint64_t)image_id[b];
        const float* xb = x + (long long)b * n_per_img;
        float* ob = out + (long long)b * n_per_img;
        for (int q = blockIdx.x * NT + threadIdx.x; q < groups_per_img; q += gridDim.x * NT) {      // groups_per_img <= 2^29, the stride <= 2^19
            float n[4];
            gauss4(seed, id, (uint64_t)q, n);
            const long long e0 = 4ll * q;
            if (VEC) {
                const float4 v = *reinterpret_cast<const float4*>(xb + e0);
                *reinterpret_cast<float4*>(ob + e0) = make_float4(fmaf(sigma, n[0], v.x), fmaf(sigma, n[1], v.y), fmaf(sigma, n[2], v.z), fmaf(sigma, n[3], v.w));
            } else {
                const int cnt = (int)min(4ll, n_per_img - e0);             // the surplus draws of an image's last group are dropped
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < cnt) ob[e0 + j] = fmaf(sigma, n[j], xb[e0 + j]);
            }
        }
    }
}

// One workgroup per image: the image's tables into the accumulators of its class.  Integer atomics only, zeros are not added: any split
// of the same images into batches, in any order, leaves the same integers.
__global__ __launch_bounds__(NT) void part_meter_kernel(const unsigned char* __restrict__ table, const unsigned char* __restrict__ noisy,
                                                        const int* __restrict__ parts, const long long* __restrict__ label, int ppc, int n_parts, int C,
                                                        int* __restrict__ hits, int* __restrict__ visible, int* __restrict__ stable,
                                                        int* __restrict__ images, int* __restrict__ bad) {
    const int b = blockIdx.x;
    const long long c = label[b];
    if (c < 0 || c >= C) {                                            // uniform
        if (threadIdx.x == 0) atomicAdd(bad, 1);
        return;
    }
    if (threadIdx.x == 0) atomicAdd(images + c, 1);
    const int* pl = parts + (size_t)b * n_parts * 3;
    for (int q = threadIdx.x; q < n_parts; q += NT)
        if (pl[3 * q] != 0) atomicAdd(visible + c * n_parts + q, 1);
    const int per = ppc * n_parts;
    const unsigned char* t = table + (size_t)b * per;
    for (int e = threadIdx.x; e < per; e += NT)
        if (t[e] != 0) atomicAdd(hits + c * per + e, (int)t[e]);
    if (noisy == nullptr) return;                                     // uniform
    const unsigned char* tn = noisy + (size_t)b * per;
    for (int p = threadIdx.x; p < ppc; p += NT) {
        bool same = true;
        for (int q = 0; q < n_parts; ++q) same = same && t[p * n_parts + q] == tn[p * n_parts + q];
        if (same) atomicAdd(stable + c * ppc + p, 1);
    }
}

int act_check(const char* fn, const void* grids, int M, int g, int S) {
    PPF_CHECK_ARG(M >= 1 && g >= 1 && g <= MAX_G && S >= 1 && S <= MAX_S, PPF_ERR_SHAPE,
                  "%s: bad shape M=%d g=%d S=%d (M >= 1, 1 <= g <= %d, 1 <= S <= %d)", fn, M, g, S, MAX_G, MAX_S);
    PPF_CHECK_ARG(act_lds_bytes(g, S) <= MAX_LDS, PPF_ERR_SHAPE, "%s: g=%d S=%d need %zu bytes of LDS (limit %d)", fn, g, S, act_lds_bytes(g, S), MAX_LDS);
    PPF_CHECK_ARG(grids != nullptr, PPF_ERR_ARG, "%s: null pointer", fn);
    return 0;
}

int parts_check(const char* fn, int M, const void* parts, int maps_per_img, int n_parts, int half_size, const void* table) {
    PPF_CHECK_ARG(maps_per_img >= 1 && M % maps_per_img == 0 && n_parts >= 1 && n_parts <= 65536, PPF_ERR_SHAPE,
                  "%s: bad part list M=%d maps_per_img=%d n_parts=%d (M a multiple of maps_per_img >= 1, 1 <= n_parts <= 65536)", fn, M, maps_per_img,
                  n_parts);
    PPF_CHECK_ARG(half_size >= 0 && half_size <= (1 << 30), PPF_ERR_ARG, "%s: half_size=%d outside [0, 2^30]", fn, half_size);
    PPF_CHECK_ARG(parts != nullptr && table != nullptr, PPF_ERR_ARG, "%s: null pointer", fn);
    return 0;
}

}  // namespace

extern "C" {

int ppf_act_upsample(const float* grids, float* out, int M, int g, int S, hipStream_t stream) {
    if (int rc = act_check("ppf_act_upsample", grids, M, g, S)) return rc;
    PPF_CHECK_ARG(out != nullptr, PPF_ERR_ARG, "ppf_act_upsample: null pointer");
    const int bands = (S + BAND - 1) / BAND;
    PPF_CHECK_ARG((long long)M * bands <= INT_MAX, PPF_ERR_SHAPE, "ppf_act_upsample: M=%d maps of %d bands exceed the grid", M, bands);
    if (S % 4 == 0 && ((uintptr_t)out & 15) == 0)
        return ppf_launch<act_upsample_kernel<true>>(dim3((unsigned)(M * bands)), dim3(NT), act_lds_bytes(g, S), stream, "ppf_act_upsample", grids, out, g, S,
                                                     (double)g / (double)S, bands);
    return ppf_launch<act_upsample_kernel<false>>(dim3((unsigned)(M * bands)), dim3(NT), act_lds_bytes(g, S), stream, "ppf_act_upsample", grids, out, g, S,
                                                  (double)g / (double)S, bands);
}

int ppf_act_peak(const float* grids, int M, int g, int S, float* peak_val, int* peak_yx, const int* parts, int maps_per_img, int n_parts,
                 int half_size, void* table_u8, hipStream_t stream) {
    if (int rc = act_check("ppf_act_peak", grids, M, g, S)) return rc;
    PPF_CHECK_ARG(peak_val != nullptr && peak_yx != nullptr, PPF_ERR_ARG, "ppf_act_peak: null pointer");
    PPF_CHECK_ARG((parts == nullptr) == (table_u8 == nullptr), PPF_ERR_ARG, "ppf_act_peak: parts and table_u8 must both be given or both be NULL");
    if (parts != nullptr)
        if (int rc = parts_check("ppf_act_peak", M, parts, maps_per_img, n_parts, half_size, table_u8)) return rc;
    return ppf_launch<act_peak_kernel>(dim3((unsigned)M), dim3(NT), act_lds_bytes(g, S), stream, "ppf_act_peak", grids, g, S, (double)g / (double)S, peak_val,
                                       peak_yx, parts, maps_per_img, n_parts, half_size, (unsigned char*)table_u8);
}

int ppf_act_part_table(const int* peak_yx, int M, int S, const int* parts, int maps_per_img, int n_parts, int half_size, void* table_u8,
                       hipStream_t stream) {
    PPF_CHECK_ARG(M >= 1 && S >= 1, PPF_ERR_SHAPE, "ppf_act_part_table: bad shape M=%d S=%d", M, S);
    if (int rc = parts_check("ppf_act_part_table", M, parts, maps_per_img, n_parts, half_size, table_u8)) return rc;
    PPF_CHECK_ARG(peak_yx != nullptr, PPF_ERR_ARG, "ppf_act_part_table: null pointer");
    const long long total = (long long)M * n_parts, blocks = (total + NT - 1) / NT;
    PPF_CHECK_ARG(blocks <= INT_MAX, PPF_ERR_SHAPE, "ppf_act_part_table: M=%d x n_parts=%d exceeds the grid", M, n_parts);
    return ppf_launch<act_part_table_kernel>(dim3((unsigned)blocks), dim3(NT), 0, stream, "ppf_act_part_table", peak_yx, total, S, parts, maps_per_img, n_parts,
                                             half_size, (unsigned char*)table_u8);
}

int ppf_act_order_stats(const float* grids, int M, int g, int S, int k_lo, int k_hi, float* stats, hipStream_t stream) {
    if (int rc = act_check("ppf_act_order_stats", grids, M, g, S)) return rc;
    PPF_CHECK_ARG(k_lo >= 0 && k_hi >= k_lo && k_hi <= k_lo + 1 && k_hi < S * S, PPF_ERR_ARG,
                  "ppf_act_order_stats: ranks k_lo=%d k_hi=%d must satisfy 0 <= k_lo <= k_hi <= k_lo + 1, k_hi < S*S=%d", k_lo, k_hi, S * S);
    PPF_CHECK_ARG(stats != nullptr, PPF_ERR_ARG, "ppf_act_order_stats: null pointer");
    return ppf_launch<act_order_stats_kernel>(dim3((unsigned)M), dim3(NT), act_lds_bytes(g, S), stream, "ppf_act_order_stats", grids, g, S, (double)g / (double)S, k_lo,
                                              k_hi, stats);
}

int ppf_act_box(const float* grids, const double* thr, int M, int g, int S, int* box, hipStream_t stream) {
    if (int rc = act_check("ppf_act_box", grids, M, g, S)) return rc;
    PPF_CHECK_ARG(thr != nullptr && box != nullptr, PPF_ERR_ARG, "ppf_act_box: null pointer");
    return ppf_launch<act_box_kernel>(dim3((unsigned)M), dim3(NT), act_lds_bytes(g, S), stream, "ppf_act_box", grids, thr, g, S, (double)g / (double)S, box);
}

int ppf_act_focus(const float* grids, const int* obj, int M, int g, int S, int maps_per_img, float* peak_val, int* peak_yx, int* hit, double* inside,
                  double* total, int* nonfinite, hipStream_t stream) {
    if (int rc = act_check("ppf_act_focus", grids, M, g, S)) return rc;
    PPF_CHECK_ARG(maps_per_img >= 1 && M % maps_per_img == 0, PPF_ERR_SHAPE, "ppf_act_focus: M=%d maps are no multiple of maps_per_img=%d (>= 1)", M,
                  maps_per_img);
    PPF_CHECK_ARG(obj != nullptr && peak_val != nullptr && peak_yx != nullptr && hit != nullptr && inside != nullptr && total != nullptr, PPF_ERR_ARG,
                  "ppf_act_focus: null pointer (only nonfinite may be NULL)");
    return ppf_launch<act_focus_kernel>(dim3((unsigned)M), dim3(NT), act_lds_bytes(g, S), stream, "ppf_act_focus", grids, obj, g, S, (double)g / (double)S,
                                        maps_per_img, peak_val, peak_yx, hit, inside, total, nonfinite);
}

int ppf_focus_box_terms(const int* box, const int* obj, int M, int maps_per_img, int S, int* terms, hipStream_t stream) {
    PPF_CHECK_ARG(M >= 1 && S >= 1 && S <= 32768, PPF_ERR_SHAPE, "ppf_focus_box_terms: bad shape M=%d S=%d (M >= 1, 1 <= S <= 32768)", M, S);
    PPF_CHECK_ARG(maps_per_img >= 1 && M % maps_per_img == 0, PPF_ERR_SHAPE, "ppf_focus_box_terms: M=%d boxes are no multiple of maps_per_img=%d (>= 1)", M,
                  maps_per_img);
    PPF_CHECK_ARG(box != nullptr && obj != nullptr && terms != nullptr, PPF_ERR_ARG, "ppf_focus_box_terms: null pointer");
    return ppf_launch<focus_box_terms_kernel>(dim3((unsigned)((M + NT - 1) / NT)), dim3(NT), 0, stream, "ppf_focus_box_terms", box, obj, M, maps_per_img, S,
                                              terms);
}

int ppf_reserve_focus(const int* idx, const int* obj, const float* token_attn, int B, int T, int g, int patch, int* out, double* attn, hipStream_t stream) {
    PPF_CHECK_ARG(B >= 1 && T >= 1 && g >= 1 && patch >= 1 && (long long)g * patch <= 32768, PPF_ERR_SHAPE,
                  "ppf_reserve_focus: bad shape B=%d T=%d g=%d patch=%d (all >= 1, g * patch <= 32768)", B, T, g, patch);
    PPF_CHECK_ARG((long long)T * patch * patch <= INT_MAX, PPF_ERR_SHAPE, "ppf_reserve_focus: T=%d cells of patch=%d pixels squared overflow int32", T, patch);
    PPF_CHECK_ARG(idx != nullptr && obj != nullptr && out != nullptr, PPF_ERR_ARG, "ppf_reserve_focus: null pointer");
    PPF_CHECK_ARG((token_attn == nullptr) == (attn == nullptr), PPF_ERR_ARG, "ppf_reserve_focus: token_attn and attn must both be given or both be NULL");
    return ppf_launch<reserve_focus_kernel>(dim3((unsigned)B), dim3(NT), 0, stream, "ppf_reserve_focus", idx, obj, token_attn, T, g, patch, out, attn);
}

int ppf_add_gauss_noise(const float* x, float* out, int B, int64_t n_per_img, const void* image_id_i64, float sigma, uint64_t seed, hipStream_t stream) {
    PPF_CHECK_ARG(B >= 1 && n_per_img >= 1 && n_per_img <= (1ll << 31), PPF_ERR_SHAPE,
                  "ppf_add_gauss_noise: bad shape B=%d n_per_img=%lld (B >= 1, 1 <= n_per_img <= 2^31)", B, (long long)n_per_img);
    PPF_CHECK_ARG(isfinite(sigma) && sigma >= 0.0f, PPF_ERR_SHAPE, "ppf_add_gauss_noise: sigma=%g must be finite and >= 0", (double)sigma);
    PPF_CHECK_ARG(x != nullptr && out != nullptr && image_id_i64 != nullptr, PPF_ERR_ARG, "ppf_add_gauss_noise: null pointer");
    // at most 2048 workgroups, as the element-wise kernels: y over the images, x over an image's groups of four
    const int gpi = (int)((n_per_img + 3) / 4), gy = B < 2048 ? B : 2048, per_img = (gpi + NT - 1) / NT, gx = per_img < 2048 / gy ? per_img : 2048 / gy;
    const dim3 grid((unsigned)(gx < 1 ? 1 : gx), (unsigned)gy);
    if (n_per_img % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0)
        return ppf_launch<gauss_noise_kernel<true>>(grid, dim3(NT), 0, stream, "ppf_add_gauss_noise", x, out, (const long long*)image_id_i64, B, gpi,
                                                    (long long)n_per_img, sigma, seed);
    return ppf_launch<gauss_noise_kernel<false>>(grid, dim3(NT), 0, stream, "ppf_add_gauss_noise", x, out, (const long long*)image_id_i64, B, gpi,
                                                 (long long)n_per_img, sigma, seed);
}

int ppf_part_meter_update(const void* table_u8, const void* table_noisy_u8, const int* parts, const void* label_i64, int B, int ppc, int n_parts, int C,
                          int* hits, int* visible, int* stable, int* images, int* bad, hipStream_t stream) {
    PPF_CHECK_ARG(B >= 1 && ppc >= 1 && n_parts >= 1 && n_parts <= 65536 && C >= 1 && (long long)C * ppc * n_parts <= INT_MAX, PPF_ERR_SHAPE,
                  "ppf_part_meter_update: bad shape B=%d ppc=%d n_parts=%d C=%d (all >= 1, n_parts <= 65536, C * ppc * n_parts < 2^31)", B, ppc, n_parts, C);
    PPF_CHECK_ARG(table_u8 != nullptr && parts != nullptr && label_i64 != nullptr && hits != nullptr && visible != nullptr && stable != nullptr &&
                      images != nullptr && bad != nullptr,
                  PPF_ERR_ARG, "ppf_part_meter_update: null pointer (only table_noisy_u8 may be NULL)");
    return ppf_launch<part_meter_kernel>(dim3((unsigned)B), dim3(NT), 0, stream, "ppf_part_meter_update", (const unsigned char*)table_u8,
                                         (const unsigned char*)table_noisy_u8, parts, (const long long*)label_i64, ppc, n_parts, C, hits, visible, stable,
                                         images, bad);
}

}  // extern "C"
