// Device-resident data sets: crop, flip and RandAugment on uint8 frames, bit-equal to Pillow (the contract is in include/ppf_hip.h).
// The decoded originals lie in one flat buffer; a batch is produced from them without the host touching a pixel.  The reference does all
// of this in CPU workers (tools/datasets.py:280-336 through timm's create_transform).
//   * resize_taps_kernel: one thread per output coordinate of one axis of one sample: Pillow's precompute_coeffs + normalize_coeffs_8bpc in
//     fp64 (IEEE + - * / in source order, no contraction), the integer taps written to the workspace.
//   * resize_h_kernel / resize_v_kernel: Pillow's two 8-bit passes in int32; the horizontal result is rounded to uint8 in the workspace, only
//     for the source rows the window's vertical taps need.  A thread owns one pixel (three channels); neighbouring lanes read overlapping
//     byte runs of one source row, which the vector L1 serves.
//   * aug_hist_kernel: per-sample histograms, LDS integer atomics flushed with global integer atomics (exact at any launch shape).
//   * aug_lut_kernel: a workgroup per sample, a lane per table entry.
//   * aug_apply_kernel / aug_sharpness_kernel / aug_affine_kernel: a lane per pixel; each writes only the samples whose op is its own.
// Deterministic: integer atomics only.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "ppf_common.h"
#include "ppf_hip.h"

// Every floating-point expression below is written in the order Pillow's C evaluates it and must round after every operation.
#pragma clang fp contract(off)

#include "device_data_plan.h"      // plan validation, workspace layout and the tap arithmetic (also built stand-alone on the host by the tests)

namespace {

int rc_checked_layout(const char* who, const double* plan, int B, int H, int W, int filter, int64_t flat_bytes, RcLayout* L) {
    char err[320];
    const int rc = rc_layout(who, plan, B, H, W, filter, flat_bytes, L, err, sizeof(err));
    if (rc) ppf_set_error("%s", err);
    return rc;
}

// entry t of sample b: t < W the column x0 + t of the window, else the row y0 + t - W
__global__ __launch_bounds__(NT_DD) void resize_taps_kernel(const double* __restrict__ plan, int B, int H, int W, int filter, int kmax, int* __restrict__ taps,
                                                            int* __restrict__ bounds) {
    const long long e = (long long)blockIdx.x * NT_DD + threadIdx.x;
    if (e >= (long long)B * (H + W)) return;
    const int b = (int)(e / (H + W)), t = (int)(e - (long long)b * (H + W));
    const double* __restrict__ p = plan + (size_t)b * PPF_RC_WORDS;
    const bool is_x = t < W;
    int xmin, n;
    rc_taps(filter, (int)(is_x ? p[2] : p[1]), is_x ? p[3] : p[4], is_x ? p[5] : p[6], (int)(is_x ? p[8] : p[7]), is_x ? (int)p[10] + t : (int)p[9] + t - W, kmax,
            taps + (size_t)e * kmax, &xmin, &n);
    bounds[e * 2 + 0] = xmin;
    bounds[e * 2 + 1] = n;
}

__device__ __forceinline__ unsigned char rc_clip8(int v) {
    v >>= 22;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// thread = (b, r, x): source row first_b + r of sample b, window column x
__global__ __launch_bounds__(NT_DD) void resize_h_kernel(const unsigned char* __restrict__ flat, const double* __restrict__ plan, int B, int H, int W,
                                                         int kmax, int maxrows, const int* __restrict__ taps, const int* __restrict__ bounds,
                                                         unsigned char* __restrict__ rows) {
    const long long e = (long long)blockIdx.x * NT_DD + threadIdx.x;
    if (e >= (long long)B * maxrows * W) return;
    const int x = (int)(e % W), r = (int)((e / W) % maxrows), b = (int)(e / ((long long)W * maxrows));
    const double* __restrict__ p = plan + (size_t)b * PPF_RC_WORDS;
    const int h = (int)p[1], w = (int)p[2];
    const size_t ent = (size_t)b * (H + W);
    const int first = bounds[(ent + W) * 2], last = min(h, bounds[(ent + W + H - 1) * 2] + bounds[(ent + W + H - 1) * 2 + 1]);
    const int row = first + r;
    if (row >= last) return;
    const int xmin = bounds[(ent + x) * 2], n = min(bounds[(ent + x) * 2 + 1], w - xmin);
    const int* __restrict__ k = taps + (ent + x) * kmax;
    const unsigned char* __restrict__ s = flat + (size_t)(long long)p[0] + ((size_t)row * w + xmin) * 3;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int t = 0; t < n; ++t) {
        const int kt = k[t];
        a0 += s[t * 3 + 0] * kt;
        a1 += s[t * 3 + 1] * kt;
        a2 += s[t * 3 + 2] * kt;
    }
    unsigned char* __restrict__ o = rows + (size_t)e * 3;
    o[0] = rc_clip8(a0);
    o[1] = rc_clip8(a1);
    o[2] = rc_clip8(a2);
}

// thread = (b, y, x) of the window
__global__ __launch_bounds__(NT_DD) void resize_v_kernel(const double* __restrict__ plan, int B, int H, int W, int kmax, int maxrows,
                                                         const int* __restrict__ taps, const int* __restrict__ bounds,
                                                         const unsigned char* __restrict__ rows, unsigned char* __restrict__ out) {
    const long long e = (long long)blockIdx.x * NT_DD + threadIdx.x;
    if (e >= (long long)B * H * W) return;
    const int x = (int)(e % W), y = (int)((e / W) % H), b = (int)(e / ((long long)W * H));
    const size_t ent = (size_t)b * (H + W);
    const int first = bounds[(ent + W) * 2];
    const int ymin = bounds[(ent + W + y) * 2], n = bounds[(ent + W + y) * 2 + 1];
    const int* __restrict__ k = taps + (ent + W + y) * kmax;
    const unsigned char* __restrict__ s = rows + (size_t)b * maxrows * W * 3 + (size_t)x * 3;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int t = 0; t < n; ++t) {
        const int r = min(max(ymin - first + t, 0), maxrows - 1);
        const unsigned char* __restrict__ q = s + (size_t)r * W * 3;
        const int kt = k[t];
        a0 += q[0] * kt;
        a1 += q[1] * kt;
        a2 += q[2] * kt;
    }
    const bool mirror = plan[(size_t)b * PPF_RC_WORDS + 11] != 0.0;
    unsigned char* __restrict__ o = out + (((size_t)b * H + y) * W + (mirror ? W - 1 - x : x)) * 3;
    o[0] = rc_clip8(a0);
    o[1] = rc_clip8(a1);
    o[2] = rc_clip8(a2);
}

// ------------------------------------------------------------------------------------------------ RandAugment
__device__ __forceinline__ int aug_op(const double* __restrict__ plan, int b, int slot) {
    const double v = plan[((size_t)b * PPF_AUG_SLOTS + slot) * PPF_AUG_WORDS];
    return v >= 0.0 && v <= 14.0 ? (int)v : PPF_AUG_SKIP;
}
__device__ __forceinline__ const double* aug_args(const double* __restrict__ plan, int b, int slot) {
    return plan + ((size_t)b * PPF_AUG_SLOTS + slot) * PPF_AUG_WORDS + 2;
}
__device__ __forceinline__ bool aug_is_affine(int op) { return op == PPF_AUG_ROTATE || (op >= PPF_AUG_SHEAR_X && op <= PPF_AUG_TRANSLATE_Y); }
__device__ __forceinline__ bool aug_is_table(int op) {
    return op == PPF_AUG_AUTOCONTRAST || op == PPF_AUG_EQUALIZE || op == PPF_AUG_INVERT || op == PPF_AUG_POSTERIZE || op == PPF_AUG_SOLARIZE ||
           op == PPF_AUG_SOLARIZE_ADD || op == PPF_AUG_CONTRAST || op == PPF_AUG_BRIGHTNESS;
}
__device__ __forceinline__ int aug_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Image.blend: two fp32 roundings and a truncation; clamped only when alpha leaves [0, 1]
__device__ __forceinline__ unsigned char aug_blend(int a, int b, float alpha) {
    const float t = (float)a + alpha * (float)(b - a);
    if (alpha >= 0.0f && alpha <= 1.0f) return (unsigned char)(int)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (unsigned char)(int)t);
}
__device__ __forceinline__ unsigned char aug_clip_trunc(double v) { return v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (unsigned char)(int)v); }

// grid (blocks per image, B)
__global__ __launch_bounds__(NT_DD) void aug_hist_kernel(const unsigned char* __restrict__ in, const double* __restrict__ plan, int slot, int HW,
                                                         int* __restrict__ hist) {
    __shared__ int h[3 * 256];
    const int b = blockIdx.y, op = aug_op(plan, b, slot);
    if (op != PPF_AUG_AUTOCONTRAST && op != PPF_AUG_EQUALIZE && op != PPF_AUG_CONTRAST) return;      // workgroup-uniform
    for (int i = threadIdx.x; i < 3 * 256; i += NT_DD) h[i] = 0;
    __syncthreads();
    const unsigned char* __restrict__ s = in + (size_t)b * HW * 3;
    for (int p = blockIdx.x * NT_DD + threadIdx.x; p < HW; p += gridDim.x * NT_DD) {
        const int r = s[(size_t)p * 3], g = s[(size_t)p * 3 + 1], bl = s[(size_t)p * 3 + 2];
        if (op == PPF_AUG_CONTRAST) {
            atomicAdd(&h[aug_luma(r, g, bl)], 1);
        } else {
            atomicAdd(&h[r], 1);
            atomicAdd(&h[256 + g], 1);
            atomicAdd(&h[512 + bl], 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * 256; i += NT_DD)
        if (h[i]) atomicAdd(&hist[(size_t)b * 768 + i], h[i]);
}

// one workgroup per sample, lane i = table entry i
__global__ __launch_bounds__(256) void aug_lut_kernel(const int* __restrict__ hist, const double* __restrict__ plan, int slot, int HW,
                                                      unsigned char* __restrict__ lut) {
    __shared__ int h[3 * 256];
    const int b = blockIdx.x, op = aug_op(plan, b, slot), i = threadIdx.x;
    if (!aug_is_table(op)) return;
    const double p0 = aug_args(plan, b, slot)[0];
    unsigned char* __restrict__ o = lut + (size_t)b * 768;
    if (op == PPF_AUG_AUTOCONTRAST || op == PPF_AUG_EQUALIZE || op == PPF_AUG_CONTRAST) {
        for (int c = 0; c < 3; ++c) h[c * 256 + i] = hist[(size_t)b * 768 + c * 256 + i];
        __syncthreads();
    }
    if (op == PPF_AUG_AUTOCONTRAST || op == PPF_AUG_EQUALIZE) {
        for (int c = 0; c < 3; ++c) {
            const int* hc = h + c * 256;
            int lo = 256, hi = -1, nz = 0;
            long long below = 0;
            for (int j = 0; j < 256; ++j) {
                if (hc[j]) {
                    if (lo == 256) lo = j;
                    hi = j;
                    ++nz;
                }
                if (j < i) below += hc[j];
            }
            int v = i;
            if (op == PPF_AUG_AUTOCONTRAST) {
                if (hi > lo) {
                    const double scale = 255.0 / (hi - lo), offset = -lo * scale;
                    const int ix = (int)(i * scale + offset);
                    v = ix < 0 ? 0 : (ix > 255 ? 255 : ix);
                }
            } else if (nz > 1) {
                const long long step = ((long long)HW - hc[hi]) / 255;
                if (step) v = (int)min((step / 2 + below) / step, 255LL);
            }
            o[c * 256 + i] = (unsigned char)v;
        }
        return;
    }
    int v = i;
    if (op == PPF_AUG_INVERT) {
        v = 255 - i;
    } else if (op == PPF_AUG_POSTERIZE) {
        const int bits = min(max((int)p0, 1), 8);
        v = i & ~((1 << (8 - bits)) - 1);
    } else if (op == PPF_AUG_SOLARIZE) {
        v = i < (int)p0 ? i : 255 - i;
    } else if (op == PPF_AUG_SOLARIZE_ADD) {
        v = i < 128 ? min(255, i + (int)p0) : i;
    } else if (op == PPF_AUG_BRIGHTNESS) {
        v = aug_blend(0, i, (float)p0);
    } else {                                                                   // PPF_AUG_CONTRAST
        long long sum = 0;
        for (int j = 0; j < 256; ++j) sum += (long long)j * h[j];
        const int mean = (int)((double)sum / (double)HW + 0.5);
        v = aug_blend(mean, i, (float)p0);
    }
    o[i] = o[256 + i] = o[512 + i] = (unsigned char)v;
}

// thread = pixel; table ops, ColorIncreasing and the copy of a skipped slot
__global__ __launch_bounds__(NT_DD) void aug_apply_kernel(const unsigned char* __restrict__ in, const double* __restrict__ plan, int slot,
                                                          const unsigned char* __restrict__ lut, int B, int HW, unsigned char* __restrict__ out) {
    const long long e = (long long)blockIdx.x * NT_DD + threadIdx.x;
    if (e >= (long long)B * HW) return;
    const int b = (int)(e / HW), op = aug_op(plan, b, slot);
    if (op == PPF_AUG_SHARPNESS || aug_is_affine(op)) return;
    const int r = in[e * 3], g = in[e * 3 + 1], bl = in[e * 3 + 2];
    unsigned char* __restrict__ o = out + e * 3;
    if (aug_is_table(op)) {
        const unsigned char* __restrict__ t = lut + (size_t)b * 768;
        o[0] = t[r];
        o[1] = t[256 + g];
        o[2] = t[512 + bl];
    } else if (op == PPF_AUG_COLOR) {
        const float f = (float)aug_args(plan, b, slot)[0];
        const int l = aug_luma(r, g, bl);
        o[0] = aug_blend(l, r, f);
        o[1] = aug_blend(l, g, f);
        o[2] = aug_blend(l, bl, f);
    } else {
        o[0] = (unsigned char)r;
        o[1] = (unsigned char)g;
        o[2] = (unsigned char)bl;
    }
}

__global__ __launch_bounds__(NT_DD) void aug_sharpness_kernel(const unsigned char* __restrict__ in, const double* __restrict__ plan, int slot, int B,
                                                              int H, int W, unsigned char* __restrict__ out) {
    const long long e = (long long)blockIdx.x * NT_DD + threadIdx.x;
    if (e >= (long long)B * H * W) return;
    const int x = (int)(e % W), y = (int)((e / W) % H), b = (int)(e / ((long long)W * H));
    if (aug_op(plan, b, slot) != PPF_AUG_SHARPNESS) return;
    const float f = (float)aug_args(plan, b, slot)[0];
    const unsigned char* __restrict__ s = in + e * 3;
    const bool border = x == 0 || y == 0 || x == W - 1 || y == H - 1;
    const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
    const long long row = (long long)W * 3;
    for (int c = 0; c < 3; ++c) {
        int sm = s[c];
        if (!border) {
            float t = 0.5f;
            t += ((float)s[row - 3 + c] * k1 + (float)s[row + c] * k1 + (float)s[row + 3 + c] * k1);
            t += ((float)s[-3 + c] * k1 + (float)s[c] * k5 + (float)s[3 + c] * k1);
            t += ((float)s[-row - 3 + c] * k1 + (float)s[-row + c] * k1 + (float)s[-row + 3 + c] * k1);
            sm = t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
        }
        out[e * 3 + c] = aug_blend(sm, s[c], f);
    }
}

__device__ __forceinline__ double aug_cubic(double v1, double v2, double v3, double v4, double d) {
    const double p2 = -v1 + v3;
    const double p3 = 2 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return v2 + d * (p2 + d * (p3 + d * p4));
}

__global__ __launch_bounds__(NT_DD) void aug_affine_kernel(const unsigned char* __restrict__ in, const double* __restrict__ plan, int slot, int B, int H,
                                                           int W, int fr, int fg, int fb, unsigned char* __restrict__ out) {
    const long long e = (long long)blockIdx.x * NT_DD + threadIdx.x;
    if (e >= (long long)B * H * W) return;
    const int xo = (int)(e % W), yo = (int)((e / W) % H), b = (int)(e / ((long long)W * H));
    if (!aug_is_affine(aug_op(plan, b, slot))) return;
    const double* __restrict__ m = aug_args(plan, b, slot);
    const bool cubic = plan[((size_t)b * PPF_AUG_SLOTS + slot) * PPF_AUG_WORDS + 1] == 3.0;
    const double xc = xo + 0.5, yc = yo + 0.5;
    double xin = m[0] * xc + m[1] * yc + m[2], yin = m[3] * xc + m[4] * yc + m[5];
    unsigned char* __restrict__ o = out + e * 3;
    if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) {         // NaN lands here too
        o[0] = (unsigned char)fr;
        o[1] = (unsigned char)fg;
        o[2] = (unsigned char)fb;
        return;
    }
    xin -= 0.5;
    yin -= 0.5;
    const double xf = floor(xin), yf = floor(yin);
    const double dx = xin - xf, dy = yin - yf;
    const int x = (int)xf, y = (int)yf;
    const unsigned char* __restrict__ s = in + (size_t)b * H * W * 3;
    const int nt = cubic ? 4 : 2, base = cubic ? -1 : 0;
    int col[4];
    for (int j = 0; j < nt; ++j) col[j] = min(max(x + base + j, 0), W - 1) * 3;
    for (int c = 0; c < 3; ++c) {
        double v[4];
        for (int j = 0; j < nt; ++j) {
            const int yy = y + base + j;
            if (j > 0 && (yy < 0 || yy >= H)) {
                v[j] = v[j - 1];
                continue;
            }
            const unsigned char* __restrict__ q = s + (size_t)min(max(yy, 0), H - 1) * W * 3 + c;
            if (cubic) v[j] = aug_cubic((double)q[col[0]], (double)q[col[1]], (double)q[col[2]], (double)q[col[3]], dx);
            else v[j] = (double)q[col[0]] + ((double)q[col[1]] - (double)q[col[0]]) * dx;
        }
        o[c] = aug_clip_trunc(cubic ? aug_cubic(v[0], v[1], v[2], v[3], dy) : v[0] + (v[1] - v[0]) * dy);
    }
}

int aug_shape(const char* who, const void* in, const double* plan, int slot, int B, int H, int W, const void* out) {
    PPF_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && H <= RC_MAX_SIDE && W <= RC_MAX_SIDE, PPF_ERR_SHAPE, "%s: bad shape B=%d H=%d W=%d (1 .. %d)", who, B, H, W,
                  RC_MAX_SIDE);
    PPF_CHECK_ARG(slot >= 0 && slot < PPF_AUG_SLOTS, PPF_ERR_ARG, "%s: slot=%d outside [0, %d)", who, slot, PPF_AUG_SLOTS);
    PPF_CHECK_ARG((long long)B * H * W <= (long long)INT_MAX * (NT_DD / 2), PPF_ERR_SHAPE, "%s: B=%d x H=%d x W=%d exceeds the grid", who, B, H, W);
    PPF_CHECK_ARG(in && plan && out, PPF_ERR_ARG, "%s: null pointer", who);
    PPF_CHECK_ARG(in != out, PPF_ERR_ARG, "%s: in place is not supported", who);
    return 0;
}

inline unsigned dd_blocks(long long n) { return (unsigned)((n + NT_DD - 1) / NT_DD); }

}  // namespace

extern "C" {

size_t ppf_resize_crop_workspace_bytes(const double* plan_host, int B, int H, int W, int filter, int64_t flat_bytes) {
    RcLayout L;
    return rc_checked_layout("ppf_resize_crop_workspace_bytes", plan_host, B, H, W, filter, flat_bytes, &L) ? 0 : L.bytes;
}

int ppf_resize_crop_u8(const void* flat_u8, int64_t flat_bytes, const double* plan_host, const double* plan_dev, int B, int H, int W, int filter,
                       void* workspace, size_t workspace_bytes, void* out_u8, hipStream_t stream) {
    RcLayout L;
    if (int rc = rc_checked_layout("ppf_resize_crop_u8", plan_host, B, H, W, filter, flat_bytes, &L)) return rc;
    PPF_CHECK_ARG(flat_u8 && plan_dev && workspace && out_u8, PPF_ERR_ARG, "ppf_resize_crop_u8: null pointer");
    PPF_CHECK_ARG(workspace_bytes >= L.bytes, PPF_ERR_ARG, "ppf_resize_crop_u8: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    PPF_CHECK_ARG(((uintptr_t)workspace & 15) == 0, PPF_ERR_ALIGN, "ppf_resize_crop_u8: workspace must be 16-byte aligned");
    int* taps = (int*)((char*)workspace + L.taps_off);
    int* bounds = (int*)((char*)workspace + L.bounds_off);
    unsigned char* rows = (unsigned char*)workspace + L.rows_off;
    if (int rc = ppf_launch<resize_taps_kernel>(dim3(dd_blocks((long long)B * (H + W))), dim3(NT_DD), 0, stream, "ppf_resize_crop_u8", plan_dev, B, H, W,
                                                filter, L.kmax, taps, bounds))
        return rc;
    if (int rc = ppf_launch<resize_h_kernel>(dim3(dd_blocks((long long)B * L.maxrows * W)), dim3(NT_DD), 0, stream, "ppf_resize_crop_u8",
                                             (const unsigned char*)flat_u8, plan_dev, B, H, W, L.kmax, L.maxrows, (const int*)taps, (const int*)bounds, rows))
        return rc;
    return ppf_launch<resize_v_kernel>(dim3(dd_blocks((long long)B * H * W)), dim3(NT_DD), 0, stream, "ppf_resize_crop_u8", plan_dev, B, H, W, L.kmax,
                                       L.maxrows, (const int*)taps, (const int*)bounds, (const unsigned char*)rows, (unsigned char*)out_u8);
}

int ppf_aug_hist(const void* in_u8, const double* plan_dev, int slot, int B, int H, int W, int* hist, hipStream_t stream) {
    if (int rc = aug_shape("ppf_aug_hist", in_u8, plan_dev, slot, B, H, W, hist)) return rc;
    PPF_CHECK_ARG(B <= 65535, PPF_ERR_SHAPE, "ppf_aug_hist: B=%d exceeds 65535", B);
    hipError_t e = ppf_memset_async(hist, 0, (size_t)B * 768 * sizeof(int), stream);
    PPF_CHECK_ARG(e == hipSuccess, (int)e, "ppf_aug_hist: memset: %s", hipGetErrorString(e));
    const int per_img = (int)std::min(64LL, ((long long)H * W + NT_DD - 1) / NT_DD);
    return ppf_launch<aug_hist_kernel>(dim3((unsigned)per_img, (unsigned)B), dim3(NT_DD), 0, stream, "ppf_aug_hist", (const unsigned char*)in_u8, plan_dev,
                                       slot, H * W, hist);
}

int ppf_aug_lut_build(const int* hist, const double* plan_dev, int slot, int B, int H, int W, void* lut_u8, hipStream_t stream) {
    if (int rc = aug_shape("ppf_aug_lut_build", hist, plan_dev, slot, B, H, W, lut_u8)) return rc;
    return ppf_launch<aug_lut_kernel>(dim3((unsigned)B), dim3(256), 0, stream, "ppf_aug_lut_build", hist, plan_dev, slot, H * W, (unsigned char*)lut_u8);
}

int ppf_aug_apply(const void* in_u8, const double* plan_dev, int slot, const void* lut_u8, int B, int H, int W, void* out_u8, hipStream_t stream) {
    if (int rc = aug_shape("ppf_aug_apply", in_u8, plan_dev, slot, B, H, W, out_u8)) return rc;
    PPF_CHECK_ARG(lut_u8, PPF_ERR_ARG, "ppf_aug_apply: null lut");
    return ppf_launch<aug_apply_kernel>(dim3(dd_blocks((long long)B * H * W)), dim3(NT_DD), 0, stream, "ppf_aug_apply", (const unsigned char*)in_u8, plan_dev,
                                        slot, (const unsigned char*)lut_u8, B, H * W, (unsigned char*)out_u8);
}

int ppf_aug_sharpness(const void* in_u8, const double* plan_dev, int slot, int B, int H, int W, void* out_u8, hipStream_t stream) {
    if (int rc = aug_shape("ppf_aug_sharpness", in_u8, plan_dev, slot, B, H, W, out_u8)) return rc;
    return ppf_launch<aug_sharpness_kernel>(dim3(dd_blocks((long long)B * H * W)), dim3(NT_DD), 0, stream, "ppf_aug_sharpness", (const unsigned char*)in_u8,
                                            plan_dev, slot, B, H, W, (unsigned char*)out_u8);
}

int ppf_aug_affine(const void* in_u8, const double* plan_dev, int slot, int B, int H, int W, int fill_r, int fill_g, int fill_b, void* out_u8,
                   hipStream_t stream) {
    if (int rc = aug_shape("ppf_aug_affine", in_u8, plan_dev, slot, B, H, W, out_u8)) return rc;
    PPF_CHECK_ARG(((fill_r | fill_g | fill_b) & ~255) == 0, PPF_ERR_ARG, "ppf_aug_affine: fill (%d, %d, %d) outside [0, 255]", fill_r, fill_g, fill_b);
    return ppf_launch<aug_affine_kernel>(dim3(dd_blocks((long long)B * H * W)), dim3(NT_DD), 0, stream, "ppf_aug_affine", (const unsigned char*)in_u8,
                                         plan_dev, slot, B, H, W, fill_r, fill_g, fill_b, (unsigned char*)out_u8);
}

}  // extern "C"
