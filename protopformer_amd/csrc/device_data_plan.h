// The host's share of ppf_resize_crop_u8 and the tap arithmetic its kernel shares with it, in plain C++ so that
// tests/device_data_plan_check.cpp can build them with the host compiler under AddressSanitizer + UBSan: the validation of the plan table
// (nothing is launched for a plan that would read outside the frames), the layout of the workspace, and Pillow's 8-bit resample taps of one
// output coordinate.  The contract is in include/ppf_hip.h.  Every floating-point expression is in the order Pillow's C evaluates it and
// must round after every operation: the including file switches contraction off.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "ppf_hip.h"

#if defined(__HIPCC__)
#define RC_HD __host__ __device__
#else
#define RC_HD
#endif

constexpr int NT_DD = 256;
constexpr int RC_MAX_SIDE = 16384;
constexpr int RC_MAX_TAPS = 1024;

struct RcLayout {                // workspace: taps int32 [B][H + W][kmax], bounds int32 [B][H + W][2], rows uint8 [B][maxrows][W][3]
    int kmax, maxrows;
    size_t taps_off, bounds_off, rows_off, bytes;
};

RC_HD inline double rc_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

RC_HD inline double rc_weight(int filter, double x) {
    if (filter == 3) return rc_bicubic(x);
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

// The taps of output coordinate xx of an axis of `size` source samples, box [in0, in1) resampled to `out`: the first tap *xmin, their
// count *n (1 .. kmax, inside the axis) and the integer weights k[0 .. *n).
RC_HD inline void rc_taps(int filter, int size, double in0, double in1, int out, int xx, int kmax, int* k, int* xmin_out, int* n_out) {
    const double scale = (in1 - in0) / out;
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = (filter == 3 ? 2.0 : 1.0) * filterscale, ss = 1.0 / filterscale;
    const double center = in0 + (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > size) xmax = size;
    if (xmin > size - 1) xmin = size - 1;               // never taken for a validated plan: keeps every later index inside the frame
    int n = xmax - xmin;
    n = n < 1 ? 1 : (n > kmax ? kmax : n);
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww += rc_weight(filter, (x + xmin - center + 0.5) * ss);
    for (int x = 0; x < n; ++x) {
        double w = rc_weight(filter, (x + xmin - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        k[x] = w < 0 ? (int)(-0.5 + w * 4194304.0) : (int)(0.5 + w * 4194304.0);
    }
    *xmin_out = xmin;
    *n_out = n;
}

inline bool rc_whole(double v) { return v == floor(v); }

inline int rc_fail(char* err, size_t err_len, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, err_len, fmt, ap);
    va_end(ap);
    return code;
}

#define RC_CHECK(cond, code, ...) \
    do {                          \
        if (!(cond)) return rc_fail(err, err_len, (code), __VA_ARGS__); \
    } while (0)

// Validates the host plan and sizes the workspace.  0, or PPF_ERR_* with the message in err.
inline int rc_layout(const char* who, const double* plan, int B, int H, int W, int filter, int64_t flat_bytes, RcLayout* L, char* err, size_t err_len) {
    RC_CHECK(plan, PPF_ERR_ARG, "%s: null plan_host", who);
    RC_CHECK(B >= 1 && H >= 1 && W >= 1 && H <= RC_MAX_SIDE && W <= RC_MAX_SIDE, PPF_ERR_SHAPE, "%s: bad shape B=%d H=%d W=%d (1 .. %d)", who, B, H, W,
             RC_MAX_SIDE);
    RC_CHECK(filter == 2 || filter == 3, PPF_ERR_ARG, "%s: filter=%d (2 BILINEAR, 3 BICUBIC)", who, filter);
    const double fs = filter == 3 ? 2.0 : 1.0;                                 // the filter's support
    RC_CHECK(flat_bytes >= 3, PPF_ERR_SHAPE, "%s: flat_bytes=%lld", who, (long long)flat_bytes);
    int kmax = 1, maxrows = 1;
    for (int b = 0; b < B; ++b) {
        const double* p = plan + (size_t)b * PPF_RC_WORDS;
        for (int i = 0; i < PPF_RC_WORDS; ++i) RC_CHECK(isfinite(p[i]), PPF_ERR_ARG, "%s: sample %d: plan word %d is not finite", who, b, i);
        const double off = p[0], h = p[1], w = p[2], oh = p[7], ow = p[8], y0 = p[9], x0 = p[10];
        RC_CHECK(rc_whole(off) && rc_whole(h) && rc_whole(w) && h >= 1 && w >= 1 && h <= RC_MAX_SIDE && w <= RC_MAX_SIDE && off >= 0 &&
                     off + h * w * 3 <= (double)flat_bytes,
                 PPF_ERR_ARG, "%s: sample %d: frame offset=%.0f h=%.0f w=%.0f leaves the %lld bytes of frames", who, b, off, h, w, (long long)flat_bytes);
        RC_CHECK(p[3] >= 0 && p[4] >= 0 && p[5] <= w && p[6] <= h && p[3] < p[5] && p[4] < p[6], PPF_ERR_ARG,
                 "%s: sample %d: box (%g, %g, %g, %g) is empty or leaves the %.0f x %.0f frame", who, b, p[3], p[4], p[5], p[6], w, h);
        RC_CHECK(rc_whole(oh) && rc_whole(ow) && oh >= 1 && ow >= 1 && oh <= RC_MAX_SIDE && ow <= RC_MAX_SIDE, PPF_ERR_ARG,
                 "%s: sample %d: output size (%g, %g) outside [1, %d]", who, b, oh, ow, RC_MAX_SIDE);
        RC_CHECK(rc_whole(y0) && rc_whole(x0) && y0 >= 0 && x0 >= 0 && y0 + H <= oh && x0 + W <= ow, PPF_ERR_ARG,
                 "%s: sample %d: window (%g, %g, %d, %d) leaves the output size (%.0f, %.0f)", who, b, y0, x0, H, W, oh, ow);
        RC_CHECK(p[11] == 0.0 || p[11] == 1.0, PPF_ERR_ARG, "%s: sample %d: mirror flag %g", who, b, p[11]);
        const double sx = (p[5] - p[3]) / ow, sy = (p[6] - p[4]) / oh;
        const double fx = sx < 1.0 ? 1.0 : sx, fy = sy < 1.0 ? 1.0 : sy;
        const double kx = ceil(fs * fx) * 2 + 1, ky = ceil(fs * fy) * 2 + 1;
        RC_CHECK(kx <= RC_MAX_TAPS && ky <= RC_MAX_TAPS, PPF_ERR_SHAPE, "%s: sample %d: %.0f x %.0f taps exceed %d", who, b, kx, ky, RC_MAX_TAPS);
        const int kb = (int)(kx > ky ? kx : ky);
        if (kb > kmax) kmax = kb;
        // source rows under the window: the centres span sy * (H - 1), the taps reach support + 0.5 to either side
        const double rows = ceil(sy * H + 2.0 * fs * fy) + 3;
        const int rb = (int)(rows < h ? rows : h);
        if (rb > maxrows) maxrows = rb;
    }
    L->kmax = kmax;
    L->maxrows = maxrows;
    const size_t n = (size_t)B * (H + W);
    L->taps_off = 0;
    L->bounds_off = (n * kmax * sizeof(int) + 15) & ~(size_t)15;
    L->rows_off = (L->bounds_off + n * 2 * sizeof(int) + 15) & ~(size_t)15;
    L->bytes = L->rows_off + (((size_t)B * maxrows * W * 3 + 15) & ~(size_t)15);
    RC_CHECK((long long)B * maxrows * W <= (long long)INT_MAX * (NT_DD / 2) && (long long)B * H * W <= (long long)INT_MAX * (NT_DD / 2), PPF_ERR_SHAPE,
             "%s: B=%d x %d rows x W=%d exceeds the grid", who, B, maxrows, W);
    return 0;
}
