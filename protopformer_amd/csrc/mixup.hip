// Mixup / CutMix on the device batch (timm 0.5.4 data/mixup.py, applied in train_one_epoch: tools/engine_proto.py:47-48):
//   * mixup_apply_kernel: in-place mixing of sample i with sample j = B-1-i AS IT WAS BEFORE THE CALL (timm's x.flip(0) / x_orig).
//     One thread owns the same pixel of both samples of a pair: it loads x_i[q] and x_j[q] and then writes both outputs, so the
//     in-place update needs neither a clone nor any ordering between threads.  Blends are fl(fl(x_i*w_self) + fl(x_j*w_other)) with
//     no FMA contraction (__fmul_rn / __fadd_rn): bit-exact to timm's torch arithmetic given the weights rounded as timm rounds them.
//   * mixup_target_kernel: timm's mixup_target, t[b] = w_self*onehot_smooth(label_b) + w_other*onehot_smooth(label_{B-1-b}), same
//     unfused arithmetic.
// The per-sample parameters are one small host table per call (PPF_MIX_WORDS int32 words per sample, layout in include/ppf_hip.h),
// validated on the host and uploaded with one H2D copy on the launch stream.
#include "ppf_common.h"
#include "ppf_hip.h"

namespace {

struct MixRow {
    int kind, yl, yh, xl, xh;
    float ws, wo;
};

__device__ __forceinline__ MixRow load_row(const int* t, int b) {
    const int* r = t + (size_t)b * PPF_MIX_WORDS;
    MixRow m;
    m.kind = r[PPF_MIX_KIND]; m.yl = r[PPF_MIX_YL]; m.yh = r[PPF_MIX_YH]; m.xl = r[PPF_MIX_XL]; m.xh = r[PPF_MIX_XH];
    m.ws = __int_as_float(r[PPF_MIX_WSELF]); m.wo = __int_as_float(r[PPF_MIX_WOTHER]);
    return m;
}

// new value of one element of a sample with parameters m at column xc of row y: s = its own value, o = the partner's pre-call value
__device__ __forceinline__ float mix_one(const MixRow& m, bool row_in, int xc, float s, float o) {
    if (m.kind == 1) return __fadd_rn(__fmul_rn(s, m.ws), __fmul_rn(o, m.wo));
    if (m.kind == 2 && row_in && xc >= m.xl && xc < m.xh) return o;
    return s;
}

// Does sample m change anything in the VW consecutive elements starting at column x0 of row y?
template <int VW>
__device__ __forceinline__ bool touches(const MixRow& m, int y, int x0) {
    if (m.kind == 1) return true;
    return m.kind == 2 && y >= m.yl && y < m.yh && x0 < m.xh && x0 + VW > m.xl;
}

// grid: x = units of one sample (VW consecutive floats along W), y = pair index i < ceil(B/2); 256 threads.
// VW == 4 needs W % 4 == 0 and a 16-byte aligned batch (a unit never straddles a row); VW == 1 serves every other shape.
template <int VW>
__global__ __launch_bounds__(256) void mixup_apply_kernel(float* __restrict__ x, const int* __restrict__ table, int B, int H, int W,
                                                          int units) {
    const int i = blockIdx.y, j = B - 1 - i;
    const MixRow ri = load_row(table, i), rj = load_row(table, j);
    if (ri.kind == 0 && rj.kind == 0) return;
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    const int e = u * VW;                                 // element index inside one sample ([Cc][H][W])
    const int x0 = e % W, y = (e / W) % H;
    const bool ti = touches<VW>(ri, y, x0), tj = j != i && touches<VW>(rj, y, x0);
    if (!ti && !tj) return;
    const size_t n = (size_t)units * VW;
    float* pi = x + (size_t)i * n + e;
    float* pj = x + (size_t)j * n + e;
    const bool yi = y >= ri.yl && y < ri.yh, yj = y >= rj.yl && y < rj.yh;
    if constexpr (VW == 4) {
        const float4 a = *reinterpret_cast<const float4*>(pi);
        const float4 b = *reinterpret_cast<const float4*>(pj);
        if (ti) {
            float4 o;
            o.x = mix_one(ri, yi, x0, a.x, b.x); o.y = mix_one(ri, yi, x0 + 1, a.y, b.y);
            o.z = mix_one(ri, yi, x0 + 2, a.z, b.z); o.w = mix_one(ri, yi, x0 + 3, a.w, b.w);
            *reinterpret_cast<float4*>(pi) = o;
        }
        if (tj) {
            float4 o;
            o.x = mix_one(rj, yj, x0, b.x, a.x); o.y = mix_one(rj, yj, x0 + 1, b.y, a.y);
            o.z = mix_one(rj, yj, x0 + 2, b.z, a.z); o.w = mix_one(rj, yj, x0 + 3, b.w, a.w);
            *reinterpret_cast<float4*>(pj) = o;
        }
    } else {
        const float a = *pi, b = *pj;
        if (ti) *pi = mix_one(ri, yi, x0, a, b);
        if (tj) *pj = mix_one(rj, yj, x0, b, a);
    }
}

// grid: x = ceil(C/256), y = B
__global__ __launch_bounds__(256) void mixup_target_kernel(const long long* __restrict__ label, const float* __restrict__ lam, int lam_stride,
                                                           float off, float on, float* __restrict__ t, int B, int C) {
    const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const long long l1 = label[b], l2 = label[B - 1 - b];
    const float ws = lam[(size_t)b * lam_stride], wo = lam[(size_t)b * lam_stride + 1];
    const float y1 = c == l1 ? on : off, y2 = c == l2 ? on : off;
    t[(size_t)b * C + c] = __fadd_rn(__fmul_rn(y1, ws), __fmul_rn(y2, wo));
}

}  // namespace

extern "C" {

int ppf_mixup_apply(float* x, const int* table_host, int* table_dev, int B, int Cc, int H, int W, hipStream_t stream) {
    PPF_CHECK_ARG(x && table_host && table_dev, PPF_ERR_ARG, "ppf_mixup_apply: null pointer");
    PPF_CHECK_ARG(B > 0 && Cc > 0 && H > 0 && W > 0, PPF_ERR_SHAPE, "ppf_mixup_apply: bad shape B=%d C=%d H=%d W=%d", B, Cc, H, W);
    PPF_CHECK_ARG((int64_t)Cc * H * W < ((int64_t)1 << 31), PPF_ERR_SHAPE, "ppf_mixup_apply: a sample of %d x %d x %d elements is too large", Cc, H, W);
    bool any = false;
    for (int b = 0; b < B; ++b) {
        const int* r = table_host + (size_t)b * PPF_MIX_WORDS;
        const int kind = r[PPF_MIX_KIND];
        PPF_CHECK_ARG(kind >= 0 && kind <= 2, PPF_ERR_ARG, "ppf_mixup_apply: sample %d has kind %d (0 untouched, 1 blend, 2 box)", b, kind);
        if (kind == 2)
            PPF_CHECK_ARG(r[PPF_MIX_YL] >= 0 && r[PPF_MIX_YL] <= r[PPF_MIX_YH] && r[PPF_MIX_YH] <= H && r[PPF_MIX_XL] >= 0 &&
                              r[PPF_MIX_XL] <= r[PPF_MIX_XH] && r[PPF_MIX_XH] <= W,
                          PPF_ERR_ARG, "ppf_mixup_apply: sample %d box y[%d,%d) x[%d,%d) is not inside the %d x %d image", b, r[PPF_MIX_YL],
                          r[PPF_MIX_YH], r[PPF_MIX_XL], r[PPF_MIX_XH], H, W);
        any = any || kind != 0;
    }
    const hipError_t e = ppf_memcpy_async(table_dev, table_host, (size_t)B * PPF_MIX_WORDS * sizeof(int), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) {
        ppf_set_error("ppf_mixup_apply: parameter upload failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    if (!any) return 0;                                   // nothing to mix: the batch is not touched at all
    const int n = Cc * H * W;
    const bool vec = W % 4 == 0 && ((uintptr_t)x & 15) == 0;
    const int units = vec ? n / 4 : n;
    const dim3 grid((units + 255) / 256, (B + 1) / 2);
    if (vec) return ppf_launch<mixup_apply_kernel<4>>(grid, dim3(256), 0, stream, "ppf_mixup_apply", x, (const int*)table_dev, B, H, W, units);
    return ppf_launch<mixup_apply_kernel<1>>(grid, dim3(256), 0, stream, "ppf_mixup_apply", x, (const int*)table_dev, B, H, W, units);
}

int ppf_mixup_target(const void* label, const float* lam, int lam_stride, float off_value, float on_value, float* target, int B, int C,
                     hipStream_t stream) {
    PPF_CHECK_ARG(label && lam && target, PPF_ERR_ARG, "ppf_mixup_target: null pointer");
    PPF_CHECK_ARG(B > 0 && C > 0 && lam_stride >= 0, PPF_ERR_SHAPE, "ppf_mixup_target: bad shape B=%d C=%d lam_stride=%d", B, C, lam_stride);
    return ppf_launch<mixup_target_kernel>(dim3((C + 255) / 256, B), dim3(256), 0, stream, "ppf_mixup_target", (const long long*)label, lam, lam_stride, off_value,
                                           on_value, target, B, C);
}

}  // extern "C"
