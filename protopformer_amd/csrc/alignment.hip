// Spatial alignment of prototypes (Sacha et al., "Interpretability Benchmark for Evaluating Spatial Misalignment of Prototypical Parts
// Explanations", AAAI 2024): does a prototype's activation at a grid cell depend on the pixels of that cell?  Perturb only the pixels
// outside the prototype's box, follow its activation and its peak, and report the share of the pixel gradient that falls inside the box.
// The model's forward and backward between the launches are the caller's (interpret.input_gradient / misalignment_attack).  The reference
// has no such pass.  Three streaming launches:
//   * col2im_kernel: the inverse of im2col_kernel / im2col_f32_kernel -- the last step of the image gradient, behind
//     dcols = dtok . W_patch_embed.  A thread owns one 16-byte vector of the image (a patch row never straddles it: p % 4 == 0, else the
//     scalar form); patch stride == patch size, so every image element is written exactly once: no atomics, no zero fill.
//   * grad_box_mass_kernel: one workgroup of NT_MASS threads per row.  Thread t adds |g| of the 16-byte vectors t, t + NT, ... (single
//     elements when W % 4 != 0) in fp64 (every term exact), the wave sums meet by butterfly shuffles and the NT / 64 wave totals are
//     added in wave order by one thread: a fixed order, bit-identical from run to run.  Non-finite elements count as 0 in both sums and
//     are counted separately.
//   * pgd_step_box_kernel: the signed-gradient step of the misalignment attack, projected onto the eps-ball around x0 and the valid pixel
//     range, outside the box; inside the box the original pixel comes back.  alpha * sign(g) is exact, so x + step has ONE rounding whether
//     or not the compiler fuses it: bit-exact to the numpy referee (interpret.pgd_step_box, device=False).
// Deterministic: no atomics.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "ppf_common.h"
#include "ppf_hip.h"

namespace {

constexpr int NT_STREAM = 256;
constexpr int NT_MASS = 512;

// cols fp32 [B*gh*gw][C*p*p], column order (c, py, px) -> img [B][C][H][W].  VEC elements of one image row per thread (VEC divides p).
template <int VEC>
__global__ __launch_bounds__(NT_STREAM) void col2im_kernel(const float* __restrict__ cols, float* __restrict__ img, int C, int H, int W, int p,
                                                           long long nvec) {
    const long long v = (long long)blockIdx.x * NT_STREAM + threadIdx.x;
    if (v >= nvec) return;
    const int Wv = W / VEC, gh = H / p, gw = W / p;
    long long t = v;
    const int x = (int)(t % Wv) * VEC; t /= Wv;
    const int y = (int)(t % H); t /= H;
    const int c = (int)(t % C); t /= C;
    const long long b = t;
    const int gy = y / p, py = y - gy * p, gx = x / p, px = x - gx * p;
    const float* __restrict__ src = cols + (((size_t)b * gh + gy) * gw + gx) * ((size_t)C * p * p) + ((size_t)c * p + py) * p + px;
    if (VEC == 4) reinterpret_cast<float4*>(img)[v] = *reinterpret_cast<const float4*>(src);
    else img[v] = *src;
}

__device__ __forceinline__ bool in_box(const int4 bx, int y, int x) { return y >= bx.x && y < bx.y && x >= bx.z && x < bx.w; }

// grid: R workgroups of NT_MASS threads.  g [R][C][H][W], box [R] as (y0, y1, x0, x1), half-open.  VEC elements of one image row per load.
template <int VEC>
__global__ __launch_bounds__(NT_MASS) void grad_box_mass_kernel(const float* __restrict__ g, const int4* __restrict__ box, int n, int H, int W,
                                                               double* __restrict__ inside, double* __restrict__ total,
                                                               int* __restrict__ nonfinite) {
    __shared__ double s_in[NT_MASS / 64], s_tot[NT_MASS / 64];
    __shared__ int s_bad[NT_MASS / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int4 bx = box[r];
    const float* __restrict__ row = g + (size_t)r * n;
    const int nv = n / VEC, Wv = W / VEC;
    double acc_in = 0.0, acc_tot = 0.0;
    int bad = 0;
#pragma unroll 4
    for (int i = tid; i < nv; i += NT_MASS) {
        float v[VEC];
        if constexpr (VEC == 4) {
            const float4 q = reinterpret_cast<const float4*>(row)[i];
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = row[i];
        }
        const int x0 = (i % Wv) * VEC, y = (i / Wv) % H;
        const bool row_in = y >= bx.x && y < bx.y;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float a = fabsf(v[k]);
            if (a <= FLT_MAX) {                                                // false for inf and NaN
                acc_tot += (double)a;
                if (row_in && x0 + k >= bx.z && x0 + k < bx.w) acc_in += (double)a;
            } else {
                ++bad;
            }
        }
    }
    acc_in = wave_sum_f64(acc_in);
    acc_tot = wave_sum_f64(acc_tot);
    bad = wave_sum_i32(bad);
    if ((tid & 63) == 0) { s_in[tid >> 6] = acc_in; s_tot[tid >> 6] = acc_tot; s_bad[tid >> 6] = bad; }
    __syncthreads();
    if (tid == 0) {
        double a = s_in[0], b = s_tot[0];
        int c = s_bad[0];
        for (int w = 1; w < NT_MASS / 64; ++w) { a += s_in[w]; b += s_tot[w]; c += s_bad[w]; }      // fixed order
        inside[r] = a;
        total[r] = b;
        if (nonfinite) nonfinite[r] = c;
    }
}

__device__ __forceinline__ float pgd_one(float x, float x0, float g, float step, float eps, float lo, float hi, bool inside) {
    if (inside) return x0;
    const float s = (float)(g > 0.0f) - (float)(g < 0.0f);                     // sign(+-0) = sign(NaN) = 0
    const float moved = __fadd_rn(x, step * s);                                // step * s is exact: one rounding
    const float lower = fmaxf(__fsub_rn(x0, eps), lo), upper = fminf(__fadd_rn(x0, eps), hi);
    return fminf(fmaxf(moved, lower), upper);
}

// VEC elements of one image row per thread.  grid: ceil(R * C * H * (W / VEC) / NT_STREAM)
template <int VEC>
__global__ __launch_bounds__(NT_STREAM) void pgd_step_box_kernel(float* __restrict__ x, const float* __restrict__ x0, const float* __restrict__ g,
                                                                 const int4* __restrict__ box, const float* __restrict__ alpha,
                                                                 const float* __restrict__ eps, const float* __restrict__ lo,
                                                                 const float* __restrict__ hi, float dir, int C, int H, int W, long long nvec) {
    const long long v = (long long)blockIdx.x * NT_STREAM + threadIdx.x;
    if (v >= nvec) return;
    const int Wv = W / VEC;
    long long t = v;
    const int xc = (int)(t % Wv) * VEC; t /= Wv;
    const int y = (int)(t % H); t /= H;
    const int c = (int)(t % C); t /= C;
    const int4 bx = box[t];
    const float step = dir * alpha[c], e = eps[c], l = lo[c], h = hi[c];       // dir = +-1: exact
    if (VEC == 4) {
        const float4 xv = reinterpret_cast<const float4*>(x)[v], ov = reinterpret_cast<const float4*>(x0)[v], gv = reinterpret_cast<const float4*>(g)[v];
        reinterpret_cast<float4*>(x)[v] = make_float4(pgd_one(xv.x, ov.x, gv.x, step, e, l, h, in_box(bx, y, xc)),
                                                      pgd_one(xv.y, ov.y, gv.y, step, e, l, h, in_box(bx, y, xc + 1)),
                                                      pgd_one(xv.z, ov.z, gv.z, step, e, l, h, in_box(bx, y, xc + 2)),
                                                      pgd_one(xv.w, ov.w, gv.w, step, e, l, h, in_box(bx, y, xc + 3)));
    } else {
        x[v] = pgd_one(x[v], x0[v], g[v], step, e, l, h, in_box(bx, y, xc));
    }
}

bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

}  // namespace

extern "C" {

int ppf_col2im_patch_f32(const float* cols, float* img, int B, int C, int H, int W, int patch, hipStream_t stream) {
    PPF_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && patch > 0, PPF_ERR_SHAPE, "ppf_col2im_patch_f32: bad shape B=%d C=%d H=%d W=%d patch=%d (all >= 1)",
                  B, C, H, W, patch);
    PPF_CHECK_ARG(H % patch == 0 && W % patch == 0, PPF_ERR_SHAPE, "ppf_col2im_patch_f32: patch=%d does not divide H=%d and W=%d", patch, H, W);
    PPF_CHECK_ARG(cols && img, PPF_ERR_ARG, "ppf_col2im_patch_f32: null pointer (cols, img)");
    const bool vec = patch % 4 == 0 && aligned16(cols, img);
    const long long nvec = (long long)B * C * H * W / (vec ? 4 : 1), blocks = (nvec + NT_STREAM - 1) / NT_STREAM;
    PPF_CHECK_ARG(blocks <= INT_MAX, PPF_ERR_SHAPE, "ppf_col2im_patch_f32: B=%d x C=%d x H=%d x W=%d exceeds the grid", B, C, H, W);
    if (vec)
        return ppf_launch<col2im_kernel<4>>(dim3((unsigned)blocks), dim3(NT_STREAM), 0, stream, "ppf_col2im_patch_f32", cols, img, C, H, W, patch, nvec);
    return ppf_launch<col2im_kernel<1>>(dim3((unsigned)blocks), dim3(NT_STREAM), 0, stream, "ppf_col2im_patch_f32", cols, img, C, H, W, patch, nvec);
}

int ppf_grad_box_mass(const float* g, const int* box, int R, int C, int H, int W, double* inside, double* total, int* nonfinite,
                      hipStream_t stream) {
    PPF_CHECK_ARG(R >= 1 && C >= 1 && H >= 1 && W >= 1, PPF_ERR_SHAPE, "ppf_grad_box_mass: bad shape R=%d C=%d H=%d W=%d (all >= 1)", R, C, H, W);
    PPF_CHECK_ARG((long long)C * H * W <= INT_MAX, PPF_ERR_SHAPE, "ppf_grad_box_mass: C=%d x H=%d x W=%d elements per row exceed 2^31 - 1", C, H, W);
    PPF_CHECK_ARG(g && box && inside && total, PPF_ERR_ARG, "ppf_grad_box_mass: null pointer (g, box, inside, total; only nonfinite may be NULL)");
    PPF_CHECK_ARG(aligned16(box), PPF_ERR_ALIGN, "ppf_grad_box_mass: box must be 16-byte aligned");
    if (W % 4 == 0 && aligned16(g))                                           // rows start 16-byte aligned: C * H * W is a multiple of 4
        return ppf_launch<grad_box_mass_kernel<4>>(dim3((unsigned)R), dim3(NT_MASS), 0, stream, "ppf_grad_box_mass", g, (const int4*)box, C * H * W, H, W,
                                                   inside, total, nonfinite);
    return ppf_launch<grad_box_mass_kernel<1>>(dim3((unsigned)R), dim3(NT_MASS), 0, stream, "ppf_grad_box_mass", g, (const int4*)box, C * H * W, H, W,
                                               inside, total, nonfinite);
}

int ppf_pgd_step_box(float* x, const float* x0, const float* g, const int* box, const float* alpha3, const float* eps3, const float* lo3,
                     const float* hi3, float dir, int R, int C, int H, int W, hipStream_t stream) {
    PPF_CHECK_ARG(R >= 1 && C >= 1 && H >= 1 && W >= 1, PPF_ERR_SHAPE, "ppf_pgd_step_box: bad shape R=%d C=%d H=%d W=%d (all >= 1)", R, C, H, W);
    PPF_CHECK_ARG(dir == 1.0f || dir == -1.0f, PPF_ERR_ARG, "ppf_pgd_step_box: dir=%g must be +1 (ascend) or -1 (descend)", (double)dir);
    PPF_CHECK_ARG(x && x0 && g && box && alpha3 && eps3 && lo3 && hi3, PPF_ERR_ARG,
                  "ppf_pgd_step_box: null pointer (x, x0, g, box, alpha3, eps3, lo3, hi3)");
    PPF_CHECK_ARG(aligned16(box), PPF_ERR_ALIGN, "ppf_pgd_step_box: box must be 16-byte aligned");
    const bool vec = W % 4 == 0 && aligned16(x, x0, g);
    const long long nvec = (long long)R * C * H * W / (vec ? 4 : 1), blocks = (nvec + NT_STREAM - 1) / NT_STREAM;
    PPF_CHECK_ARG(blocks <= INT_MAX, PPF_ERR_SHAPE, "ppf_pgd_step_box: R=%d x C=%d x H=%d x W=%d exceeds the grid", R, C, H, W);
    if (vec)
        return ppf_launch<pgd_step_box_kernel<4>>(dim3((unsigned)blocks), dim3(NT_STREAM), 0, stream, "ppf_pgd_step_box", x, x0, g, (const int4*)box, alpha3,
                                                  eps3, lo3, hi3, dir, C, H, W, nvec);
    return ppf_launch<pgd_step_box_kernel<1>>(dim3((unsigned)blocks), dim3(NT_STREAM), 0, stream, "ppf_pgd_step_box", x, x0, g, (const int4*)box, alpha3,
                                              eps3, lo3, hi3, dir, C, H, W, nvec);
}

}  // extern "C"
