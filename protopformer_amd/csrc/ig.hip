// Integrated gradients (Sundararajan et al., "Axiomatic Attribution for Deep Networks", 2017): the attribution of an image is
// (x - baseline) times the gradient averaged along the straight path from the baseline to x, and the attributions sum to
// f(x) - f(baseline).  The forwards and backwards along the path are the caller's (interpret.input_gradient); what lies between them
// stays on the device and is written here.  The reference has no such pass.  Three streaming launches, each a written contract
// (include/ppf_hip.h) that the numpy referees (interpret.ig_point / ig_accumulate / ig_finish, device=False) keep bit for bit:
//   * ig_point_kernel: the path point base + alpha * (x - base).  One thread per 16-byte vector (single elements when the size or a
//     pointer does not allow it).
//   * ig_accumulate_kernel: acc (+)= w * g over R rows, the accumulator's rows `acc_stride` apart so that one class column of a
//     [B][M][...] accumulator is the target; with `first` the accumulator is written, not read: no zero fill.
//   * ig_finish_kernel: attr = (x - base) * acc and the fp64 sum of attr over every cell of the patch grid, in ONE pass: a workgroup owns
//     a run of cells of one grid row of one (sample, class) plane stack; a thread keeps one 16-byte column position (so one cell) and
//     walks the C * patch image rows of the band, writes the attribution from the registers it adds to its fp64 partial, and the
//     partials of a cell meet in LDS, added by one thread in ascending thread order: a fixed order, bit-identical from run to run, no
//     atomics.  A NaN stays in its own cell: the partials of different cells never meet.
// Every operation is rounded once, as numpy's: fsub_rn / fmul_rn / fadd_rn below are plain operators under the pragma.  The HIP headers'
// intrinsics of those names are inline functions compiled under the default contraction mode, and a multiply and an add that come from
// them were fused into an fma after inlining (seen in this file's ig_point_kernel, and in rise.hip before).
#include <limits.h>
#include <stdint.h>

#include "ppf_common.h"
#include "ppf_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT_STREAM = 256;
constexpr int NT_FINISH = 256;

__device__ __forceinline__ float fsub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float fmul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float fadd_rn(float a, float b) { return a + b; }

__device__ __forceinline__ float point_one(float x, float b, float alpha) { return fadd_rn(b, fmul_rn(alpha, fsub_rn(x, b))); }

// grid: ceil(nvec / NT_STREAM); nvec vectors of VEC elements.  base: the tensor, or NULL for the constant.
template <int VEC>
__global__ __launch_bounds__(NT_STREAM) void ig_point_kernel(const float* __restrict__ x, const float* __restrict__ base, float base_const, float alpha,
                                                             long long nvec, float* __restrict__ out) {
    const long long v = (long long)blockIdx.x * NT_STREAM + threadIdx.x;
    if (v >= nvec) return;
    if constexpr (VEC == 4) {
        const float4 xv = reinterpret_cast<const float4*>(x)[v];
        const float4 bv = base ? reinterpret_cast<const float4*>(base)[v] : make_float4(base_const, base_const, base_const, base_const);
        reinterpret_cast<float4*>(out)[v] = make_float4(point_one(xv.x, bv.x, alpha), point_one(xv.y, bv.y, alpha), point_one(xv.z, bv.z, alpha),
                                                        point_one(xv.w, bv.w, alpha));
    } else {
        out[v] = point_one(x[v], base ? base[v] : base_const, alpha);
    }
}

// grid: ceil(R * nv / NT_STREAM); nv vectors per row of g, the accumulator's rows stride_v vectors apart.
template <int VEC>
__global__ __launch_bounds__(NT_STREAM) void ig_accumulate_kernel(const float* __restrict__ g, float w, int first, long long nv, long long total,
                                                                  float* __restrict__ acc, long long stride_v) {
    const long long v = (long long)blockIdx.x * NT_STREAM + threadIdx.x;
    if (v >= total) return;
    const long long r = v / nv, a = r * stride_v + (v - r * nv);
    if constexpr (VEC == 4) {
        const float4 gv = reinterpret_cast<const float4*>(g)[v];
        float4 o = make_float4(fmul_rn(w, gv.x), fmul_rn(w, gv.y), fmul_rn(w, gv.z), fmul_rn(w, gv.w));
        if (!first) {                                                             // uniform over the launch
            const float4 av = reinterpret_cast<const float4*>(acc)[a];
            o = make_float4(fadd_rn(av.x, o.x), fadd_rn(av.y, o.y), fadd_rn(av.z, o.z), fadd_rn(av.w, o.w));
        }
        reinterpret_cast<float4*>(acc)[a] = o;
    } else {
        const float o = fmul_rn(w, g[v]);
        acc[a] = first ? o : fadd_rn(acc[a], o);
    }
}

// grid: B * M * gh * chunks workgroups of NT_FINISH threads; workgroup -> (plane stack bm, grid row gy, chunk of cw cells).  pv = patch / VEC
// vectors per cell row.  A chunk's ncol = cells * pv column positions: with ncol <= NT_FINISH a thread keeps column t % ncol and the
// threads share the band's rows NT_FINISH / ncol at a time; a single cell wider than the workgroup (cw == 1) is walked column by column.
template <int VEC>
__global__ __launch_bounds__(NT_FINISH) void ig_finish_kernel(const float* __restrict__ acc, const float* __restrict__ x, const float* __restrict__ base,
                                                              float base_const, int M, int C, int H, int W, int patch, int cw, int chunks,
                                                              float* __restrict__ attr, double* __restrict__ cell64) {
    __shared__ double s_part[NT_FINISH];
    const int t = threadIdx.x, gh = H / patch, gw = W / patch, pv = patch / VEC;
    long long wg = blockIdx.x;
    const int chunk = (int)(wg % chunks); wg /= chunks;
    const int gy = (int)(wg % gh); wg /= gh;
    const long long bm = wg, b = bm / M;
    const int cell0 = chunk * cw, cells = min(cw, gw - cell0), ncol = cells * pv, rows = C * patch;
    int row0, rstep, col0, cstep;
    if (ncol <= NT_FINISH) {
        rstep = NT_FINISH / ncol; cstep = ncol;
        row0 = t < rstep * ncol ? t / ncol : rows;                                // the threads past the last full row of columns idle
        col0 = t % ncol;
    } else {
        row0 = 0; rstep = 1; col0 = t; cstep = NT_FINISH;
    }
    const size_t plane = (size_t)H * W;
    const float* __restrict__ accp = acc + (size_t)bm * C * plane;
    float* __restrict__ attrp = attr + (size_t)bm * C * plane;
    const float* __restrict__ xp = x + (size_t)b * C * plane;
    const float* __restrict__ bp = base ? base + (size_t)b * C * plane : nullptr;
    double part = 0.0;
#pragma unroll 2
    for (int row = row0; row < rows; row += rstep) {
        const int c = row / patch, py = row - c * patch;
        const size_t line = (size_t)c * plane + (size_t)(gy * patch + py) * W + (size_t)cell0 * patch;
        for (int col = col0; col < ncol; col += cstep) {
            const size_t e = line + (size_t)col * VEC;
            if constexpr (VEC == 4) {
                const float4 av = *reinterpret_cast<const float4*>(accp + e), xv = *reinterpret_cast<const float4*>(xp + e);
                const float4 bv = bp ? *reinterpret_cast<const float4*>(bp + e) : make_float4(base_const, base_const, base_const, base_const);
                const float4 o = make_float4(fmul_rn(fsub_rn(xv.x, bv.x), av.x), fmul_rn(fsub_rn(xv.y, bv.y), av.y),
                                             fmul_rn(fsub_rn(xv.z, bv.z), av.z), fmul_rn(fsub_rn(xv.w, bv.w), av.w));
                *reinterpret_cast<float4*>(attrp + e) = o;
                part += (double)o.x; part += (double)o.y; part += (double)o.z; part += (double)o.w;
            } else {
                const float o = fmul_rn(fsub_rn(xp[e], bp ? bp[e] : base_const), accp[e]);
                attrp[e] = o;
                part += (double)o;
            }
        }
    }
    s_part[t] = part;
    __syncthreads();
    if (t < cells) {                                                              // one thread per cell: its partials in ascending thread order
        double sum = 0.0;
        if (ncol <= NT_FINISH) {
            for (int r = 0; r < rstep; ++r)
                for (int k = 0; k < pv; ++k) sum += s_part[r * ncol + t * pv + k];
        } else {
            for (int k = 0; k < NT_FINISH; ++k) sum += s_part[k];
        }
        cell64[((size_t)bm * gh + gy) * gw + cell0 + t] = sum;
    }
}

bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

}  // namespace

extern "C" {

int ppf_ig_point(const float* x, const float* baseline, float baseline_const, float alpha, int64_t n, float* out, hipStream_t stream) {
    PPF_CHECK_ARG(n >= 1, PPF_ERR_SHAPE, "ppf_ig_point: n=%lld elements (>= 1)", (long long)n);
    PPF_CHECK_ARG(x && out, PPF_ERR_ARG, "ppf_ig_point: null pointer (x, out; only baseline may be NULL)");
    const bool vec = n % 4 == 0 && aligned16(x, baseline, out);
    const long long nvec = n / (vec ? 4 : 1), blocks = (nvec + NT_STREAM - 1) / NT_STREAM;
    PPF_CHECK_ARG(blocks <= INT_MAX, PPF_ERR_SHAPE, "ppf_ig_point: n=%lld exceeds the grid", (long long)n);
    if (vec) return ppf_launch<ig_point_kernel<4>>(dim3((unsigned)blocks), dim3(NT_STREAM), 0, stream, "ppf_ig_point", x, baseline, baseline_const, alpha, nvec, out);
    return ppf_launch<ig_point_kernel<1>>(dim3((unsigned)blocks), dim3(NT_STREAM), 0, stream, "ppf_ig_point", x, baseline, baseline_const, alpha, nvec, out);
}

int ppf_ig_accumulate(const float* g, float w, int first, int R, int64_t n, float* acc, int64_t acc_stride, hipStream_t stream) {
    PPF_CHECK_ARG(R >= 1 && n >= 1, PPF_ERR_SHAPE, "ppf_ig_accumulate: bad shape R=%d n=%lld (both >= 1)", R, (long long)n);
    PPF_CHECK_ARG(acc_stride >= n, PPF_ERR_SHAPE, "ppf_ig_accumulate: acc_stride=%lld below the row length n=%lld", (long long)acc_stride, (long long)n);
    PPF_CHECK_ARG(n <= LLONG_MAX / R && acc_stride <= LLONG_MAX / R, PPF_ERR_SHAPE, "ppf_ig_accumulate: R=%d x acc_stride=%lld overflows", R,
                  (long long)acc_stride);
    PPF_CHECK_ARG(first == 0 || first == 1, PPF_ERR_ARG, "ppf_ig_accumulate: first=%d must be 0 or 1", first);
    PPF_CHECK_ARG(g && acc, PPF_ERR_ARG, "ppf_ig_accumulate: null pointer (g, acc)");
    const bool vec = n % 4 == 0 && acc_stride % 4 == 0 && aligned16(g, acc);
    const long long nv = n / (vec ? 4 : 1), total = nv * R, blocks = (total + NT_STREAM - 1) / NT_STREAM;
    PPF_CHECK_ARG(blocks <= INT_MAX, PPF_ERR_SHAPE, "ppf_ig_accumulate: R=%d x n=%lld exceeds the grid", R, (long long)n);
    if (vec)
        return ppf_launch<ig_accumulate_kernel<4>>(dim3((unsigned)blocks), dim3(NT_STREAM), 0, stream, "ppf_ig_accumulate", g, w, first, nv, total, acc,
                                                   (long long)(acc_stride / 4));
    return ppf_launch<ig_accumulate_kernel<1>>(dim3((unsigned)blocks), dim3(NT_STREAM), 0, stream, "ppf_ig_accumulate", g, w, first, nv, total, acc,
                                               (long long)acc_stride);
}

int ppf_ig_finish(const float* acc, const float* x, const float* baseline, float baseline_const, int B, int M, int C, int H, int W, int patch,
                  float* attr, double* cell64, hipStream_t stream) {
    PPF_CHECK_ARG(B >= 1 && C >= 1 && H >= 1 && W >= 1 && patch >= 1, PPF_ERR_SHAPE, "ppf_ig_finish: bad shape B=%d C=%d H=%d W=%d patch=%d (all >= 1)", B,
                  C, H, W, patch);
    PPF_CHECK_ARG(M >= 1 && M <= 8, PPF_ERR_SHAPE, "ppf_ig_finish: M=%d outside [1, 8]", M);
    PPF_CHECK_ARG(H % patch == 0 && W % patch == 0, PPF_ERR_SHAPE, "ppf_ig_finish: patch=%d does not divide H=%d and W=%d", patch, H, W);
    const int gh = H / patch, gw = W / patch;
    PPF_CHECK_ARG((long long)gh * gw <= 1024, PPF_ERR_SHAPE, "ppf_ig_finish: G=%lld grid cells exceed 1024", (long long)gh * gw);
    PPF_CHECK_ARG((long long)C * patch <= INT_MAX, PPF_ERR_SHAPE, "ppf_ig_finish: C=%d x patch=%d rows per cell exceed 2^31 - 1", C, patch);
    PPF_CHECK_ARG(acc && x && attr && cell64, PPF_ERR_ARG, "ppf_ig_finish: null pointer (acc, x, attr, cell64; only baseline may be NULL)");
    PPF_CHECK_ARG(((uintptr_t)cell64 & 7) == 0, PPF_ERR_ALIGN, "ppf_ig_finish: cell64 must be 8-byte aligned");
    const bool vec = patch % 4 == 0 && aligned16(acc, x, baseline, attr);       // patch divides W: rows and cells start on vectors
    const int pv = patch / (vec ? 4 : 1);
    const int cw = pv >= NT_FINISH ? 1 : (NT_FINISH / pv < gw ? NT_FINISH / pv : gw), chunks = (gw + cw - 1) / cw;
    const long long blocks = (long long)B * M * gh * chunks;
    PPF_CHECK_ARG(blocks <= INT_MAX, PPF_ERR_SHAPE, "ppf_ig_finish: B=%d x M=%d x %d x %d workgroups exceed the grid", B, M, gh, chunks);
    if (vec)
        return ppf_launch<ig_finish_kernel<4>>(dim3((unsigned)blocks), dim3(NT_FINISH), 0, stream, "ppf_ig_finish", acc, x, baseline, baseline_const, M, C, H,
                                               W, patch, cw, chunks, attr, cell64);
    return ppf_launch<ig_finish_kernel<1>>(dim3((unsigned)blocks), dim3(NT_FINISH), 0, stream, "ppf_ig_finish", acc, x, baseline, baseline_const, M, C, H, W,
                                           patch, cw, chunks, attr, cell64);
}

}  // extern "C"
