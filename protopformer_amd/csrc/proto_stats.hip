// Prototype statistics: the distribution of every prototype's pooled activation over a whole data set, split into own-class and
// other-class images, and how often two prototypes of a class point at the same grid cell (ProtoPNet's pruning pass and the
// activation percentiles of its local analysis need exactly this; the reference has neither).  One call folds a batch's act_max [B][P]
// (and, on the local branch, argmax / idx) into small persistent int32 tables; nothing of size B x P is read back.
//   * proto_hist_kernel: lanes along p (coalesced rows of act_max), one wave per 64 consecutive prototypes and per strip of rows.  Each
//     lane keeps its prototype's [2][NB] counters in LDS as [slot * NB + bin][lane]: a wave-instruction touches 64 consecutive words
//     (conflict-free), and only the owning lane ever touches a word, so the increments need no LDS atomics.  At the end the non-zero
//     counters go to the global table by atomicAdd.  The column-group-0 waves also count their strip's labels into images / bad.
//   * proto_coloc_kernel: one wave per sample; lane q holds the cell of prototype c * ppc + q of the sample's class c, a loop over the
//     class's prototypes broadcasts one cell at a time and the lanes that fired at the same cell add one to coloc[p][q].
// The bin is t = fl(fl(a - lo) * inv_width) without contraction (__fsub_rn / __fmul_rn): numpy's float32 arithmetic gives the same bits.
// Integer atomics only: any split of the same images into batches, in any order, leaves the same tables.
#include <limits.h>
#include <math.h>

#include "ppf_common.h"
#include "ppf_hip.h"

namespace {

constexpr int MIN_ROWS = 8;            // rows per strip at least: below this the LDS clear and flush outweigh the rows
constexpr int RC = 8;                  // rows whose loads are in flight together

// grid (ceil(P / 64), strips), 64 threads, dynamic LDS 2 * NB * 64 ints.
__global__ __launch_bounds__(64) void proto_hist_kernel(const float* __restrict__ act_max, const long long* __restrict__ label, int ppc, int B, int P,
                                                        int NB, float lo, float inv_width, int rows_per_strip, int* __restrict__ hist,
                                                        int* __restrict__ nan_count, int* __restrict__ images, int* __restrict__ bad) {
    extern __shared__ int cnt[];                                       // [2 * NB][64]
    const int lane = threadIdx.x;
    const int p = blockIdx.x * 64 + lane;
    const int b0 = blockIdx.y * rows_per_strip, b1 = min(B, b0 + rows_per_strip);
    const int C = P / ppc;

    if (blockIdx.x == 0) {                                             // this strip's labels: images[c] += 1, or bad[0] += 1
        for (int b = b0 + lane; b < b1; b += 64) {
            const long long c = label[b];
            if (c < 0 || c >= C) atomicAdd(bad, 1);
            else atomicAdd(images + c, 1);
        }
    }
    for (int i = 0; i < 2 * NB; ++i) cnt[i * 64 + lane] = 0;           // own column only: no barrier needed (one wave, one owner per word)

    const bool live = p < P;
    const int my_class = live ? p / ppc : -1;
    const float fnb = (float)NB;
    int nan_own = 0, nan_other = 0;
    // RC rows at a time: their labels, then their activations, are all requested before the first is used (a row costs one memory
    // latency otherwise: the counter update of row b would stand between the loads of rows b and b + 1)
    for (int b = b0; b < b1; b += RC) {
        long long c[RC];
        float a[RC];
#pragma unroll
        for (int j = 0; j < RC; ++j) c[j] = label[min(b + j, b1 - 1)];  // wave-uniform
#pragma unroll
        for (int j = 0; j < RC; ++j) {
            const bool use = b + j < b1 && c[j] >= 0 && c[j] < C;       // wave-uniform; a bad label reads nothing else and adds nothing else
            if (!use) c[j] = -1;
            a[j] = use && live ? act_max[(size_t)(b + j) * P + p] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < RC; ++j) {
            if (c[j] < 0 || !live) continue;
            const int slot = (long long)my_class == c[j] ? 0 : 1;
            if (a[j] != a[j]) {
                if (slot == 0) ++nan_own; else ++nan_other;
                continue;
            }
            const float t = __fmul_rn(__fsub_rn(a[j], lo), inv_width);
            const int bin = t < 0.0f ? 0 : (t >= fnb ? NB - 1 : (int)t);
            cnt[(slot * NB + bin) * 64 + lane] += 1;
        }
    }
    if (!live) return;
    int* h = hist + (size_t)p * 2 * NB;
    for (int i = 0; i < 2 * NB; ++i) {
        const int v = cnt[i * 64 + lane];
        if (v != 0) atomicAdd(h + i, v);
    }
    if (nan_own != 0) atomicAdd(nan_count + 2 * (size_t)p, nan_own);
    if (nan_other != 0) atomicAdd(nan_count + 2 * (size_t)p + 1, nan_other);
}

// grid ceil(B / 4), 256 threads: one wave per sample.
__global__ __launch_bounds__(256) void proto_coloc_kernel(const int* __restrict__ argmax, const int* __restrict__ idx, int T,
                                                          const long long* __restrict__ label, int ppc, int B, int P, int* __restrict__ coloc) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                                // wave-uniform
    const long long c = label[b];
    if (c < 0 || c >= P / ppc) return;                                 // wave-uniform
    const int first = (int)c * ppc;
    int cell = 0;
    bool valid = false;
    if (lane < ppc) {
        const int am = argmax[(size_t)b * P + first + lane];
        valid = am >= 0 && am < T;
        if (valid) cell = idx[(size_t)b * T + am];
    }
    for (int i = 0; i < ppc; ++i) {                                    // wave-uniform trip count: every lane takes part in the broadcast
        const int cell_i = __shfl(cell, i, 64);
        const int valid_i = __shfl((int)valid, i, 64);
        if (valid && valid_i && cell == cell_i) atomicAdd(coloc + ((size_t)(first + i)) * ppc + lane, 1);
    }
}

}  // namespace

extern "C" {

int ppf_proto_stats_update(const float* act_max, const int* argmax, const int* idx, int T, const void* label_i64, int ppc, int B, int P, int NB,
                           float lo, float inv_width, int* hist, int* nan_count, int* coloc, int* images, int* bad, hipStream_t stream) {
    PPF_CHECK_ARG(B >= 1 && B <= 1024, PPF_ERR_SHAPE, "ppf_proto_stats_update: B=%d outside [1, 1024]", B);
    PPF_CHECK_ARG(ppc >= 1 && ppc <= 64, PPF_ERR_SHAPE, "ppf_proto_stats_update: ppc=%d outside [1, 64] (one prototype of the class per lane)", ppc);
    PPF_CHECK_ARG(P >= 1 && P % ppc == 0, PPF_ERR_SHAPE, "ppf_proto_stats_update: P=%d must be a positive multiple of ppc=%d", P, ppc);
    PPF_CHECK_ARG(NB >= 8 && NB <= 128, PPF_ERR_SHAPE, "ppf_proto_stats_update: NB=%d bins outside [8, 128]", NB);
    PPF_CHECK_ARG(isfinite(lo) && isfinite(inv_width) && inv_width > 0.0f, PPF_ERR_SHAPE,
                  "ppf_proto_stats_update: lo=%g must be finite and inv_width=%g finite and > 0", (double)lo, (double)inv_width);
    PPF_CHECK_ARG((long long)P * 2 * NB <= INT_MAX && (long long)P * ppc <= INT_MAX, PPF_ERR_SHAPE,
                  "ppf_proto_stats_update: P=%d ppc=%d NB=%d: a table exceeds 2^31 entries", P, ppc, NB);
    PPF_CHECK_ARG((argmax == nullptr) == (idx == nullptr), PPF_ERR_ARG, "ppf_proto_stats_update: argmax and idx must both be given or both be NULL");
    PPF_CHECK_ARG(argmax == nullptr || T >= 1, PPF_ERR_SHAPE, "ppf_proto_stats_update: T=%d reserved tokens with an argmax", T);
    PPF_CHECK_ARG(act_max && label_i64 && hist && nan_count && images && bad && (argmax == nullptr || coloc), PPF_ERR_ARG,
                  "ppf_proto_stats_update: null pointer (only argmax / idx / coloc may be NULL, together: the global branch)");
    // strips: the grid reaches about the CU count (P / 64 = 32 column groups x 8 strips of 32 rows at batch 256 and 2000 prototypes)
    const int groups = (P + 63) / 64, cu = ppf_cu_count();
    const int want = cu / groups > 1 ? cu / groups : 1;
    int rows = (B + want - 1) / want;
    if (rows < MIN_ROWS) rows = MIN_ROWS;
    const int strips = (B + rows - 1) / rows;
    const long long* label = (const long long*)label_i64;
    if (int rc = ppf_launch<proto_hist_kernel>(dim3((unsigned)groups, (unsigned)strips), dim3(64), (size_t)2 * NB * 64 * sizeof(int), stream,
                                               "ppf_proto_stats_update", act_max, label, ppc, B, P, NB, lo, inv_width, rows, hist, nan_count, images,
                                               bad))
        return rc;
    if (argmax == nullptr) return 0;
    return ppf_launch<proto_coloc_kernel>(dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, "ppf_proto_stats_update", argmax, idx, T, label, ppc, B,
                                          P, coloc);
}

}  // extern "C"
