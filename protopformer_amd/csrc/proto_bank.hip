// Prototype bank: a running, dataset-wide top-K of activations per prototype, kept on the device across batches
// (ProtoPNet-family "nearest patches" / prototype projection; the reference has no such pass -- its push step was dropped).
//   * proto_topk_merge_kernel: merges one batch's candidates (act_max [B][P] as ppf_proto_fwd writes it) into the persistent lists
//     val / img / pos [P][K], sorted best-first under a TOTAL order: larger activation first, equal activations by smaller image id.
//     The final state therefore does not depend on the batch size or on the order the batches arrive in.
//   * One wave owns a prototype (no atomics), lane j holds list entry j (K <= 64).  A workgroup of 4 waves covers 32 prototypes, 8 per
//     wave, their lists in registers for the whole launch.  The lanes of a wave want a COLUMN of act_max (stride P), so 64 rows x 32
//     prototypes are staged through LDS with row-contiguous 128-byte loads and read back by column (leading dimension 33: conflict-free).
//   * A candidate is first tested by ballot against the current K-th entry: after the first few batches almost nothing survives, and a
//     chunk costs one LDS read, one compare and one ballot per prototype.  A survivor's rank is the number of entries that beat it
//     (popcount of a ballot: the list is sorted, so these are a prefix); the entries from that rank on move one lane up.
//   * The latent token of a prototype's rank-0 entry is copied into best_feat [P][Dp] at the end of the launch, only when this launch
//     changed rank 0 (the source sample is remembered as a wave-uniform index; nothing of size B x Dp is kept).
// NaN never compares greater or equal, so a NaN candidate is never admitted; neither is -inf (it does not beat an unfilled slot).
#include <math.h>

#include "ppf_common.h"
#include "ppf_hip.h"
#include "ppf_select.h"

namespace {

constexpr int TP = 32;                 // prototypes per workgroup
constexpr int PW = 8;                  // prototypes per wave
constexpr int CH = 64;                 // samples per staged chunk (one per lane)
constexpr int LD = TP + 1;             // LDS leading dimension of the staged tile

__global__ __launch_bounds__(256) void proto_topk_init_kernel(float* __restrict__ val, int* __restrict__ img, int* __restrict__ pos, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    val[i] = -INFINITY;
    img[i] = -1;
    pos[i] = -1;
}

// grid: ceil(P / TP) workgroups of 256 threads.  The list steps (survivors, rank, placement) are ppf_select.h's, shared with explain.hip.
__global__ __launch_bounds__(256) void proto_topk_merge_kernel(const float* __restrict__ act_max, const int* __restrict__ argmax,
                                                               const int* __restrict__ idx, int k, const float* __restrict__ tok,
                                                               long long stride_b, int t0, int Dp, const long long* __restrict__ label,
                                                               const int* __restrict__ image_id, int ppc, int B, int P, int K,
                                                               float* __restrict__ val, int* __restrict__ img, int* __restrict__ pos,
                                                               float* __restrict__ best_feat) {
    __shared__ float tile[CH * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p_blk = blockIdx.x * TP;
    const int p_wave = p_blk + wave * PW;

    float sv[PW];
    int si[PW], sp[PW], best_b[PW];                          // best_b: sample of this launch that became rank 0 (wave-uniform), -1: none
#pragma unroll
    for (int q = 0; q < PW; ++q) {
        const int p = p_wave + q;
        const bool live = p < P && lane < K;
        sv[q] = live ? val[(size_t)p * K + lane] : -INFINITY;
        si[q] = live ? img[(size_t)p * K + lane] : -1;
        sp[q] = live ? pos[(size_t)p * K + lane] : -1;
        best_b[q] = -1;
    }

    for (int b0 = 0; b0 < B; b0 += CH) {
        // stage act_max[b0 .. b0+64)[p_blk .. p_blk+32): thread -> (row tid/32 + 8 i, column tid%32), 128 contiguous bytes per half wave
        const int c = tid & (TP - 1), r0 = tid >> 5;
#pragma unroll
        for (int i = 0; i < CH / 8; ++i) {
            const int r = r0 + 8 * i, b = b0 + r, p = p_blk + c;
            tile[r * LD + c] = (b < B && p < P) ? act_max[(size_t)b * P + p] : -INFINITY;
        }
        __syncthreads();

        const int b = b0 + lane;
        const bool row_in = b < B;
        const int my_id = row_in ? image_id[b] : -1;
        const long long my_label = (row_in && ppc > 0) ? label[b] : -1;
#pragma unroll
        for (int q = 0; q < PW; ++q) {
            const int p = p_wave + q;
            if (p >= P) break;                                               // wave-uniform
            const float v = tile[lane * LD + wave * PW + q];
            const bool offered = row_in && (ppc <= 0 || my_label == (long long)(p / ppc));
            unsigned long long surv = list_survivors(offered, v, my_id, sv[q], si[q], K);
            while (surv) {                                                    // wave-uniform loop over the survivors of the prefilter
                ListCand<int> c = list_next(surv, v, my_id, -1, sv[q], si[q], K, lane);
                if (!c.enters) continue;
                const int cb = b0 + c.src;
                if (argmax) {                                                 // the payload: looked up only for a candidate that enters
                    const int am = min(max(argmax[(size_t)cb * P + p], 0), k - 1);
                    c.pay = idx[(size_t)cb * k + am];
                }
                list_place(c, K, lane, sv[q], si[q], sp[q]);
                if (c.rank == 0) best_b[q] = cb;
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int q = 0; q < PW; ++q) {
        const int p = p_wave + q;
        if (p >= P) break;
        if (lane < K) {
            val[(size_t)p * K + lane] = sv[q];
            img[(size_t)p * K + lane] = si[q];
            pos[(size_t)p * K + lane] = sp[q];
        }
        const int bb = best_b[q];
        if (bb < 0) continue;
        const int am = argmax ? min(max(argmax[(size_t)bb * P + p], 0), k - 1) : 0;
        const float4* src = reinterpret_cast<const float4*>(tok + (size_t)bb * stride_b + (size_t)(t0 + am) * Dp);
        float4* dst = reinterpret_cast<float4*>(best_feat + (size_t)p * Dp);
        for (int i = lane; i < Dp / 4; i += 64) dst[i] = src[i];
    }
}

}  // namespace

extern "C" {

int ppf_proto_topk_init(float* val, int* img, int* pos, int P, int K, hipStream_t stream) {
    PPF_CHECK_ARG(P >= 1 && K >= 1 && K <= 64, PPF_ERR_SHAPE, "ppf_proto_topk_init: bad shape P=%d K=%d (P >= 1, 1 <= K <= 64)", P, K);
    PPF_CHECK_ARG(val && img && pos, PPF_ERR_ARG, "ppf_proto_topk_init: null pointer");
    const size_t n = (size_t)P * K;
    return ppf_launch<proto_topk_init_kernel>(dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, "ppf_proto_topk_init", val, img, pos, n);
}

int ppf_proto_topk_merge(const float* act_max, const int* argmax, const int* idx, int k, const float* tok, int64_t stride_b, int t0, int Dp,
                         const void* label_i64, const int* image_id, int ppc, int B, int P, int K, float* val, int* img, int* pos,
                         float* best_feat, hipStream_t stream) {
    PPF_CHECK_ARG(K >= 1 && K <= 64, PPF_ERR_SHAPE, "ppf_proto_topk_merge: K=%d outside [1, 64] (one list entry per lane)", K);
    PPF_CHECK_ARG(B >= 1 && B <= 1024, PPF_ERR_SHAPE, "ppf_proto_topk_merge: B=%d outside [1, 1024]", B);
    PPF_CHECK_ARG(P >= 1, PPF_ERR_SHAPE, "ppf_proto_topk_merge: P=%d must be >= 1", P);
    PPF_CHECK_ARG(Dp >= 4 && Dp % 4 == 0, PPF_ERR_SHAPE, "ppf_proto_topk_merge: Dp=%d must be a positive multiple of 4", Dp);
    PPF_CHECK_ARG(t0 >= 0 && ppc >= 0 && stride_b >= 0, PPF_ERR_SHAPE, "ppf_proto_topk_merge: bad t0=%d ppc=%d stride_b=%lld", t0, ppc, (long long)stride_b);
    PPF_CHECK_ARG((argmax == nullptr) == (idx == nullptr), PPF_ERR_ARG, "ppf_proto_topk_merge: argmax and idx must both be given or both be NULL");
    PPF_CHECK_ARG(argmax == nullptr || k >= 1, PPF_ERR_SHAPE, "ppf_proto_topk_merge: k=%d reserved tokens with an argmax", k);
    PPF_CHECK_ARG(act_max && tok && image_id && val && img && pos && best_feat && (ppc == 0 || label_i64), PPF_ERR_ARG,
                  "ppf_proto_topk_merge: null pointer");
    PPF_CHECK_ARG(stride_b % 4 == 0 && (((uintptr_t)tok | (uintptr_t)best_feat) & 15) == 0, PPF_ERR_ALIGN,
                  "ppf_proto_topk_merge: tok / best_feat must be 16-byte aligned and stride_b a multiple of 4");
    return ppf_launch<proto_topk_merge_kernel>(dim3((P + TP - 1) / TP), dim3(256), 0, stream, "ppf_proto_topk_merge", act_max, argmax, idx, k, tok, (long long)stride_b,
                                               t0, Dp, (const long long*)label_i64, image_id, ppc, B, P, K, val, img, pos, best_feat);
}

}  // extern "C"
