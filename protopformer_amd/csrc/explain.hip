// Local analysis: why did this image get this class?  For every (sample, class) pair the K prototypes with the largest class evidence
// act_max[b][p] * (scale * weight[c][p]), the evidence totals, and the activation maps of the selected prototypes on the full patch grid,
// all from what an eval forward leaves on the device (ProtoPNet's "local analysis"; the reference has no such pass -- its
// main_visualize.py draws every prototype of a chosen class and never ranks evidence).
//   * explain_topk_kernel: one wave owns one (b, m) list (no atomics), lane j holds list entry j (K <= 64), as in proto_bank.hip.  The
//     form kept is ONE WAVE PER WORKGROUP: at B = 256, M = 1 the 256 lists then spread over 256 compute units instead of 64, and nothing
//     is shared between the lists of a workgroup that the caches do not already share (the act_max row of a sample).  P is not split over
//     waves: the list and the sums are those of a single in-order pass.
//   * Classes: given (cls_in) or picked by the wave itself as the top-M of its logits row with the same list mechanism (larger logit
//     first, equal logits by smaller class id, NaN never picked); the wave of slot m takes entry m.
//   * P is streamed in chunks of 64 with coalesced reads of the act_max and weight rows, the loads of four chunks issued together (a
//     launch is a few hundred waves that each walk P alone: it is bound by the chain of memory round trips, not by bandwidth); the
//     chunks are then offered one after the other in ascending order, so nothing depends on the grouping.  A chunk is tested by ballot
//     against the current K-th entry; a survivor's rank is the popcount of the ballot of the entries that come before it (the list is
//     sorted, so these are a prefix); the entries from that rank on move one lane up.  The order is total: sign * contribution
//     descending, equal keys by smaller prototype id.  Both products are separate fp32 multiplications (__fmul_rn: no contraction with
//     the sums).  NaN and +-inf contributions are never admitted, but they are part of the evidence sums.
//   * Evidence: per-lane fp64 partial sums over the chunks, one shuffle reduction at the end, one rounding to fp32.
//   * Maps: written by the wave after the list is final.  The inverse of idx[b] (grid cell -> reserved token, -1 elsewhere) is built once
//     in LDS, so every cell of every map is written exactly once, coalesced: zero, or act_full[b][p][t] at cell idx[b][t].
//   * evidence_focus_kernel: the same walk over P without a list; the evidence of a class split four ways, by own / other class and by
//     whether the prototype's cell has its centre pixel inside the image's object box (interpret.foreground_focus).
#include <limits.h>
#include <math.h>

#include "ppf_common.h"
#include "ppf_hip.h"
#include "ppf_select.h"

namespace {

constexpr int NO_ID = INT_MAX;          // id of an unfilled list entry (sorts last among equal keys; a finite key always beats -inf)
constexpr int UNR = 4;                  // chunks whose loads are issued together (the wave's walk over P is a chain of memory round trips)
constexpr int MAX_G = 8192;             // grid cells whose inverse index fits the static 48 KiB of LDS with room to spare

// Offers the candidate (v, id, pay) of every lane with `offered` set to the sorted list (sk, sid, sp) held one entry per lane (K entries):
// the list steps of ppf_select.h, the payload shuffled from the source lane.
__device__ __forceinline__ void offer_chunk(bool offered, float v, int id, float pay, int K, int lane, float& sk, int& sid, float& sp) {
    unsigned long long surv = list_survivors(offered, v, id, sk, sid, K);
    while (surv) {                                                            // wave-uniform loop over the survivors of the prefilter
        const ListCand<float> c = list_next(surv, v, id, pay, sk, sid, K, lane);
        if (c.enters) list_place(c, K, lane, sk, sid, sp);
    }
}

// grid: B * M workgroups of one wave; dynamic LDS: G ints when maps != NULL
__global__ __launch_bounds__(64) void explain_topk_kernel(const float* __restrict__ act_max, const int* __restrict__ argmax, const int* __restrict__ idx,
                                                          int T, const float* __restrict__ act_full, const float* __restrict__ weight, float scale,
                                                          int ppc, const float* __restrict__ logits, const int* __restrict__ cls_in, int sign, int P,
                                                          int C, int M, int K, int G, int* __restrict__ cls_out, float* __restrict__ cls_logit,
                                                          int* __restrict__ proto, float* __restrict__ contrib, float* __restrict__ act,
                                                          int* __restrict__ cell, float* __restrict__ evidence, float* __restrict__ maps) {
    extern __shared__ int inv[];                                              // inv[g] = the reserved token that sits at grid cell g, or -1
    const int lane = threadIdx.x;
    const int list = blockIdx.x, b = list / M, m = list - b * M;

    // ---- the class of this list
    int c = -1;
    float c_logit = -INFINITY;
    if (cls_in) {
        c = cls_in[list];
        if (c >= 0 && c < C) c_logit = logits[(size_t)b * C + c];
        else c = -1;
    } else {
        float ck = -INFINITY, cpay = 0.0f;
        int cid = NO_ID;
        for (int c0 = 0; c0 < C; c0 += 64 * UNR) {
            float v[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int cc = c0 + u * 64 + lane;
                v[u] = cc < C ? logits[(size_t)b * C + cc] : NAN;
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int cc = c0 + u * 64 + lane;
                if (c0 + u * 64 < C) offer_chunk(cc < C && v[u] == v[u], v[u], cc, 0.0f, M, lane, ck, cid, cpay);   // -inf is a logit like any other; NaN is not offered
            }
        }
        const int pick = __shfl(cid, m, 64);
        if (pick != NO_ID) { c = pick; c_logit = __shfl(ck, m, 64); }
    }
    c = __builtin_amdgcn_readfirstlane(c);                                    // wave-uniform: the weight row below is addressed by scalars
    if (lane == 0) { cls_out[list] = c; cls_logit[list] = c_logit; }

    // ---- the list and the evidence sums
    float sk = -INFINITY, sa = -INFINITY;                                     // key = sign * contribution, activation
    int sid = NO_ID;
    double ev_own = 0.0, ev_other = 0.0;
    if (c >= 0) {
        const float* __restrict__ arow = act_max + (size_t)b * P;
        const float* __restrict__ wrow = weight + (size_t)c * P;
        const int own_lo = c * ppc, own_hi = own_lo + ppc;                    // p / ppc == c
        for (int p0 = 0; p0 < P; p0 += 64 * UNR) {
            float av[UNR], wv[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {                                   // the loads of UNR chunks in flight together ...
                const int p = p0 + u * 64 + lane;
                av[u] = p < P ? arow[p] : 0.0f;
                wv[u] = p < P ? wrow[p] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {                                   // ... the chunks themselves one after the other, in order
                const int p = p0 + u * 64 + lane;
                if (p0 + u * 64 >= P) break;                                  // wave-uniform
                const bool in = p < P;
                const float a = av[u];
                const float w = __fmul_rn(scale, wv[u]);
                const float ctr = __fmul_rn(a, w);
                if (in) {
                    if (p >= own_lo && p < own_hi) ev_own += (double)ctr;
                    else ev_other += (double)ctr;
                }
                offer_chunk(in && isfinite(ctr), sign > 0 ? ctr : -ctr, p, a, K, lane, sk, sid, sa);
            }
        }
    }
    ev_own = wave_sum_f64(ev_own);
    ev_other = wave_sum_f64(ev_other);
    if (lane == 0) {
        evidence[(size_t)list * 2] = (float)ev_own;
        evidence[(size_t)list * 2 + 1] = (float)ev_other;
    }

    const bool filled = sid != NO_ID;
    if (lane < K) {
        int at = -1;
        if (filled && argmax) {
            const int t = argmax[(size_t)b * P + sid];
            if (t >= 0 && t < T) at = idx[(size_t)b * T + t];
        }
        const size_t o = (size_t)list * K + lane;
        proto[o] = filled ? sid : -1;
        contrib[o] = filled ? (sign > 0 ? sk : -sk) : -INFINITY;              // exact: the key is the contribution or its negation
        act[o] = filled ? sa : -INFINITY;
        cell[o] = at;
    }

    // ---- the maps of the selected prototypes on the full grid
    if (!maps) return;                                                        // kernel-uniform
    for (int g = lane; g < G; g += 64) inv[g] = -1;
    __syncthreads();
    for (int t = lane; t < T; t += 64) {
        const int g = idx[(size_t)b * T + t];
        if (g >= 0 && g < G) inv[g] = t;                                      // the cells of a sample are distinct (caller's contract)
    }
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        const int pk = __shfl(sid, k, 64);                                    // wave-uniform
        float* __restrict__ out = maps + ((size_t)list * K + k) * G;
        const float* __restrict__ src = pk != NO_ID ? act_full + ((size_t)b * P + pk) * T : nullptr;
        for (int g = lane; g < G; g += 64) {
            const int t = inv[g];
            out[g] = (src && t >= 0) ? src[t] : 0.0f;
        }
    }
}

// Foreground focus of the evidence: the contributions of explain_topk_kernel (the same two roundings), split by whose class the prototype
// is and by whether its cell's centre pixel lies in the image's object box.  One wave per (sample, class) row, per-lane fp64 partial sums
// over the chunks, one shuffle reduction: no atomics.  grid: B * M workgroups of one wave.
__global__ __launch_bounds__(64) void evidence_focus_kernel(const float* __restrict__ act_max, const int* __restrict__ argmax, const int* __restrict__ idx,
                                                            int T, const float* __restrict__ weight, float scale, int ppc, const int* __restrict__ classes,
                                                            const int* __restrict__ obj, int g, int patch, int P, int C, int M, double* __restrict__ ev,
                                                            int* __restrict__ cnt) {
    const int lane = threadIdx.x;
    const int list = blockIdx.x, b = list / M;
    int c = classes[list];
    if (c < 0 || c >= C) c = -1;
    c = __builtin_amdgcn_readfirstlane(c);
    double s[4] = {0.0, 0.0, 0.0, 0.0};                                       // own & inside, own & not, other & inside, other & not
    int n[4] = {0, 0, 0, 0};
    if (c >= 0) {
        const int S = g * patch, G = g * g;
        const int* o = obj + 4 * (size_t)b;
        const int y0 = min(max(o[0], 0), S), y1 = min(max(o[1], 0), S), x0 = min(max(o[2], 0), S), x1 = min(max(o[3], 0), S);
        const float* __restrict__ arow = act_max + (size_t)b * P;
        const float* __restrict__ wrow = weight + (size_t)c * P;
        const int own_lo = c * ppc, own_hi = own_lo + ppc;
        for (int p0 = 0; p0 < P; p0 += 64 * UNR) {
            float av[UNR], wv[UNR];
            int tv[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int p = p0 + u * 64 + lane;
                av[u] = p < P ? arow[p] : 0.0f;
                wv[u] = p < P ? wrow[p] : 0.0f;
                tv[u] = (p < P && argmax) ? argmax[(size_t)b * P + p] : 0;
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int p = p0 + u * 64 + lane;
                if (p >= P) continue;
                const float ctr = __fmul_rn(av[u], __fmul_rn(scale, wv[u]));
                bool in = false;
                if (tv[u] >= 0 && tv[u] < T) {
                    const int cell = idx[(size_t)b * T + tv[u]];
                    if (cell >= 0 && cell < G) {
                        const int cy = cell / g, cx = cell - cy * g;
                        const int py = cy * patch + patch / 2, px = cx * patch + patch / 2;
                        in = py >= y0 && py < y1 && px >= x0 && px < x1;
                    }
                }
                const int k = ((p >= own_lo && p < own_hi) ? 0 : 2) + (in ? 0 : 1);
#pragma unroll
                for (int j = 0; j < 4; ++j) {                                 // (no dynamic register index)
                    s[j] += j == k ? (double)ctr : 0.0;
                    n[j] += j == k ? 1 : 0;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s[j] = wave_sum_f64(s[j]);
        n[j] = wave_sum_i32(n[j]);
    }
    if (lane < 4) {
        double sv = s[0];
        int nv = n[0];
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if (lane == j) { sv = s[j]; nv = n[j]; }
        ev[4 * (size_t)list + lane] = sv;
        cnt[4 * (size_t)list + lane] = nv;
    }
}

}  // namespace

extern "C" {

int ppf_explain_topk(const float* act_max, const int* argmax, const int* idx, int T, const float* act_full, const float* weight, float scale,
                     int ppc, const float* logits, const int* cls_in, int sign, int B, int P, int C, int M, int K, int G, int* cls_out,
                     float* cls_logit, int* proto, float* contrib, float* act, int* cell, float* evidence, float* maps, hipStream_t stream) {
    PPF_CHECK_ARG(K >= 1 && K <= 64, PPF_ERR_SHAPE, "ppf_explain_topk: K=%d outside [1, 64] (one list entry per lane)", K);
    PPF_CHECK_ARG(M >= 1 && M <= 8, PPF_ERR_SHAPE, "ppf_explain_topk: M=%d outside [1, 8] (classes explained per sample)", M);
    PPF_CHECK_ARG(C >= 1 && M <= C, PPF_ERR_SHAPE, "ppf_explain_topk: M=%d classes per sample of C=%d (1 <= M <= C)", M, C);
    PPF_CHECK_ARG(B >= 1 && P >= 1, PPF_ERR_SHAPE, "ppf_explain_topk: bad shape B=%d P=%d (both >= 1)", B, P);
    PPF_CHECK_ARG((long long)B * M <= INT_MAX, PPF_ERR_SHAPE, "ppf_explain_topk: B=%d x M=%d lists exceed the grid", B, M);
    PPF_CHECK_ARG(ppc >= 1 && P % ppc == 0, PPF_ERR_SHAPE, "ppf_explain_topk: ppc=%d must be >= 1 and divide P=%d", ppc, P);
    PPF_CHECK_ARG((long long)C * ppc <= INT_MAX, PPF_ERR_SHAPE, "ppf_explain_topk: C=%d x ppc=%d overflows", C, ppc);
    PPF_CHECK_ARG(sign == 1 || sign == -1, PPF_ERR_ARG, "ppf_explain_topk: sign=%d must be +1 (evidence for) or -1 (evidence against)", sign);
    PPF_CHECK_ARG((argmax == nullptr) == (idx == nullptr), PPF_ERR_ARG, "ppf_explain_topk: argmax and idx must both be given or both be NULL");
    PPF_CHECK_ARG(argmax != nullptr || (act_full == nullptr && maps == nullptr), PPF_ERR_ARG,
                  "ppf_explain_topk: the global branch (argmax NULL) has no act_full and no maps");
    PPF_CHECK_ARG(argmax == nullptr || T >= 1, PPF_ERR_SHAPE, "ppf_explain_topk: T=%d reserved tokens with an argmax", T);
    PPF_CHECK_ARG(maps == nullptr || act_full != nullptr, PPF_ERR_ARG, "ppf_explain_topk: maps need act_full");
    PPF_CHECK_ARG(maps == nullptr || (G >= 1 && G <= MAX_G), PPF_ERR_SHAPE, "ppf_explain_topk: G=%d grid cells outside [1, %d]", G, MAX_G);
    PPF_CHECK_ARG(act_max && weight && logits && cls_out && cls_logit && proto && contrib && act && cell && evidence, PPF_ERR_ARG,
                  "ppf_explain_topk: null pointer");
    return ppf_launch<explain_topk_kernel>(dim3((unsigned)(B * M)), dim3(64), maps ? (size_t)G * sizeof(int) : 0, stream, "ppf_explain_topk", act_max,
                                           argmax, idx, T, act_full, weight, scale, ppc, logits, cls_in, sign, P, C, M, K, G, cls_out, cls_logit, proto,
                                           contrib, act, cell, evidence, maps);
}

int ppf_evidence_focus(const float* act_max, const int* argmax, const int* idx, int T, const float* weight, float scale, int ppc, const int* classes,
                       const int* obj, int g, int patch, int B, int P, int C, int M, double* ev, int* cnt, hipStream_t stream) {
    PPF_CHECK_ARG(M >= 1 && M <= 8, PPF_ERR_SHAPE, "ppf_evidence_focus: M=%d outside [1, 8] (classes per sample)", M);
    PPF_CHECK_ARG(B >= 1 && P >= 1 && C >= 1 && T >= 1, PPF_ERR_SHAPE, "ppf_evidence_focus: bad shape B=%d P=%d C=%d T=%d (all >= 1)", B, P, C, T);
    PPF_CHECK_ARG((long long)B * M <= INT_MAX, PPF_ERR_SHAPE, "ppf_evidence_focus: B=%d x M=%d rows exceed the grid", B, M);
    PPF_CHECK_ARG(ppc >= 1 && P % ppc == 0 && (long long)C * ppc <= INT_MAX, PPF_ERR_SHAPE, "ppf_evidence_focus: ppc=%d must be >= 1 and divide P=%d (C=%d)",
                  ppc, P, C);
    PPF_CHECK_ARG(g >= 1 && patch >= 1 && (long long)g * patch <= 32768, PPF_ERR_SHAPE, "ppf_evidence_focus: bad grid g=%d patch=%d (both >= 1, g * patch <= 32768)",
                  g, patch);
    PPF_CHECK_ARG(act_max && idx && weight && classes && obj && ev && cnt, PPF_ERR_ARG, "ppf_evidence_focus: null pointer (only argmax may be NULL)");
    return ppf_launch<evidence_focus_kernel>(dim3((unsigned)(B * M)), dim3(64), 0, stream, "ppf_evidence_focus", act_max, argmax, idx, T, weight, scale, ppc,
                                             classes, obj, g, patch, P, C, M, ev, cnt);
}

}  // extern "C"
