// Ordering and selection steps shared by the ranking kernels (device code; the order itself is order_keys.h): a sorted list of K <= 64
// entries held one per lane (proto_bank.hip, explain.hip), rank by counting over keys in LDS (rollout.hip, faithful.hip), and the steps of
// one 8-bit radix-select pass around a kernel's own histogram feed (rollout.hip, interp.hip).  Everything is __forceinline__ over
// references to the caller's registers: no helper takes the address of a register array.
#pragma once
#include "order_keys.h"
#include "ppf_common.h"

// ---- sorted list, entry j in lane j (lanes >= K hold the caller's fill and never take part) ---------------------------------------------
// The lanes whose candidate (v, id) is offered and comes before the current K-th entry: after the first few chunks almost none.
__device__ __forceinline__ unsigned long long list_survivors(bool offered, float v, int id, float sk, int sid, int K) {
    const float kv = __shfl(sk, K - 1, 64);               // in front of the condition: lane K - 1 must take part in the shuffles
    const int ki = __shfl(sid, K - 1, 64);
    return __ballot(offered && comes_before(v, id, kv, ki));
}
// Takes the next survivor off `surv` (wave-uniform): its lane, key, payload and id, and its rank in the list -- the entries that come before
// it are a prefix of the sorted list, so their count is the rank.  enters false: the list moved on since the prefilter, the candidate is
// dropped.  Pay: one 32-bit payload per entry; a caller that looks its payload up (the bank) passes its "none" and sets c.pay afterwards.
template <typename Pay> struct ListCand { int src, id, rank; float v; Pay pay; bool enters; };
template <typename Pay>
__device__ __forceinline__ ListCand<Pay> list_next(unsigned long long& surv, float v, int id, Pay pay, float sk, int sid, int K, int lane) {
    ListCand<Pay> c;
    c.src = __ffsll((long long)surv) - 1;
    surv &= surv - 1;
    c.v = __shfl(v, c.src, 64);
    c.pay = __shfl(pay, c.src, 64);                       // the three shuffles together, in front of the rank's ballot (explain.hip: +3 % behind it)
    c.id = __shfl(id, c.src, 64);
    c.rank = __popcll(__ballot(lane < K && comes_before(sk, sid, c.v, c.id)));
    c.enters = c.rank < K;
    return c;
}
// Puts the candidate at its rank; the entries from there on move one lane up and the K-th falls off.
template <typename Pay>
__device__ __forceinline__ void list_place(const ListCand<Pay>& c, int K, int lane, float& sk, int& sid, Pay& sp) {
    const float uk = __shfl_up(sk, 1, 64);
    const Pay up = __shfl_up(sp, 1, 64);                  // key, payload, id: the order explain_topk_kernel was measured with
    const int ui = __shfl_up(sid, 1, 64);
    if (lane < K) {
        if (lane > c.rank) { sk = uk; sid = ui; sp = up; }
        else if (lane == c.rank) { sk = c.v; sid = c.id; sp = c.pay; }
    }
}
// The pair that comes before the other 63 of the wave's (v, id), to every lane.
__device__ __forceinline__ void wave_first(float& v, int& id) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(id, o, 64);
        if (comes_before(ov, oi, v, id)) { v = ov; id = oi; }
    }
}

// ---- rank by counting ----------------------------------------------------------------------------------------------------------------
// Number of entries of keys[0 .. n) (LDS; every lane reads the same address: a broadcast) that come before entry i: a larger key, or the
// same key at a smaller index.  Key: float or unsigned long long.
template <typename Key>
__device__ __forceinline__ int count_before(const Key* keys, int n, int i) {
    const Key mine = keys[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
        const Key kj = keys[j];
        rank += (kj > mine) || (kj == mine && j < i);     // comes_before, written out: through the call cell_order_kernel measured +1.5 %
    }
    return rank;
}
// The k best of vals[0 .. n), n <= 256 (LDS, written and synchronised by the caller): sel[i] = 1 for them, 0 for the others, and their
// indices ascending in idx_row[0 .. k).  All threads of the workgroup call; sel is complete for every thread on return.
__device__ __forceinline__ void select_topk_ascending(const float* vals, int* sel, int n, int k, int* idx_row) {
    const int tid = threadIdx.x;
    if (tid < n) sel[tid] = count_before(vals, n, tid) < k;
    __syncthreads();
    if (tid < n && sel[tid]) {
        int pos = 0;
        for (int j = 0; j < tid; ++j) pos += sel[j];
        idx_row[pos] = tid;
    }
}

// ---- one pass of an 8-bit radix select ---------------------------------------------------------------------------------------------------
// hist: HC replicas of 256 bins, RADIX_HSTRIDE apart (odd: the replicas of one bin fall on different LDS banks), so that keys which cluster
// in two or three bins do not serialise on one LDS atomic; misc: 16 words.  A pass is radix_clear, the kernel's own feed into
// hist[radix_replica<HC>() + digit] (made visible by a barrier), radix_close.  All threads of a workgroup of >= 256 threads call these.
constexpr int RADIX_HSTRIDE = 257;
template <int HC>
__device__ __forceinline__ void radix_clear(uint32_t* hist, int nthreads) {
    for (int i = threadIdx.x; i < HC * RADIX_HSTRIDE; i += nthreads) hist[i] = 0;
    __syncthreads();
}
template <int HC>
__device__ __forceinline__ int radix_replica() { return (threadIdx.x & (HC - 1)) * RADIX_HSTRIDE; }
// Merges the replicas, scans the 256 bins inclusively (one bin per thread of the first four waves: shuffles inside a wave, wave totals
// through misc[0 .. 3]) and locates the bin that holds the 1-based rank `remaining`: its digit is appended to `prefix`, `remaining` becomes
// the rank among the bin's own keys, whose count is returned.  Two barriers, none behind the closing reads of misc[8 .. 10].  Contract on
// the caller: after the call no thread writes misc[8 .. 10] before it has passed a barrier -- another thread may still be reading them
// (hist and misc[0 .. 3] are read in front of the second barrier and are free; radix_clear ends with a barrier, so a next pass is safe).
// act_order_stats_kernel (interp.hip) closes its passes with its own copy of this step: see the measured reason there.
template <int HC>
__device__ __forceinline__ uint32_t radix_close(const uint32_t* hist, uint32_t* misc, uint32_t& prefix, int& remaining) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool scans = threadIdx.x < 256;                 // the barriers and the misc reads stay outside this branch: all threads reach them
    uint32_t cnt = 0, cum = 0;
    if (scans) {
#pragma unroll
        for (int c = 0; c < HC; ++c) cnt += hist[c * RADIX_HSTRIDE + threadIdx.x];
        cum = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t nb = __shfl_up(cum, o, 64);
            if (lane >= o) cum += nb;
        }
        if (lane == 63) misc[wave] = cum;
    }
    __syncthreads();
    if (scans) {
        for (int w = 0; w < wave; ++w) cum += misc[w];
        const uint32_t before = cum - cnt;
        if ((uint32_t)remaining > before && (uint32_t)remaining <= cum) { misc[8] = threadIdx.x; misc[9] = before; misc[10] = cnt; }
    }
    __syncthreads();
    prefix = (prefix << 8) | misc[8];
    remaining -= (int)misc[9];
    return misc[10];
}
