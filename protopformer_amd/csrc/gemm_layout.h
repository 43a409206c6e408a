// Index arithmetic of the bf16 GEMM family (gemm_bf16.hip) that a host program can check without a GPU: the transposed-tile LDS layout,
// the split-K slicing and the piece mapping of the weight-gradient kernel's LDS-DMA path.  No HIP header is needed to include this file;
// tests/wgrad_dma_layout_check.cpp compiles it with the host compiler.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define PPF_HD __host__ __device__ __forceinline__
#else
#define PPF_HD inline
#endif

namespace ppfg {

constexpr int BK = 64;                           // contraction values per K tile

// transposed tile [64 kc][ROWS r]: row pitch ROWS*2 bytes, 64-byte units XOR-swizzled by kc&3 inside each 256-byte group
template <int ROWS>
PPF_HD int lds_off_mode1(int kc, int col) {
    return kc * (ROWS * 2) + ((((col >> 5) ^ (kc & 3))) << 6) + ((col & 31) << 1);
}

// Contraction range [kbeg, kend) of K slice `zslice` of `nsplit`: multiples of BK except the tail; kbeg >= kend: an empty slice.  The K-tile
// count is left to the caller, after its empty-slice return: computed in front of that return the kernels come out 5 % longer.
struct KSlice { int kbeg, kend; };
PPF_HD KSlice k_slice(int K, int nsplit, int zslice) {
    const int kchunk = (((K + nsplit - 1) / nsplit) + BK - 1) / BK * BK;
    const int kbeg = zslice * kchunk;
    return {kbeg, K < kbeg + kchunk ? K : kbeg + kchunk};
}

// K slices of a weight-gradient-style problem (small output, very long contraction).
#ifndef PPF_WGRAD_SPLITK_TARGET
#define PPF_WGRAD_SPLITK_TARGET 432                // workgroup slots aimed at (a measurement build can set another for a same-box A/B)
#endif
inline int pick_splitk(int M, int N, int K) {
    const int tiles = ((M + 127) / 128) * ((N + 127) / 128);         // in 128 x 128 tiles, whichever kernel runs
    // K slices: alone on the GPU the kernel is fastest with as many slices as fit in ONE round of 3 workgroups per CU (768:
    // -17 % vs 540; one slice more spills into a second round and gives it all back).  In the train step these GEMMs run on
    // the side stream under the dgrad chain, where a smaller footprint wins (step time: 432 <= 540 < 768), so that is the default.
    // Narrow layers (an output side <= 256: the D = 192 models) take half as many: their reduce kernel reads every slab back and is a
    // third of the side stream's time there (216: deit_tiny +1.5 %, cait_xxs24 +2.9 % same-box; 144: -2 %; at D = 384 288: -4 %).
    const int target = (M < N ? M : N) <= 256 ? 216 : PPF_WGRAD_SPLITK_TARGET;
    int s = target / tiles;
    const int maxs = (K + 4 * BK - 1) / (4 * BK);      // at least 4 K-tiles per slice
    if (s > maxs) s = maxs;
    if (s < 1) s = 1;
    // slices are BK-aligned chunks: drop the ones that would be empty (a partial-tile slice must always be written)
    const int kchunk = (((K + s - 1) / s) + BK - 1) / BK * BK;
    return (K + kchunk - 1) / kchunk;
}

// ---- LDS-DMA fill of a transposed K tile (wgrad8_kernel's DMA path) ----------------------------------------------------------------
// One global_load_lds_dwordx4 writes 1 KiB of LDS lane-linearly (wave-uniform base + 16 * lane), so the [64 kc][ROWS] image is cut into
// ROWS / 8 pieces of 1 KiB: two kc rows of a 256-row operand, four of a 128-row one.  The swizzle of lds_off_mode1 goes on the SOURCE side:
// lane l of piece p fills LDS bytes [1024 p + 16 l, + 16), which lds_off_mode1<ROWS> assigns to row kc and the eight columns col ..
// col + 7 of the tile (the XOR permutes 64-byte units inside one kc row: source and destination stay in the same global row).
constexpr int WG8_SLOT_BYTES = (256 + 128) * BK * 2;     // both operand images of one K tile: 48 KiB
constexpr int WG8_RING_BYTES = 2 * WG8_SLOT_BYTES;       // two slots: 96 KiB
struct DmaPiece { int kc, col, lds; };                   // tile row, first tile column, byte offset inside the operand image
template <int ROWS>
PPF_HD DmaPiece wgrad_dma_piece(int piece, int lane) {
    const int lds = piece * 1024 + lane * 16;
    const int kc = lds / (ROWS * 2), w = lds % (ROWS * 2);
    return {kc, ((((w >> 6) ^ (kc & 3))) << 5) + ((w & 63) >> 1), lds};
}
// Element offset of that 16-byte chunk in an operand X(r, kc) = X[kc * ld + r] of R rows (R % 8 == 0) for the K tile starting at k0 and the
// tile rows row0 ..: column groups past the edge re-read the last valid group (LDS-DMA cannot zero-fill; the epilogue's masks drop them).
PPF_HD size_t wgrad_dma_src(const DmaPiece& pc, int k0, int ld, int row0, int R) {
    const int c = row0 + pc.col;
    return (size_t)(k0 + pc.kc) * (size_t)ld + (size_t)(c < R - 8 ? c : R - 8);
}

}  // namespace ppfg
