// Host check of the LDS-DMA piece mapping of wgrad8_kernel (protopformer_amd/csrc/gemm_layout.h); built and run by
// tests/test_wgrad_dma_layout_cpu.py with the host compiler (no HIP, no GPU).
//   1. For both tile widths the 1 KiB pieces land every 16-byte chunk exactly where lds_off_mode1<ROWS> expects (kc, col .. col + 7), every
//      chunk of the image is written exactly once, and pieces b / b + 8 are whole rows apart with the same columns (the kernel keeps one
//      source offset per operand and steps wave-uniform pointers by that distance).
//   2. For the shapes of tests/test_gpu_wgrad_dma.py -- every tile, every K slice, every K tile, every piece and lane, walked the way the
//      kernel walks them -- each 16 source bytes lie inside their operand and in the row / column group the image position stands for (or the
//      clamped last group past the edge), and each destination inside the 96 KiB ring.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gemm_layout.h"

using namespace ppfg;

static int failures = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            if (++failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                     \
    } while (0)

template <int ROWS>
static void check_image() {
    constexpr int NP = ROWS / 8, BYTES = ROWS * BK * 2;
    std::vector<int> written(BYTES / 16, 0);
    for (int piece = 0; piece < NP; ++piece)
        for (int lane = 0; lane < 64; ++lane) {
            const DmaPiece pc = wgrad_dma_piece<ROWS>(piece, lane);
            CHECK(pc.lds == piece * 1024 + lane * 16, "ROWS %d piece %d lane %d: image is not lane-linear", ROWS, piece, lane);
            CHECK(pc.kc >= 0 && pc.kc < BK && pc.col >= 0 && pc.col + 8 <= ROWS && pc.col % 8 == 0, "ROWS %d piece %d lane %d: (kc %d, col %d)", ROWS, piece, lane, pc.kc, pc.col);
            for (int e = 0; e < 8; ++e)                          // every element of the chunk, not only its first
                CHECK(lds_off_mode1<ROWS>(pc.kc, pc.col + e) == pc.lds + 2 * e, "ROWS %d piece %d lane %d: column %d belongs at %d, DMA writes %d", ROWS,
                      piece, lane, pc.col + e, lds_off_mode1<ROWS>(pc.kc, pc.col + e), pc.lds + 2 * e);
            ++written[pc.lds / 16];
            if (piece + 8 < NP) {
                const DmaPiece nx = wgrad_dma_piece<ROWS>(piece + 8, lane);
                CHECK(nx.col == pc.col && nx.kc == pc.kc + 4096 / ROWS, "ROWS %d piece %d lane %d: piece + 8 is not %d rows down", ROWS, piece, lane, 4096 / ROWS);
            }
        }
    for (int kc = 0; kc < BK; ++kc)                              // the other direction: every (kc, col) the fragments read was filled once
        for (int col = 0; col < ROWS; col += 8) CHECK(written[lds_off_mode1<ROWS>(kc, col) / 16] == 1, "ROWS %d (kc %d, col %d) written %d times", ROWS, kc, col, written[lds_off_mode1<ROWS>(kc, col) / 16]);
}

// One operand of one workgroup, walked as the kernel does: source offset of piece 0 .. 7 per lane, + (4096 / ROWS) rows per further piece, + 64 rows per K tile.
template <int ROWS>
static void check_operand(const char* what, int R, int K, int ld, int row0, int kbeg, int nk, int image_base) {
    const long long extent = (long long)(K - 1) * ld + R;        // elements of X[kc * ld + r], kc < K, r < R
    for (int wave = 0; wave < 8; ++wave)
        for (int lane = 0; lane < 64; ++lane) {
            const DmaPiece p0 = wgrad_dma_piece<ROWS>(wave, lane);
            const long long off = (long long)wgrad_dma_src(p0, 0, ld, row0, R);
            for (int kt = 0; kt < nk; ++kt)
                for (int i = 0; i < ROWS / 64; ++i) {
                    const long long src = (long long)kbeg * ld + (long long)kt * BK * ld + (long long)i * (4096 / ROWS) * ld + off;
                    CHECK(src >= 0 && src + 8 <= extent && src % 8 == 0, "%s: source [%lld, +8) outside the operand of %lld elements", what, src, extent);
                    const DmaPiece pc = wgrad_dma_piece<ROWS>(wave + 8 * i, lane);
                    const long long want_row = kbeg + kt * BK + pc.kc, want_col = row0 + pc.col < R - 8 ? row0 + pc.col : R - 8;
                    CHECK(src == want_row * ld + want_col, "%s: piece %d lane %d tile %d reads %lld, its image position stands for %lld", what, wave + 8 * i, lane, kt,
                          src, want_row * ld + want_col);
                    for (int slot = 0; slot < 2; ++slot) {
                        const int dst = slot * WG8_SLOT_BYTES + image_base + pc.lds;
                        CHECK(dst >= 0 && dst + 16 <= WG8_RING_BYTES, "%s: destination %d outside the ring", what, dst);
                    }
                }
        }
}

template <int WMW, int WNW>
static void check_shape(int M, int N, int K) {
    constexpr int TBM = 64 * WMW, TBN = 64 * WNW;
    if (K % BK != 0) return;                                     // falls back to the register-staged kernel
    const int ns = pick_splitk(M, N, K);
    long long tiles_k = 0;
    for (int z = 0; z < ns; ++z) {
        const KSlice ks = k_slice(K, ns, z);
        CHECK(ks.kbeg < ks.kend && ks.kbeg % BK == 0 && ks.kend % BK == 0, "M %d N %d K %d slice %d: [%d, %d) is not whole K tiles", M, N, K, z, ks.kbeg, ks.kend);
        const int nk = (ks.kend - ks.kbeg + BK - 1) / BK;
        tiles_k += nk;
        for (int m0 = 0; m0 < M; m0 += TBM) check_operand<TBM>("A", M, K, M, m0, ks.kbeg, nk, 0);
        for (int n0 = 0; n0 < N; n0 += TBN) check_operand<TBN>("B", N, K, N, n0, ks.kbeg, nk, TBM * BK * 2);
    }
    CHECK(tiles_k * BK == K, "M %d N %d K %d: the slices cover %lld of %d K tiles", M, N, K, tiles_k, K / BK);
    std::printf("shape %4d x %4d, K %4d: %d slices, %lld K tiles checked\n", M, N, K, ns, tiles_k);
}

// 3. The K slicing every split-K kernel relies on: for ns = pick_splitk(M, N, K) the slices k_slice(K, ns, z), z < ns, are non-empty, start on
//    multiples of 64, follow each other without gap or overlap and end at K -- for the (M, N) of every split-K case of
//    tests/test_gpu_gemm_paths.py and K = 8 .. 4096 in steps of 8 (a partial-tile slab that is never written would be read by the reduce).
static void check_slices() {
    static const int mn[][2] = {{192, 192}, {136, 72}, {136, 200}, {512, 320}, {1032, 328}, {320, 512}, {328, 1032},
                                {1, 8}, {33, 132}, {130, 260}, {257, 128}, {16261, 520}, {16261, 516}, {16384, 512}, {225, 136}, {449, 392},
                                {33, 136}, {130, 264}, {264, 136}};
    long long slices = 0;
    for (const auto& s : mn)
        for (int K = 8; K <= 4096; K += 8) {
            const int M = s[0], N = s[1], ns = pick_splitk(M, N, K);
            CHECK(ns >= 1 && ns <= (K + BK - 1) / BK, "M %d N %d K %d: %d slices", M, N, K, ns);
            int next = 0;
            for (int z = 0; z < ns; ++z) {
                const KSlice ks = k_slice(K, ns, z);
                CHECK(ks.kbeg == next && ks.kbeg % BK == 0, "M %d N %d K %d slice %d of %d starts at %d, the one before ended at %d", M, N, K, z, ns, ks.kbeg, next);
                CHECK(ks.kend > ks.kbeg && ks.kend <= K, "M %d N %d K %d slice %d of %d: [%d, %d) is empty or past K", M, N, K, z, ns, ks.kbeg, ks.kend);
                next = ks.kend;
                ++slices;
            }
            CHECK(next == K, "M %d N %d K %d: %d slices end at %d", M, N, K, ns, next);
        }
    // the slice counts the GPU tests' cases are built around
    CHECK(pick_splitk(192, 192, 520) == 3 && pick_splitk(136, 72, 200) == 1 && pick_splitk(136, 200, 264) == 2, "slice counts of the 128 x 128 split-K cases");
    CHECK(pick_splitk(512, 320, 512) == 2 && pick_splitk(1032, 328, 520) == 3 && pick_splitk(320, 512, 264) == 2, "slice counts of the eight-wave cases");
    const KSlice last = k_slice(520, 3, 2);
    CHECK(last.kbeg == 384 && last.kend == 520, "K = 520 in three slices: 192 / 192 / 136");
    std::printf("K slicing: %lld slices checked\n", slices);
}

int main() {
    check_slices();
    static_assert((256 + 128) * BK * 2 == WG8_SLOT_BYTES && 2 * WG8_SLOT_BYTES == 96 * 1024, "ring budget");
    check_image<256>();
    check_image<128>();
    // n_out x n_in, rows of tests/test_gpu_wgrad_dma.py (M = n_out, N = n_in, K = rows; lda = M, ldb = N)
    check_shape<4, 2>(512, 384, 1024);
    check_shape<4, 2>(1152, 384, 832);
    check_shape<2, 4>(384, 1536, 1024);
    check_shape<2, 4>(400, 1288, 960);
    check_shape<4, 2>(1152, 384, 840);
    CHECK(pick_splitk(512, 384, 1024) == 4 && pick_splitk(1152, 384, 832) == 4, "slice counts the GPU test's cases are built around");
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("wgrad DMA layout: ok\n");
    return 0;
}
