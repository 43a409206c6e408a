// PartsWorld: a data set the library renders itself, so that a model can be trained and every interpretability tool run end to end with
// annotations that are true by construction (the idea of FunnyBirds, Hesse et al., ICCV 2023, at this code base's size).  A class is a
// row of part attributes; an image is an object body with its parts on fixed slots, a few distractor shapes, a smooth background and
// pixel noise.  The contract is in include/ppf_hip.h and the shared arithmetic in synth_plan.h: integers only, Philox4x32-10 keyed by
// (seed, image id, item), so the kernels and the numpy referees (data.partsworld_*) agree bit for bit.  The reference has no such pass.
//   * synth_scene_kernel: one lane per image; about ninety Philox calls and a few dozen words.  Not tuned.
//   * synth_render_kernel: write-bound.  A workgroup lies inside one image and stages that image's scene row in LDS, so every primitive
//     test reads workgroup-uniform words and the primitive loops have the trip counts of the launch (D, K), not of the lane.  A lane owns
//     16 consecutive pixels of a row: 48 bytes written as three 16-byte stores (byte stores made the table and colour passes of
//     device_data.hip 3.5 x a copy), the partmap as one 16-byte store.  Painter's order: background, distractors, body, parts, then noise.
//   * synth_edit_kernel: the interventions.  One workgroup per (image, edit), one lane per word of the row; the rule is synth_plan.h's.
#include <limits.h>

#include "ppf_common.h"
#include "ppf_hip.h"
#include "synth_plan.h"

static_assert(SYNTH_WORDS == PPF_SYNTH_WORDS, "synth_plan.h and ppf_hip.h disagree about the scene table");
static_assert(SYNTH_NODE0 + SYNTH_MAX_NODES <= SYNTH_WORDS && SYNTH_WORDS % 4 == 0, "the scene row holds every node and is 16-byte sized");

namespace {

constexpr int NT_SYNTH = 256;
constexpr int SYNTH_PX = 16;                                                  // pixels per lane

__device__ __forceinline__ uint4 synth_draw(uint32_t item, uint32_t stream, uint64_t id, uint64_t seed) {
    return philox4x32_10(make_uint4(item, stream, (uint32_t)id, (uint32_t)(id >> 32)), make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
}

__global__ __launch_bounds__(NT_SYNTH) void synth_scene_kernel(int* __restrict__ scene, const long long* __restrict__ ids, int B, int C, int K, int D,
                                                               int H, int W, int g, uint64_t seed) {
    const int b = blockIdx.x * NT_SYNTH + threadIdx.x;
    if (b >= B) return;
    const uint64_t id = (uint64_t)ids[b];
    int* __restrict__ row = scene + (size_t)b * SYNTH_WORDS;
    for (int e = 0; e < SYNTH_WORDS; ++e) row[e] = 0;
    row[SYNTH_LABEL] = (int)(id % (uint64_t)C);
    const int label = row[SYNTH_LABEL];
    const uint4 wo = synth_draw(SYNTH_ITEM_OBJECT, SYNTH_STREAM_SCENE, id, seed);
    const SynthObject o = synth_object(wo.x >> 8, wo.y >> 8, wo.z >> 8, H, W);
    row[SYNTH_BOX + 0] = o.ox - o.hs;
    row[SYNTH_BOX + 1] = o.oy - o.hs;
    row[SYNTH_BOX + 2] = o.ox + o.hs + 1;
    row[SYNTH_BOX + 3] = o.oy + o.hs + 1;
    const int forced = synth_range(wo.w >> 8, K);
    for (int k = 0; k < K; ++k) {
        const uint4 w = synth_draw(SYNTH_ITEM_PART0 + k, SYNTH_STREAM_SCENE, id, seed);
        int* __restrict__ p = row + SYNTH_PART0 + SYNTH_PRIM_WORDS * k;
        p[SYNTH_ON] = ((w.x >> 8) < SYNTH_VISIBLE_THR || k == forced) ? 1 : 0;
        synth_part(k, o, w.y >> 8, w.z >> 8, p + SYNTH_CX, p + SYNTH_CY, p + SYNTH_R);
        p[SYNTH_ATTR] = synth_class_part(label, k);
    }
    for (int d = 0; d < D; ++d) {
        const uint4 w0 = synth_draw(SYNTH_ITEM_DIST0 + 2 * d, SYNTH_STREAM_SCENE, id, seed);
        const uint4 w1 = synth_draw(SYNTH_ITEM_DIST0 + 2 * d + 1, SYNTH_STREAM_SCENE, id, seed);
        int* __restrict__ p = row + SYNTH_DIST0 + SYNTH_PRIM_WORDS * d;
        p[SYNTH_ON] = (w0.x >> 8) < SYNTH_DISTRACTOR_THR ? 1 : 0;
        p[SYNTH_ATTR] = synth_range(w0.y >> 8, SYNTH_ATTRS);
        synth_distractor(w0.z >> 8, w1.x >> 8, w1.y >> 8, H, W, p + SYNTH_CX, p + SYNTH_CY, p + SYNTH_R);
    }
    const int draws = 3 * (g + 1) * (g + 1);
    for (int c4 = 0; 4 * c4 < draws; ++c4) {
        const uint4 w = synth_draw(SYNTH_ITEM_NODE0 + c4, SYNTH_STREAM_SCENE, id, seed);
        const uint32_t word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = 4 * c4 + i;
            if (e < draws) row[SYNTH_NODE0 + e / 3] |= (SYNTH_NODE_LOW + synth_range(word[i] >> 8, SYNTH_NODE_SPAN)) << (8 * (e % 3));
        }
    }
}

// Paints one primitive over the lane's 16 pixels: row y, columns x0 .. x0 + 15.
__device__ __forceinline__ void synth_paint(const int* prim, int code, int y, int x0, int (&rgb)[SYNTH_PX], int (&top)[SYNTH_PX]) {
    if (!prim[SYNTH_ON]) return;
    const int r = prim[SYNTH_R], dy = y - prim[SYNTH_CY], dx0 = x0 - prim[SYNTH_CX];
    if (dy > r || -dy > r || dx0 > r || dx0 + SYNTH_PX - 1 < -r) return;
    const int shape = synth_shape_of(prim[SYNTH_ATTR]), colour = synth_palette(synth_colour_of(prim[SYNTH_ATTR]));
#pragma unroll
    for (int e = 0; e < SYNTH_PX; ++e) {
        if (synth_inside(shape, dx0 + e, dy, r)) { rgb[e] = colour; top[e] = code; }
    }
}

// grid: B * blocks_per_img workgroups; a lane owns pixels (y, x0 .. x0 + 15) of image b
__global__ __launch_bounds__(NT_SYNTH) void synth_render_kernel(uint4* __restrict__ out, uint4* __restrict__ partmap, const int* __restrict__ scene,
                                                                const long long* __restrict__ ids, int H, int W, int K, int D, int g, int noise,
                                                                uint64_t seed, int blocks_per_img) {
    __shared__ int sc[SYNTH_WORDS];
    const int b = blockIdx.x / blocks_per_img, blk = blockIdx.x - b * blocks_per_img;
    if (threadIdx.x < SYNTH_WORDS) sc[threadIdx.x] = scene[(size_t)b * SYNTH_WORDS + threadIdx.x];
    __syncthreads();
    const int W16 = W / SYNTH_PX, v = blk * NT_SYNTH + threadIdx.x;
    if (v >= H * W16) return;
    const int y = v / W16, x0 = (v - y * W16) * SYNTH_PX;
    int rgb[SYNTH_PX], top[SYNTH_PX];
    {   // 1. the background
        const int ch = synth_cell(H, g), cw = synth_cell(W, g), L = g + 1;
        const int i = y / ch, ry = y - i * ch;
        int j = x0 / cw, rx = x0 - j * cw;
#ifdef PPF_SYNTH_KNOCKOUT                                                     // measurement build of scripts/bench_partsworld.py: a flat background
#pragma unroll
        for (int e = 0; e < SYNTH_PX; ++e) { rgb[e] = sc[SYNTH_NODE0]; top[e] = SYNTH_CODE_BG; }
        (void)i; (void)ry; (void)j; (void)rx; (void)L;
#else
#pragma unroll
        for (int e = 0; e < SYNTH_PX; ++e) {
            const int n00 = sc[SYNTH_NODE0 + i * L + j], n01 = sc[SYNTH_NODE0 + i * L + j + 1];
            const int n10 = sc[SYNTH_NODE0 + (i + 1) * L + j], n11 = sc[SYNTH_NODE0 + (i + 1) * L + j + 1];
            int px = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                px |= synth_blend((n00 >> (8 * c)) & 255, (n01 >> (8 * c)) & 255, (n10 >> (8 * c)) & 255, (n11 >> (8 * c)) & 255, ry, rx, ch, cw) << (8 * c);
            rgb[e] = px;
            top[e] = SYNTH_CODE_BG;
            if (++rx == cw) { rx = 0; ++j; }
        }
#endif
    }
#ifndef PPF_SYNTH_KNOCKOUT
    for (int d = 0; d < D; ++d) synth_paint(sc + SYNTH_DIST0 + SYNTH_PRIM_WORDS * d, SYNTH_CODE_DISTRACTOR, y, x0, rgb, top);     // 2.
    if (y >= sc[SYNTH_BOX + 1] && y < sc[SYNTH_BOX + 3]) {                                                                         // 3. the body
#pragma unroll
        for (int e = 0; e < SYNTH_PX; ++e)
            if (x0 + e >= sc[SYNTH_BOX] && x0 + e < sc[SYNTH_BOX + 2]) { rgb[e] = SYNTH_BODY_RGB; top[e] = SYNTH_CODE_BODY; }
    }
    for (int k = 0; k < K; ++k) synth_paint(sc + SYNTH_PART0 + SYNTH_PRIM_WORDS * k, SYNTH_CODE_PART0 + k, y, x0, rgb, top);       // 4.
#endif
    if (noise > 0) {                                                          // workgroup-uniform
        const uint64_t id = (uint64_t)ids[b];
        const int span = 2 * noise + 1;
#pragma unroll
        for (int e = 0; e < SYNTH_PX; ++e) {
            const uint4 w = synth_draw((uint32_t)(y * W + x0 + e), SYNTH_STREAM_NOISE, id, seed);
            const uint32_t word[3] = {w.x, w.y, w.z};
            int px = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int val = ((rgb[e] >> (8 * c)) & 255) + synth_range(word[c] >> 8, span) - noise;
                px |= min(max(val, 0), 255) << (8 * c);
            }
            rgb[e] = px;
        }
    }
    // 16 pixels x 3 bytes = 12 words: byte q of the run is channel q % 3 of pixel q / 3
    uint32_t wd[12];
#pragma unroll
    for (int q4 = 0; q4 < 12; ++q4) {
        uint32_t word = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = 4 * q4 + i;
            word |= (uint32_t)((rgb[q / 3] >> (8 * (q % 3))) & 255) << (8 * i);
        }
        wd[q4] = word;
    }
    uint4* __restrict__ o = out + ((size_t)b * H * W16 + v) * 3;
    o[0] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    o[1] = make_uint4(wd[4], wd[5], wd[6], wd[7]);
    o[2] = make_uint4(wd[8], wd[9], wd[10], wd[11]);
    if (partmap) {
        uint32_t pm[4];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
            pm[q4] = (uint32_t)top[4 * q4] | (uint32_t)top[4 * q4 + 1] << 8 | (uint32_t)top[4 * q4 + 2] << 16 | (uint32_t)top[4 * q4 + 3] << 24;
        partmap[(size_t)b * H * W16 + v] = make_uint4(pm[0], pm[1], pm[2], pm[3]);
    }
}

// grid: B * E workgroups of NT_SYNTH threads, one per (image, edit); lane w < SYNTH_WORDS owns word w of the edited row.  The row is staged
// in LDS because the rule reads the primitive's on-word next to the word it edits.  Latency-bound and not tuned.
__global__ __launch_bounds__(NT_SYNTH) void synth_edit_kernel(int* __restrict__ out, int* __restrict__ changed, const int* __restrict__ scene,
                                                              const int* __restrict__ edits, int E, int K, int D, int g) {
    __shared__ int sc[SYNTH_WORDS];
    const int be = blockIdx.x, b = be / E, w = threadIdx.x;
    if (w < SYNTH_WORDS) sc[w] = scene[(size_t)b * SYNTH_WORDS + w];
    const int op = edits[2 * (size_t)be], arg = edits[2 * (size_t)be + 1];
    __syncthreads();
    const bool valid = synth_edit_valid(op, arg, K, D);
    int differs = 0;
    if (w < SYNTH_WORDS) {
        const int v = valid ? synth_edit_word(sc, w, op, arg, K, D, g) : sc[w];
        out[(size_t)be * SYNTH_WORDS + w] = v;
        differs = v != sc[w] && synth_edit_live(sc, w, op, arg, K, D, g);
    }
    const int any = __syncthreads_or(differs);
    if (w == 0) changed[be] = valid ? (any ? 1 : 0) : -1;
}

// The spec words both entry points take, refused by name before any device call.
int synth_check(const char* who, int B, int C, int K, int D, int H, int W, int g, int noise) {
    PPF_CHECK_ARG(B >= 1, PPF_ERR_SHAPE, "%s: B=%d (>= 1)", who, B);
    switch (synth_spec_fault(C, K, D, H, W, g, noise)) {
        case 0: return 0;
        case 1: ppf_set_error("%s: K=%d parts per object outside [1, %d]", who, K, SYNTH_MAX_PARTS); break;
        case 2: ppf_set_error("%s: D=%d distractors outside [0, %d]", who, D, SYNTH_MAX_DISTRACTORS); break;
        case 3: ppf_set_error("%s: C=%d classes outside [2, %d]", who, C, SYNTH_MAX_CLASSES); break;
        case 4: ppf_set_error("%s: C=%d classes exceed A^K = %lld rows of K=%d attributes (C > A^K)", who, C, (long long)synth_class_limit(K), K); break;
        case 5: ppf_set_error("%s: H=%d outside [%d, %d]", who, H, SYNTH_MIN_SIDE, SYNTH_MAX_SIDE); break;
        case 6: ppf_set_error("%s: W=%d outside [%d, %d]", who, W, SYNTH_MIN_SIDE, SYNTH_MAX_SIDE); break;
        case 7: ppf_set_error("%s: W=%d is not a multiple of 16 (W %% 16: a lane writes 16 pixels as 16-byte stores)", who, W); break;
        case 8: ppf_set_error("%s: g=%d background cells per side outside [1, %d]", who, g, SYNTH_MAX_GRID); break;
        default: ppf_set_error("%s: noise=%d amplitude outside [0, %d]", who, noise, SYNTH_MAX_NOISE); break;
    }
    return PPF_ERR_SHAPE;
}

}  // namespace

extern "C" {

int ppf_synth_scene(int* scene, const void* ids_i64, int B, int C, int K, int D, int H, int W, int g, int noise, uint64_t seed, hipStream_t stream) {
    if (int rc = synth_check("ppf_synth_scene", B, C, K, D, H, W, g, noise)) return rc;
    PPF_CHECK_ARG(scene && ids_i64, PPF_ERR_ARG, "ppf_synth_scene: null pointer (scene, ids)");
    return ppf_launch<synth_scene_kernel>(dim3((unsigned)((B + NT_SYNTH - 1) / NT_SYNTH)), dim3(NT_SYNTH), 0, stream, "ppf_synth_scene", scene,
                                          (const long long*)ids_i64, B, C, K, D, H, W, g, seed);
}

int ppf_synth_render(void* out_u8, void* partmap_u8, const int* scene, const void* ids_i64, int B, int H, int W, int C, int K, int D, int g, int noise,
                     uint64_t seed, hipStream_t stream) {
    if (int rc = synth_check("ppf_synth_render", B, C, K, D, H, W, g, noise)) return rc;
    PPF_CHECK_ARG((((uintptr_t)out_u8 | (uintptr_t)partmap_u8) & 15) == 0, PPF_ERR_SHAPE,
                  "ppf_synth_render: out and partmap must be 16-byte aligned (16-byte stores)");
    PPF_CHECK_ARG(out_u8 && scene && ids_i64, PPF_ERR_ARG, "ppf_synth_render: null pointer (only partmap may be NULL)");
    const int blocks_per_img = (H * (W / SYNTH_PX) + NT_SYNTH - 1) / NT_SYNTH;                    // <= 256
    PPF_CHECK_ARG((long long)B * blocks_per_img <= INT_MAX, PPF_ERR_SHAPE, "ppf_synth_render: B=%d x H=%d x W=%d exceeds the grid", B, H, W);
    return ppf_launch<synth_render_kernel>(dim3((unsigned)(B * blocks_per_img)), dim3(NT_SYNTH), 0, stream, "ppf_synth_render", (uint4*)out_u8,
                                           (uint4*)partmap_u8, scene, (const long long*)ids_i64, H, W, K, D, g, noise, seed, blocks_per_img);
}

int ppf_synth_edit(int* out, int* changed, const int* scene, const int* edits, int B, int E, int C, int K, int D, int g, hipStream_t stream) {
    if (int rc = synth_check("ppf_synth_edit", B, C, K, D, SYNTH_MIN_SIDE, SYNTH_MIN_SIDE, g, 0)) return rc;   // the frame and the noise are not an edit's business
    PPF_CHECK_ARG(E >= 1, PPF_ERR_SHAPE, "ppf_synth_edit: E=%d edits per image (>= 1)", E);
    PPF_CHECK_ARG((long long)B * E <= INT_MAX / SYNTH_WORDS, PPF_ERR_SHAPE, "ppf_synth_edit: B=%d x E=%d rows exceed the grid", B, E);
    PPF_CHECK_ARG(out && changed && scene && edits, PPF_ERR_ARG, "ppf_synth_edit: null pointer (out, changed, scene, edits)");
    return ppf_launch<synth_edit_kernel>(dim3((unsigned)(B * E)), dim3(NT_SYNTH), 0, stream, "ppf_synth_edit", out, changed, scene, edits, E, K, D, g);
}

}  // extern "C"
