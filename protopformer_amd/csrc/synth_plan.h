// What the PartsWorld kernels (synth.hip; the contract is in include/ppf_hip.h) and the host share, as arithmetic that a host program can
// check without a GPU: the word layout of the scene table, the Philox streams and items, the class-table rule, the object's size and
// place from its draws, the slot layout of the parts, the distractors, the background cells and the integer membership test of the four
// shapes.  No HIP header is needed to include this file; tests/synth_plan_check.cpp compiles it with the host compiler.
#pragma once
#include <stdint.h>

#ifndef PPF_HD
#if defined(__HIPCC__)                                                        // the same definition as order_keys.h's
#define PPF_HD __host__ __device__ __forceinline__
#else
#define PPF_HD inline
#endif
#endif

constexpr int SYNTH_SHAPES = 4, SYNTH_COLOURS = 6, SYNTH_ATTRS = SYNTH_SHAPES * SYNTH_COLOURS;   // attribute = shape * 6 + colour
constexpr int SYNTH_DISK = 0, SYNTH_SQUARE = 1, SYNTH_DIAMOND = 2, SYNTH_RING = 3;
constexpr int SYNTH_MAX_CLASSES = 1024, SYNTH_MAX_PARTS = 8, SYNTH_MAX_DISTRACTORS = 8, SYNTH_MAX_GRID = 8, SYNTH_MAX_NOISE = 32;
constexpr int SYNTH_MAX_NODES = (SYNTH_MAX_GRID + 1) * (SYNTH_MAX_GRID + 1);                     // 81
constexpr int SYNTH_MIN_SIDE = 32, SYNTH_MAX_SIDE = 1024;

// the scene table: int32 [B][SYNTH_WORDS]; entries past K parts, D distractors and (g + 1)^2 nodes are zero
constexpr int SYNTH_LABEL = 0, SYNTH_BOX = 1;                                 // box = (x0, y0, x1, y1), x1 and y1 exclusive
constexpr int SYNTH_PRIM_WORDS = 5;                                           // (on, cx, cy, r, attribute) of a part or a distractor
constexpr int SYNTH_ON = 0, SYNTH_CX = 1, SYNTH_CY = 2, SYNTH_R = 3, SYNTH_ATTR = 4;
constexpr int SYNTH_PART0 = SYNTH_BOX + 4;                                    // 5
constexpr int SYNTH_DIST0 = SYNTH_PART0 + SYNTH_PRIM_WORDS * SYNTH_MAX_PARTS; // 45
constexpr int SYNTH_NODE0 = SYNTH_DIST0 + SYNTH_PRIM_WORDS * SYNTH_MAX_DISTRACTORS;              // 85: node colour r | g << 8 | b << 16
constexpr int SYNTH_WORDS = 168;                                              // 85 + 81 = 166, rounded up to a multiple of 4

// the partmap's codes
constexpr int SYNTH_CODE_BG = 0, SYNTH_CODE_DISTRACTOR = 1, SYNTH_CODE_BODY = 2, SYNTH_CODE_PART0 = 3;

// Philox counter word 1 of the two streams, and counter word 0 (the item) inside the scene stream
constexpr uint32_t SYNTH_STREAM_SCENE = 0xC0000001u, SYNTH_STREAM_NOISE = 0xC0000002u;
constexpr uint32_t SYNTH_ITEM_OBJECT = 0;                                     // (half-size, centre x, centre y, the part forced visible)
constexpr uint32_t SYNTH_ITEM_PART0 = 1;                                      // + k: (visible, jitter x, jitter y, -)
constexpr uint32_t SYNTH_ITEM_DIST0 = 9;                                      // + 2d: (on, attribute, radius, -);  + 2d + 1: (centre x, centre y, -, -)
constexpr uint32_t SYNTH_ITEM_NODE0 = 32;                                     // + e / 4, word e % 4: channel e % 3 of node e / 3
constexpr uint32_t SYNTH_VISIBLE_THR = 3u << 22;                              // a part is visible when its draw is below 3/4 * 2^24
constexpr uint32_t SYNTH_DISTRACTOR_THR = 1u << 23;                           // a distractor is on when its draw is below 1/2 * 2^24
constexpr int SYNTH_NODE_LOW = 64, SYNTH_NODE_SPAN = 128;                     // node channels in [64, 192)
constexpr int SYNTH_BODY_RGB = 112 | 112 << 8 | 112 << 16;

// a 24-bit draw u mapped to [0, n): no modulo bias beyond 2^-24 * n
PPF_HD int synth_range(uint32_t u, int n) { return (int)(((uint64_t)u * (uint32_t)n) >> 24); }

// ---- the class table: part k of class c is digit k of c in base A.  Injective for c < A^K, a function of (c, k) alone.
PPF_HD int64_t synth_class_limit(int K) {                                     // min(A^K, 2^31): every class count above it is refused
    int64_t n = 1;
    for (int k = 0; k < K && n < (1LL << 31); ++k) n *= SYNTH_ATTRS;
    return n < (1LL << 31) ? n : (1LL << 31);
}
PPF_HD int synth_class_part(int c, int k) {
    int64_t v = c;
    for (int i = 0; i < k; ++i) v /= SYNTH_ATTRS;
    return (int)(v % SYNTH_ATTRS);
}
PPF_HD int synth_shape_of(int attr) { return (int)((uint32_t)attr % SYNTH_ATTRS) / SYNTH_COLOURS; }
PPF_HD int synth_colour_of(int attr) { return (int)((uint32_t)attr % SYNTH_ATTRS) % SYNTH_COLOURS; }
PPF_HD int synth_palette(int colour) {                                       // r | g << 8 | b << 16
    switch (colour) {
        case 0: return 220 | 40 << 8 | 40 << 16;                              // red
        case 1: return 40 | 180 << 8 | 60 << 16;                              // green
        case 2: return 50 | 80 << 8 | 220 << 16;                              // blue
        case 3: return 235 | 210 << 8 | 40 << 16;                             // yellow
        case 4: return 200 | 60 << 8 | 200 << 16;                             // magenta
        default: return 40 | 200 << 8 | 210 << 16;                            // cyan
    }
}

// ---- the object: a square body of half-size hs around (ox, oy), pixels |x - ox| <= hs and |y - oy| <= hs, inside the frame
struct SynthObject { int hs, ox, oy; };
PPF_HD int synth_hs_min(int m) { return 5 * m / 16; }
PPF_HD int synth_hs_max(int m) { return 13 * m / 32; }                        // 2 * hs_max + 1 <= m for m >= 16
PPF_HD SynthObject synth_object(uint32_t u_hs, uint32_t u_x, uint32_t u_y, int H, int W) {
    const int m = H < W ? H : W;
    SynthObject o;
    o.hs = synth_hs_min(m) + synth_range(u_hs, synth_hs_max(m) - synth_hs_min(m) + 1);
    o.ox = o.hs + synth_range(u_x, W - 2 * o.hs);                             // in [hs, W - 1 - hs]
    o.oy = o.hs + synth_range(u_y, H - 2 * o.hs);
    return o;
}

// ---- the slots: a 3 x 3 grid of cells of pitch p = (2 hs + 1) / 3 around the object's centre, the centre cell left to the body.  A part
// of radius r jittered by at most j per axis stays inside its cell when 2 (r + j) <= p - 1: parts of neighbouring cells are p apart, so
// they are disjoint, and the outermost pixel is p + r + j <= (3 p - 1) / 2 <= hs from the centre, so they are inside the box.
PPF_HD int synth_pitch(int hs) { return (2 * hs + 1) / 3; }
PPF_HD int synth_jitter(int p) { return (p - 1) / 8; }
PPF_HD int synth_part_radius(int p) { return (p - 1) / 2 - synth_jitter(p); }
PPF_HD int synth_slot_cell(int k) { return (int)((0x75318620u >> (4 * k)) & 15u); }              // corners first: 0 2 6 8 1 3 5 7
PPF_HD void synth_part(int k, SynthObject o, uint32_t u_jx, uint32_t u_jy, int* cx, int* cy, int* r) {
    const int p = synth_pitch(o.hs), j = synth_jitter(p), cell = synth_slot_cell(k);
    *cx = o.ox + (cell % 3 - 1) * p + synth_range(u_jx, 2 * j + 1) - j;
    *cy = o.oy + (cell / 3 - 1) * p + synth_range(u_jy, 2 * j + 1) - j;
    *r = synth_part_radius(p);
}

// ---- a distractor: radius in [m / 16, m / 8], the whole shape inside the frame; it may lie under the object
PPF_HD void synth_distractor(uint32_t u_r, uint32_t u_x, uint32_t u_y, int H, int W, int* cx, int* cy, int* r) {
    const int m = H < W ? H : W;
    *r = m / 16 + synth_range(u_r, m / 8 - m / 16 + 1);
    *cx = *r + synth_range(u_x, W - 2 * *r);
    *cy = *r + synth_range(u_y, H - 2 * *r);
}

// ---- membership of the pixel at offset (dx, dy) from the centre of a shape of radius r: integers only; every shape lies inside
// max(|dx|, |dy|) <= r and contains its centre.  The ring is the annulus r / 2 <= d <= r with a centre dot of radius r / 4, told by the
// two squared radii r^2 / 4 and r^2 / 16.
PPF_HD bool synth_inside(int shape, int dx, int dy, int r) {
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    if (ax > r || ay > r) return false;
    const int d2 = ax * ax + ay * ay, r2 = r * r;                             // <= 2^21: sides are at most 1024
    switch (shape) {
        case SYNTH_DISK: return d2 <= r2;
        case SYNTH_SQUARE: return true;
        case SYNTH_DIAMOND: return ax + ay <= r;
        default: return d2 <= r2 && !(16 * d2 > r2 && 4 * d2 < r2);
    }
}

// ---- the background: (g + 1)^2 nodes, cells of ch x cw pixels, ch = ceil(H / g): pixel (y, x) lies in cell (y / ch, x / cw), both < g
PPF_HD int synth_cell(int side, int g) { return (side + g - 1) / g; }
// one channel of the blend: floor(K / (ch * cw)), K <= 255 * 2^20
PPF_HD int synth_blend(int n00, int n01, int n10, int n11, int ry, int rx, int ch, int cw) {
    return ((ch - ry) * ((cw - rx) * n00 + rx * n01) + ry * ((cw - rx) * n10 + rx * n11)) / (ch * cw);
}

// ---- the spec words both entry points take, in one place: 0 or the index of the first rule that fails (synth.hip names it)
PPF_HD int synth_spec_fault(int C, int K, int D, int H, int W, int g, int noise) {
    if (K < 1 || K > SYNTH_MAX_PARTS) return 1;
    if (D < 0 || D > SYNTH_MAX_DISTRACTORS) return 2;
    if (C < 2 || C > SYNTH_MAX_CLASSES) return 3;
    if ((int64_t)C > synth_class_limit(K)) return 4;
    if (H < SYNTH_MIN_SIDE || H > SYNTH_MAX_SIDE) return 5;
    if (W < SYNTH_MIN_SIDE || W > SYNTH_MAX_SIDE) return 6;
    if (W % 16 != 0) return 7;
    if (g < 1 || g > SYNTH_MAX_GRID) return 8;
    if (noise < 0 || noise > SYNTH_MAX_NOISE) return 9;
    return 0;
}

// ---- scene edits (ppf_synth_edit): one edit (op, arg) applied to a scene row.  synth_edit_valid says whether the edit is one; for a valid
// edit synth_edit_word gives word w of the edited row from the row itself, so a lane per word needs nothing else; synth_edit_live says
// whether a difference in word w counts as a change: a node always, a word of a primitive when the primitive is on before or after the
// edit, nothing else (label and box never differ).  An invalid edit copies the row and reports -1.
constexpr int SYNTH_EDIT_COPY = 0, SYNTH_EDIT_PARTS_OFF = 1, SYNTH_EDIT_DISTRACTORS_OFF = 2, SYNTH_EDIT_BACKGROUND = 3, SYNTH_EDIT_PART_ATTR = 4;
constexpr int SYNTH_EDIT_OPS = 5;
PPF_HD bool synth_edit_valid(int op, int arg, int K, int D) {
    const uint32_t a = (uint32_t)arg;                                         // a negative arg has bit 31 set: above every mask and colour
    switch (op) {
        case SYNTH_EDIT_COPY: return true;
        case SYNTH_EDIT_PARTS_OFF: return (a >> K) == 0;                      // K <= 8: the shift is defined
        case SYNTH_EDIT_DISTRACTORS_OFF: return (a >> D) == 0;
        case SYNTH_EDIT_BACKGROUND: return a <= 0xFFFFFFu;
        case SYNTH_EDIT_PART_ATTR: return (a & 255u) < (uint32_t)K && (a >> 8) < (uint32_t)SYNTH_ATTRS;
        default: return false;
    }
}
PPF_HD int synth_edit_word(const int* row, int w, int op, int arg, int K, int D, int g) {
    const int v = row[w];
    if (w >= SYNTH_PART0 && w < SYNTH_DIST0) {
        const int k = (w - SYNTH_PART0) / SYNTH_PRIM_WORDS, f = (w - SYNTH_PART0) - k * SYNTH_PRIM_WORDS;
        if (op == SYNTH_EDIT_PARTS_OFF && f == SYNTH_ON && k < K && ((arg >> k) & 1)) return 0;
        if (op == SYNTH_EDIT_PART_ATTR && f == SYNTH_ATTR && k == (arg & 255)) return arg >> 8;
    } else if (w >= SYNTH_DIST0 && w < SYNTH_NODE0) {
        const int d = (w - SYNTH_DIST0) / SYNTH_PRIM_WORDS, f = (w - SYNTH_DIST0) - d * SYNTH_PRIM_WORDS;
        if (op == SYNTH_EDIT_DISTRACTORS_OFF && f == SYNTH_ON && d < D && ((arg >> d) & 1)) return 0;
    } else if (w >= SYNTH_NODE0 && w < SYNTH_NODE0 + (g + 1) * (g + 1)) {
        if (op == SYNTH_EDIT_BACKGROUND) return arg;
    }
    return v;
}
PPF_HD bool synth_edit_live(const int* row, int w, int op, int arg, int K, int D, int g) {
    if (w >= SYNTH_NODE0) return w < SYNTH_NODE0 + (g + 1) * (g + 1);
    if (w < SYNTH_PART0) return false;
    const int on = w - (w - SYNTH_PART0) % SYNTH_PRIM_WORDS + SYNTH_ON;       // SYNTH_DIST0 - SYNTH_PART0 is a multiple of the primitive's words
    return row[on] != 0 || synth_edit_word(row, on, op, arg, K, D, g) != 0;
}
