// Host check of protopformer_amd/csrc/synth_plan.h, what the PartsWorld kernels and the host share: a stand-alone program built with the
// host compiler (tests/test_synth_plan_cpu.py), no GPU.  The word layout of the scene table, the class-table rule, the object and the slot
// layout at the extreme draws of every frame side, the distractors, the four shapes pixel by pixel, the background blend and the spec
// rules.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "synth_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++failures <= 20) {                       \
                printf("FAIL %s: ", #cond);               \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
        }                                                 \
    } while (0)

static const uint32_t U_MAX = (1u << 24) - 1;
static const uint32_t DRAWS[] = {0u, 1u, 1u << 23, (1u << 23) + 12345u, U_MAX - 1, U_MAX};

static void check_layout() {
    CHECK(SYNTH_PART0 == 5 && SYNTH_DIST0 == 45 && SYNTH_NODE0 == 85, "the word offsets moved: %d %d %d", SYNTH_PART0, SYNTH_DIST0, SYNTH_NODE0);
    CHECK(SYNTH_NODE0 + SYNTH_MAX_NODES <= SYNTH_WORDS && SYNTH_WORDS % 4 == 0, "the row does not hold %d nodes", SYNTH_MAX_NODES);
    CHECK(SYNTH_ITEM_PART0 + SYNTH_MAX_PARTS <= SYNTH_ITEM_DIST0 && SYNTH_ITEM_DIST0 + 2 * SYNTH_MAX_DISTRACTORS <= SYNTH_ITEM_NODE0, "items overlap");
    CHECK(SYNTH_STREAM_SCENE > 0xC0000000u && SYNTH_STREAM_NOISE > 0xC0000000u && SYNTH_STREAM_SCENE != SYNTH_STREAM_NOISE, "streams");
    std::set<int> cells;
    for (int k = 0; k < SYNTH_MAX_PARTS; ++k) cells.insert(synth_slot_cell(k));
    CHECK((int)cells.size() == SYNTH_MAX_PARTS && !cells.count(4) && *cells.begin() == 0 && *cells.rbegin() == 8, "the slots are not the 8 outer cells");
    for (uint32_t u : DRAWS)
        for (int n : {1, 2, 24, 1023}) CHECK(synth_range(u, n) >= 0 && synth_range(u, n) < n, "range(%u, %d) = %d", u, n, synth_range(u, n));
    CHECK(synth_range(U_MAX, 24) == 23 && synth_range(0, 24) == 0, "the range does not reach both ends");
}

static void check_classes() {
    const int cases[][2] = {{2, 1}, {24, 1}, {25, 2}, {1024, 3}, {1024, 8}};
    for (auto& ck : cases) {
        const int C = ck[0], K = ck[1];
        CHECK((int64_t)C <= synth_class_limit(K), "C=%d K=%d refused", C, K);
        std::set<std::vector<int>> rows;
        for (int c = 0; c < C; ++c) {
            std::vector<int> row(K);
            for (int k = 0; k < K; ++k) {
                row[k] = synth_class_part(c, k);
                CHECK(row[k] >= 0 && row[k] < SYNTH_ATTRS, "class %d part %d = %d", c, k, row[k]);
            }
            rows.insert(row);
        }
        CHECK((int)rows.size() == C, "C=%d K=%d: %d distinct rows", C, K, (int)rows.size());
    }
    CHECK(synth_class_limit(1) == 24 && synth_class_limit(2) == 576 && synth_class_limit(8) == (1LL << 31), "the limits: %lld %lld %lld",
          (long long)synth_class_limit(1), (long long)synth_class_limit(2), (long long)synth_class_limit(8));
    CHECK(synth_spec_fault(25, 1, 0, 32, 32, 1, 0) == 4 && synth_spec_fault(24, 1, 0, 32, 32, 1, 0) == 0, "C > A^K is not what is refused");
    for (int a = -3; a < 60; ++a) {
        CHECK(synth_shape_of(a) >= 0 && synth_shape_of(a) < SYNTH_SHAPES && synth_colour_of(a) >= 0 && synth_colour_of(a) < SYNTH_COLOURS, "attr %d", a);
    }
    std::set<int> colours;
    for (int c = 0; c < SYNTH_COLOURS; ++c) colours.insert(synth_palette(c));
    CHECK((int)colours.size() == SYNTH_COLOURS && !colours.count(SYNTH_BODY_RGB), "the palette repeats a colour or the body's");
}

// every frame side, the extreme draws: the box inside the frame, the parts inside the box and pairwise disjoint in the max norm
static void check_geometry() {
    for (int H = SYNTH_MIN_SIDE; H <= SYNTH_MAX_SIDE; H += (H < 80 ? 1 : 59)) {
        for (int W = SYNTH_MIN_SIDE; W <= SYNTH_MAX_SIDE; W += (W < 80 ? 16 : 112)) {
            for (uint32_t uh : DRAWS) for (uint32_t ux : DRAWS) for (uint32_t uy : DRAWS) {
                const SynthObject o = synth_object(uh, ux, uy, H, W);
                CHECK(o.ox - o.hs >= 0 && o.ox + o.hs + 1 <= W && o.oy - o.hs >= 0 && o.oy + o.hs + 1 <= H, "H=%d W=%d: box of hs=%d at (%d, %d)", H, W,
                      o.hs, o.ox, o.oy);
                const int p = synth_pitch(o.hs);
                CHECK(synth_part_radius(p) >= 3 && 2 * (synth_part_radius(p) + synth_jitter(p)) <= p - 1, "hs=%d: p=%d r=%d j=%d", o.hs, p,
                      synth_part_radius(p), synth_jitter(p));
                int cx[8], cy[8], r[8];
                for (int k = 0; k < 8; ++k) {
                    synth_part(k, o, k % 2 ? ux : uy, k % 3 ? uh : U_MAX - ux, &cx[k], &cy[k], &r[k]);
                    CHECK(cx[k] - r[k] >= o.ox - o.hs && cx[k] + r[k] <= o.ox + o.hs && cy[k] - r[k] >= o.oy - o.hs && cy[k] + r[k] <= o.oy + o.hs,
                          "H=%d W=%d hs=%d: part %d leaves the box", H, W, o.hs, k);
                    for (int q = 0; q < k; ++q) {
                        const int gx = abs(cx[k] - cx[q]) - r[k] - r[q], gy = abs(cy[k] - cy[q]) - r[k] - r[q];
                        CHECK(gx > 0 || gy > 0, "H=%d W=%d hs=%d: parts %d and %d touch", H, W, o.hs, q, k);
                    }
                }
                int dx, dy, dr;
                synth_distractor(uh, ux, uy, H, W, &dx, &dy, &dr);
                CHECK(dr >= 2 && dx - dr >= 0 && dx + dr < W && dy - dr >= 0 && dy + dr < H, "H=%d W=%d: distractor r=%d at (%d, %d)", H, W, dr, dx, dy);
            }
        }
    }
}

static void check_shapes() {
    for (int r = 1; r <= 130; ++r) {
        for (int s = 0; s < SYNTH_SHAPES; ++s) {
            CHECK(synth_inside(s, 0, 0, r), "shape %d r=%d misses its centre", s, r);
            int n = 0;
            for (int dy = -r - 2; dy <= r + 2; ++dy)
                for (int dx = -r - 2; dx <= r + 2; ++dx) {
                    const bool in = synth_inside(s, dx, dy, r);
                    n += in;
                    if (in) CHECK(abs(dx) <= r && abs(dy) <= r, "shape %d r=%d holds (%d, %d)", s, r, dx, dy);
                    CHECK(in == synth_inside(s, -dx, dy, r) && in == synth_inside(s, dy, dx, r), "shape %d r=%d is not symmetric at (%d, %d)", s, r, dx, dy);
                    if (s != SYNTH_SQUARE && in) CHECK(synth_inside(SYNTH_SQUARE, dx, dy, r), "shape %d r=%d outside the square", s, r);
                    if (s == SYNTH_RING && in) CHECK(synth_inside(SYNTH_DISK, dx, dy, r), "ring r=%d outside the disk", r);
                }
            if (s == SYNTH_SQUARE) CHECK(n == (2 * r + 1) * (2 * r + 1), "square r=%d has %d pixels", r, n);
            if (s == SYNTH_DIAMOND) CHECK(n == 2 * r * (r + 1) + 1, "diamond r=%d has %d pixels", r, n);
        }
        if (r >= 3) {
            int disk = 0, ring = 0;
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) { disk += synth_inside(SYNTH_DISK, dx, dy, r); ring += synth_inside(SYNTH_RING, dx, dy, r); }
            CHECK(ring < disk, "ring r=%d has no hole", r);
        }
    }
}

static void check_background_and_spec() {
    for (int side : {32, 37, 48, 256, 1000, 1024})
        for (int g = 1; g <= SYNTH_MAX_GRID; ++g) {
            const int c = synth_cell(side, g);
            CHECK(c * g >= side && (side - 1) / c < g, "side=%d g=%d: cell %d", side, g, c);
        }
    const int ch = synth_cell(1024, 1), cw = synth_cell(1024, 1);
    CHECK(synth_blend(255, 255, 255, 255, ch - 1, cw - 1, ch, cw) == 255 && synth_blend(7, 9, 200, 3, 0, 0, ch, cw) == 7, "the blend's ends");
    CHECK(synth_blend(0, 255, 0, 255, 0, cw / 2, ch, cw) == 127, "the blend's middle");
    const int ok[7] = {20, 4, 3, 256, 256, 4, 8};
    CHECK(synth_spec_fault(ok[0], ok[1], ok[2], ok[3], ok[4], ok[5], ok[6]) == 0, "the defaults are refused");
    CHECK(synth_spec_fault(20, 9, 3, 256, 256, 4, 8) == 1 && synth_spec_fault(20, 0, 3, 256, 256, 4, 8) == 1, "K");
    CHECK(synth_spec_fault(20, 4, 9, 256, 256, 4, 8) == 2 && synth_spec_fault(20, 4, -1, 256, 256, 4, 8) == 2, "D");
    CHECK(synth_spec_fault(1, 4, 3, 256, 256, 4, 8) == 3 && synth_spec_fault(1025, 4, 3, 256, 256, 4, 8) == 3, "C");
    CHECK(synth_spec_fault(20, 4, 3, 31, 256, 4, 8) == 5 && synth_spec_fault(20, 4, 3, 1025, 256, 4, 8) == 5, "H");
    CHECK(synth_spec_fault(20, 4, 3, 256, 16, 4, 8) == 6 && synth_spec_fault(20, 4, 3, 256, 1040, 4, 8) == 6, "W");
    CHECK(synth_spec_fault(20, 4, 3, 256, 40, 4, 8) == 7 && synth_spec_fault(20, 4, 3, 37, 48, 4, 8) == 0, "W %% 16");
    CHECK(synth_spec_fault(20, 4, 3, 256, 256, 0, 8) == 8 && synth_spec_fault(20, 4, 3, 256, 256, 9, 8) == 8, "g");
    CHECK(synth_spec_fault(20, 4, 3, 256, 256, 4, -1) == 9 && synth_spec_fault(20, 4, 3, 256, 256, 4, 33) == 9, "noise");
}

int main() {
    check_layout();
    check_classes();
    check_geometry();
    check_shapes();
    check_background_and_spec();
    if (failures) {
        printf("synth plan: %d failures\n", failures);
        return 1;
    }
    printf("synth plan: ok\n");
    return 0;
}
