// Host check of the scene-edit rule of protopformer_amd/csrc/synth_plan.h (what ppf_synth_edit's lanes run): synth_edit_valid,
// synth_edit_word and synth_edit_live against a second, naive implementation that edits a copy of the row op by op -- over every op,
// every part k and distractor d, every mask, rows with primitives on and off, and the invalid cases.  Stand-alone (its own main); built
// with the host compiler under AddressSanitizer + UBSan by tests/test_synth_edit_cpu.py.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "synth_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++failures <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                  \
    } while (0)

// the rule as the kernel applies it: word by word
static int rule(const int* row, int op, int arg, int K, int D, int g, int* out) {
    if (!synth_edit_valid(op, arg, K, D)) {
        memcpy(out, row, sizeof(int) * SYNTH_WORDS);
        return -1;
    }
    int changed = 0;
    for (int w = 0; w < SYNTH_WORDS; ++w) {
        out[w] = synth_edit_word(row, w, op, arg, K, D, g);
        if (out[w] != row[w] && synth_edit_live(row, w, op, arg, K, D, g)) changed = 1;
    }
    return changed;
}

// the naive form: the issue's sentences, one after the other
static int naive(const int* row, int op, long long arg, int K, int D, int g, int* out) {
    memcpy(out, row, sizeof(int) * SYNTH_WORDS);
    int changed = 0;
    if (op == 0) return 0;
    if (op == 1 || op == 2) {
        const int n = op == 1 ? K : D, base = op == 1 ? SYNTH_PART0 : SYNTH_DIST0;
        if (arg < 0 || arg >= (1LL << n)) return -1;
        for (int k = 0; k < n; ++k)
            if (arg & (1LL << k)) {
                if (out[base + 5 * k] != 0) changed = 1;
                out[base + 5 * k] = 0;
            }
        return changed;
    }
    if (op == 3) {
        if (arg < 0 || arg > 0xFFFFFF) return -1;
        for (int q = 0; q < (g + 1) * (g + 1); ++q) {
            if (out[SYNTH_NODE0 + q] != (int)arg) changed = 1;
            out[SYNTH_NODE0 + q] = (int)arg;
        }
        return changed;
    }
    if (op == 4) {
        if (arg < 0) return -1;
        const long long k = arg & 255, attr = arg >> 8;
        if (k >= K || attr >= 24) return -1;
        if (out[SYNTH_PART0 + 5 * k] != 0 && out[SYNTH_PART0 + 5 * k + 4] != (int)attr) changed = 1;
        out[SYNTH_PART0 + 5 * k + 4] = (int)attr;
        return changed;
    }
    return -1;
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// a row as ppf_synth_scene would leave it for (K, D, g): entries past K, D and the nodes are zero
static void make_row(int* row, int K, int D, int g, uint32_t& s, int on_mode) {
    memset(row, 0, sizeof(int) * SYNTH_WORDS);
    row[SYNTH_LABEL] = (int)(lcg(s) >> 8) % 20;
    row[SYNTH_BOX] = 3; row[SYNTH_BOX + 1] = 4; row[SYNTH_BOX + 2] = 40; row[SYNTH_BOX + 3] = 41;
    for (int k = 0; k < K + D; ++k) {
        int* p = row + (k < K ? SYNTH_PART0 + 5 * k : SYNTH_DIST0 + 5 * (k - K));
        p[SYNTH_ON] = on_mode == 0 ? 0 : on_mode == 1 ? 1 : (int)((lcg(s) >> 16) & 1);
        p[SYNTH_CX] = 5 + (int)((lcg(s) >> 8) % 50); p[SYNTH_CY] = 5 + (int)((lcg(s) >> 8) % 50); p[SYNTH_R] = 3 + (int)((lcg(s) >> 8) % 5);
        p[SYNTH_ATTR] = (int)((lcg(s) >> 8) % SYNTH_ATTRS);
    }
    for (int q = 0; q < (g + 1) * (g + 1); ++q) row[SYNTH_NODE0 + q] = (int)(lcg(s) >> 8);
}

static long checked = 0;
static void one(const int* row, int op, int arg, int K, int D, int g) {
    std::vector<int> a(SYNTH_WORDS), b(SYNTH_WORDS);
    const int ca = rule(row, op, arg, K, D, g, a.data()), cb = naive(row, op, (long long)arg, K, D, g, b.data());
    CHECK(ca == cb, "changed %d != %d for op %d arg %d K %d D %d g %d", ca, cb, op, arg, K, D, g);
    CHECK(memcmp(a.data(), b.data(), sizeof(int) * SYNTH_WORDS) == 0, "rows differ for op %d arg %d K %d D %d g %d", op, arg, K, D, g);
    if (ca == -1) CHECK(memcmp(a.data(), row, sizeof(int) * SYNTH_WORDS) == 0, "an invalid edit must copy the row (op %d arg %d)", op, arg);
    ++checked;
}

int main() {
    static_assert((SYNTH_DIST0 - SYNTH_PART0) % SYNTH_PRIM_WORDS == 0, "synth_edit_live finds a primitive's on-word by this");
    uint32_t s = 12345u;
    std::vector<int> row(SYNTH_WORDS);
    const int KD[][2] = {{1, 0}, {4, 3}, {8, 8}, {3, 8}, {8, 1}};
    for (const auto& kd : KD) {
        const int K = kd[0], D = kd[1];
        for (int g = 1; g <= SYNTH_MAX_GRID; g += (g == 1 ? 3 : 4)) {            // 1, 4, 8
            for (int on_mode = 0; on_mode < 4; ++on_mode) {
                make_row(row.data(), K, D, g, s, on_mode);
                one(row.data(), SYNTH_EDIT_COPY, 0, K, D, g);
                one(row.data(), SYNTH_EDIT_COPY, -7, K, D, g);                   // COPY ignores its arg
                for (int mask = 0; mask < (1 << K); ++mask) one(row.data(), SYNTH_EDIT_PARTS_OFF, mask, K, D, g);
                for (int mask = 0; mask < (1 << D); ++mask) one(row.data(), SYNTH_EDIT_DISTRACTORS_OFF, mask, K, D, g);
                for (int k = 0; k < K; ++k)
                    for (int attr = 0; attr < SYNTH_ATTRS; ++attr) one(row.data(), SYNTH_EDIT_PART_ATTR, k | attr << 8, K, D, g);
                const int colours[] = {0, 0x808080, 0xFFFFFF, row[SYNTH_NODE0] & 0xFFFFFF};
                for (int c : colours) one(row.data(), SYNTH_EDIT_BACKGROUND, c, K, D, g);
                // the invalid kinds: an unknown op, a mask bit at K or D and above, k >= K, attr >= 24, a colour above 24 bits, negatives
                const int ops[] = {-1, SYNTH_EDIT_OPS, 6, 1000, (int)0x80000000};
                for (int op : ops) one(row.data(), op, 0, K, D, g);
                for (int bit = K; bit < 32; ++bit) one(row.data(), SYNTH_EDIT_PARTS_OFF, (int)(1u << bit) | 1, K, D, g);
                for (int bit = D; bit < 32; ++bit) one(row.data(), SYNTH_EDIT_DISTRACTORS_OFF, (int)(1u << bit), K, D, g);
                for (int k = K; k < 256; k += (k < 16 ? 1 : 37)) one(row.data(), SYNTH_EDIT_PART_ATTR, k | 3 << 8, K, D, g);
                const int attrs[] = {24, 25, 255, 256, 1 << 15, (1 << 23) - 1};
                for (int attr : attrs) one(row.data(), SYNTH_EDIT_PART_ATTR, 0 | attr << 8, K, D, g);
                one(row.data(), SYNTH_EDIT_PART_ATTR, -1, K, D, g);
                one(row.data(), SYNTH_EDIT_BACKGROUND, 0x1000000, K, D, g);
                one(row.data(), SYNTH_EDIT_BACKGROUND, -1, K, D, g);
                one(row.data(), SYNTH_EDIT_BACKGROUND, (int)0x80000000, K, D, g);
            }
        }
    }
    // the sentences of the contract, on one row: an invisible part and a no-op attribute change nothing
    make_row(row.data(), 4, 3, 4, s, 1);
    row[SYNTH_PART0 + 5 * 2 + SYNTH_ON] = 0;
    std::vector<int> out(SYNTH_WORDS);
    CHECK(rule(row.data(), SYNTH_EDIT_PARTS_OFF, 1 << 2, 4, 3, 4, out.data()) == 0, "hiding an invisible part changes nothing");
    CHECK(rule(row.data(), SYNTH_EDIT_PART_ATTR, 2 | ((row[SYNTH_PART0 + 14] + 1) % 24) << 8, 4, 3, 4, out.data()) == 0, "recolouring an invisible part changes nothing");
    CHECK(out[SYNTH_PART0 + 14] == (row[SYNTH_PART0 + 14] + 1) % 24, "... but the attribute is written");
    CHECK(rule(row.data(), SYNTH_EDIT_PART_ATTR, 1 | row[SYNTH_PART0 + 9] << 8, 4, 3, 4, out.data()) == 0, "an attribute set to its own value changes nothing");
    CHECK(rule(row.data(), SYNTH_EDIT_PARTS_OFF, 0xF, 4, 3, 4, out.data()) == 1, "hiding the visible parts is a change");
    CHECK(rule(row.data(), SYNTH_EDIT_PARTS_OFF, 1 << 4, 4, 3, 4, out.data()) == -1, "a mask bit at K is invalid");
    printf("checked %ld edits\n", checked);
    if (failures) { printf("synth edit: %d FAILURES\n", failures); return 1; }
    printf("synth edit: ok\n");
    return 0;
}
