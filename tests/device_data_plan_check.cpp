// Stand-alone host check of protopformer_amd/csrc/device_data_plan.h (built by tests/test_device_data_plan_cpu.py with the host compiler
// under AddressSanitizer + UBSan): the plan validation refuses every table that would carry a kernel outside the frames, the workspace
// layout holds what the kernels index, and the taps of a fixed table of cases are printed for the test to compare with the numpy
// referee (which tests/test_device_data_cpu.py holds to Pillow).  The tap buffers are allocated at exactly kmax entries, so a tap written
// past them is an AddressSanitizer report.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "device_data_plan.h"

static int failures = 0;

#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            ++failures;                   \
            printf("FAILED %s: ", #cond); \
            printf(__VA_ARGS__);          \
            printf("\n");                 \
        }                                 \
    } while (0)

static std::vector<double> good_plan() {
    // offset, h, w, box x0 y0 x1 y1, oh, ow, window y0 x0, mirror
    return {7, 37, 53, 3, 2, 50, 30, 12, 16, 0, 0, 1, /* second sample */ 7 + 37 * 53 * 3, 90, 61, 0, 0, 61, 90, 24, 18, 4, 1, 0};
}

static void check_layout() {
    const int64_t flat = 7 + 37 * 53 * 3 + 90 * 61 * 3;
    char err[320];
    RcLayout L;
    std::vector<double> p = good_plan();
    EXPECT(rc_layout("t", p.data(), 2, 12, 16, 3, flat, &L, err, sizeof(err)) == 0, "%s", err);
    // sample 1: scale 90 / 24 = 3.75, support 7.5: 2 * 8 + 1 taps; rows under the 12-row window: 3.75 * 12 + 15 + 3
    EXPECT(L.kmax == 17 && L.maxrows == 63, "kmax=%d maxrows=%d", L.kmax, L.maxrows);
    EXPECT(L.bounds_off >= (size_t)2 * 28 * L.kmax * 4 && L.rows_off >= L.bounds_off + 2 * 28 * 2 * 4 && L.bytes >= L.rows_off + (size_t)2 * L.maxrows * 16 * 3,
           "layout %zu %zu %zu", L.bounds_off, L.rows_off, L.bytes);
    EXPECT(L.bounds_off % 16 == 0 && L.rows_off % 16 == 0 && L.bytes % 16 == 0, "alignment");
    EXPECT(rc_layout("t", p.data(), 2, 12, 16, 2, flat, &L, err, sizeof(err)) == 0 && L.kmax == 9, "bilinear kmax=%d", L.kmax);
    struct Bad { int word; double value; const char* text; int code; };
    const Bad bad[] = {{12, 1e12, "leaves the", PPF_ERR_ARG},  {12, 7 + 37 * 53 * 3 + 1, "leaves the", PPF_ERR_ARG}, {0, -1, "leaves the", PPF_ERR_ARG},
                       {0, 7.5, "leaves the", PPF_ERR_ARG},    {1, 0, "leaves the", PPF_ERR_ARG},                    {2, 1e9, "leaves the", PPF_ERR_ARG},
                       {3, -1, "box", PPF_ERR_ARG},            {5, 54, "box", PPF_ERR_ARG},                          {5, 3, "box", PPF_ERR_ARG},
                       {6, 38, "box", PPF_ERR_ARG},            {7, 0, "output size", PPF_ERR_ARG},                   {8, 16.5, "output size", PPF_ERR_ARG},
                       {7, 11, "window", PPF_ERR_ARG},         {9, 1, "window", PPF_ERR_ARG},                        {10, -1, "window", PPF_ERR_ARG},
                       {11, 2, "mirror", PPF_ERR_ARG},         {4, NAN, "finite", PPF_ERR_ARG},                      {0, INFINITY, "finite", PPF_ERR_ARG}};
    for (const Bad& b : bad) {
        std::vector<double> q = good_plan();
        q[b.word] = b.value;
        err[0] = 0;
        const int rc = rc_layout("t", q.data(), 2, 12, 16, 3, flat, &L, err, sizeof(err));
        EXPECT(rc == b.code && strstr(err, b.text), "word %d = %g: rc=%d '%s'", b.word, b.value, rc, err);
    }
    EXPECT(rc_layout("t", nullptr, 2, 12, 16, 3, flat, &L, err, sizeof(err)) == PPF_ERR_ARG, "null plan");
    EXPECT(rc_layout("t", p.data(), 0, 12, 16, 3, flat, &L, err, sizeof(err)) == PPF_ERR_SHAPE, "B = 0");
    EXPECT(rc_layout("t", p.data(), 2, 12, 16, 1, flat, &L, err, sizeof(err)) == PPF_ERR_ARG && strstr(err, "filter"), "filter");
    std::vector<double> wide = {0, 16384, 16384, 0, 0, 16384, 16384, 1, 1, 0, 0, 0};          // 16384 -> 1: more taps than the kernels take
    EXPECT(rc_layout("t", wide.data(), 1, 1, 1, 3, (int64_t)16384 * 16384 * 3, &L, err, sizeof(err)) == PPF_ERR_SHAPE && strstr(err, "taps"), "'%s'", err);
}

// prints "taps filter size in0 in1 out xx : xmin k0 k1 ..." for every output coordinate of a case
static void print_taps(int filter, int size, double in0, double in1, int out) {
    const double scale = (in1 - in0) / out, fsc = scale < 1.0 ? 1.0 : scale;
    const int kmax = (int)ceil((filter == 3 ? 2.0 : 1.0) * fsc) * 2 + 1;
    for (int xx = 0; xx < out; ++xx) {
        std::vector<int> k(kmax);                      // exactly kmax: one tap more is a heap overflow
        int xmin = -1, n = -1;
        rc_taps(filter, size, in0, in1, out, xx, kmax, k.data(), &xmin, &n);
        EXPECT(n >= 1 && n <= kmax && xmin >= 0 && xmin + n <= size, "taps leave the axis: xmin=%d n=%d size=%d", xmin, n, size);
        long long sum = 0;
        for (int t = 0; t < n; ++t) sum += k[t];
        EXPECT(sum >= (1 << 22) - n && sum <= (1 << 22) + n, "weights sum to %lld", sum);
        printf("taps %d %d %.17g %.17g %d %d : %d", filter, size, in0, in1, out, xx, xmin);
        for (int t = 0; t < n; ++t) printf(" %d", k[t]);
        printf("\n");
    }
}

int main() {
    check_layout();
    for (int filter = 2; filter <= 3; ++filter) {
        print_taps(filter, 53, 0, 53, 16);             // minification
        print_taps(filter, 9, 0, 9, 16);               // magnification: the filter scale clamps to 1
        print_taps(filter, 53, 30, 53, 16);            // a box at the right edge: the taps clamp at the frame
        print_taps(filter, 53, 20, 21, 16);            // a one-pixel box
        print_taps(filter, 37, 2.25, 30.5, 12);        // a fractional box
        print_taps(filter, 375, 0, 375, 256);
        print_taps(filter, 16, 0, 16, 16);             // identity
    }
    if (failures) printf("device data plan: %d FAILED\n", failures);
    else printf("device data plan: ok\n");
    return failures ? 1 : 0;
}
