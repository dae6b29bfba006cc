// Stand-alone check of the Elastic loop's step arithmetic in
// opticalflow2d_amd/csrc/batch_plan.h (host only: no device, no libof2d.so):
// the workgroup's size, the sweep's steps, and the columns a thread relaxes at
// a step.  The sweep is walked as the kernel walks it
// (batch_elastic_kernels.hip: for every step, every thread, its columns) over a
// host grid of exactly the image's size, so a pixel outside the interior is an
// out-of-bounds access for AddressSanitizer as well as a failed check.  At each
// relaxed pixel the reference's order (OpticalFlowElastic.cpp:37-50, i outer, j
// inner, in place) is checked: the four neighbours it reads NEW were relaxed
// at an earlier step, the five it reads OLD at no step so far, and no pixel of
// the same step is a neighbour.
//   g++ -std=c++17 -I opticalflow2d_amd/csrc tests/host/batch_elastic_plan_test.cpp
//   (with -fsanitize=address,undefined for the sanitizer run)
#include <cstdio>
#include <vector>

#include "batch_plan.h"

namespace batch = of2d::batch;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        g_checked++;                                     \
        if (!(cond)) {                                   \
            if (g_failed++ < 20) {                       \
                std::fprintf(stderr, "FAIL: ");          \
                std::fprintf(stderr, __VA_ARGS__);       \
                std::fprintf(stderr, "  [%s]\n", #cond); \
            }                                            \
        }                                                \
    } while (0)

static void test_threads() {
    CHECK(batch::elastic_threads(1) == 64 && batch::elastic_threads(64) == 64, "one wave");
    CHECK(batch::elastic_threads(65) == 128 && batch::elastic_threads(130) == 192, "two, three");
    CHECK(batch::elastic_threads(512) == 512 && batch::elastic_threads(513) == 512 &&
              batch::elastic_threads(262144) == 512,
          "eight waves at most");
    for (int dx = 1; dx <= 2048; dx++) {
        const int T = batch::elastic_threads(dx);
        CHECK(T % 64 == 0 && T >= 64 && T <= 512 && (T >= dx || T == 512), "dx %d: %d threads", dx,
              T);
    }
}

static void test_first_col() {
    for (int T : {64, 192, 512})
        for (int lo = 1; lo < 3 * T; lo += 7)
            for (int tid = 0; tid < T; tid++) {
                const int i = batch::elastic_first_col(tid, lo, T);
                CHECK(i >= lo && i < lo + T && i % T == tid, "T %d lo %d tid %d: %d", T, lo, tid, i);
            }
}

// the step at which the walk relaxed each pixel, 0 for never
static void walk(int dx, int dy) {
    const int T = batch::elastic_threads(dx), tlast = batch::elastic_last_step(dx, dy);
    std::vector<int> step((size_t)dx * dy, 0);
    auto at = [&](int i, int j) -> int & { return step.at((size_t)j * dx + i); };
    long relaxed = 0;
    bool order = true, inside = true, once = true;
    for (int t = batch::kElasticFirstStep; t <= tlast; t++) {
        const int lo = batch::elastic_col_lo(t, dy), hi = batch::elastic_col_hi(t, dx);
        for (int tid = 0; tid < T; tid++)
            for (int i = batch::elastic_first_col(tid, lo, T); i <= hi; i += T) {
                const int j = t - 2 * i;
                if (i < 1 || i > dx - 2 || j < 1 || j > dy - 2) {
                    inside = false;
                    continue;
                }
                once = once && at(i, j) == 0;
                // NEW: relaxed at an earlier step, or on the border (never relaxed)
                const int nw[4][2] = {{i - 1, j - 1}, {i - 1, j}, {i - 1, j + 1}, {i, j - 1}};
                for (auto &q : nw) {
                    const bool border = q[0] == 0 || q[1] == 0 || q[1] == dy - 1;
                    order = order && (border ? at(q[0], q[1]) == 0
                                             : (at(q[0], q[1]) > 0 && at(q[0], q[1]) < t));
                }
                // OLD: not relaxed so far, this step included
                const int od[4][2] = {{i, j + 1}, {i + 1, j - 1}, {i + 1, j}, {i + 1, j + 1}};
                for (auto &q : od) order = order && at(q[0], q[1]) == 0;
                at(i, j) = t;
                relaxed++;
            }
    }
    CHECK(inside, "%dx%d: a pixel outside the interior", dx, dy);
    CHECK(once, "%dx%d: a pixel relaxed twice", dx, dy);
    CHECK(order, "%dx%d: the reference's order", dx, dy);
    const long want = (dx < 3 || dy < 3) ? 0 : (long)(dx - 2) * (dy - 2);
    CHECK(relaxed == want, "%dx%d: %ld of %ld interior pixels", dx, dy, relaxed, want);
    bool all = true;
    for (int j = 1; j < dy - 1; j++)
        for (int i = 1; i < dx - 1; i++) all = all && at(i, j) == 2 * i + j;
    CHECK(all, "%dx%d: pixel (i, j) at step 2 i + j", dx, dy);
}

static void test_walks() {
    const int shapes[][2] = {{1, 1},   {2, 7},    {7, 2},    {3, 3},   {5, 4},    {4, 5},
                             {63, 9},  {64, 9},   {65, 9},   {130, 20}, {9, 200},  {1024, 16},
                             {513, 3}, {1537, 5}, {64, 64},  {128, 128}, {3, 600},  {600, 3}};
    for (auto &s : shapes) walk(s[0], s[1]);
    CHECK(batch::elastic_last_step(3, 3) == 3 && batch::elastic_last_step(64, 64) == 186, "steps");
    CHECK(batch::elastic_last_step(2, 7) < batch::kElasticFirstStep &&
              batch::elastic_last_step(7, 2) < batch::kElasticFirstStep,
          "no interior, no step");
}

int main() {
    test_threads();
    test_first_col();
    test_walks();
    std::printf("batch_elastic_plan_test: %d checked, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
