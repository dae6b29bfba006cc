// Stand-alone check of the Curvature loop's host arithmetic in
// opticalflow2d_amd/csrc/batch_plan.h (host only: no device, no libof2d.so):
// which levels qualify, the chunks a pass moves its lines in, the dynamic LDS
// of a launch and a pair's scratch.  The chunking is checked by walking the
// kernel's own loops (batch_curvature_kernels.hip, curv_pass) over host
// buffers of exactly the sizes the driver allocates, so an index that is off
// by one is an out-of-bounds access for AddressSanitizer as well as a failed
// check.
//   g++ -std=c++17 -I opticalflow2d_amd/csrc tests/host/batch_curvature_plan_test.cpp
//   (with -fsanitize=address,undefined for the sanitizer run)
#include <algorithm>
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

static void test_sides() {
    for (int n = -4; n <= 2048; n++) {
        const bool want = n == 8 || n == 16 || n == 32 || n == 64 || n == 128 || n == 256 || n == 512;
        CHECK(batch::curv_side_ok(n) == want, "side %d", n);
    }
    CHECK(batch::curv_level_ok(8, 512) && batch::curv_level_ok(512, 8), "8 x 512");
    CHECK(!batch::curv_level_ok(16, 12) && !batch::curv_level_ok(4, 8) &&
              !batch::curv_level_ok(1024, 256) && !batch::curv_level_ok(64, 0),
          "refused levels");
    CHECK(batch::kCurvNMin == 8 && batch::kCurvNMax == 512, "the limits of include/of2d.h");
}

// one pass along an axis as the kernel walks it: every element of both planes
// is loaded into the chunk's LDS image exactly once, inside it, and stored
// back to where it came from
static void walk(int dx, int dy, int axis) {
    const int N = axis ? dy : dx, nlines = axis ? dx : dy;
    const int lpc = batch::curv_chunk_lines(N, nlines), chunks = batch::curv_chunks(N, nlines);
    const size_t lds = batch::curv_lds_bytes(dx, dy);
    CHECK(lpc >= 1 && lpc * N <= batch::kCurvChunkPoints, "%dx%d axis %d: a chunk's points", dx,
          dy, axis);
    CHECK(lpc * N <= batch::kCurvPointsPerThread * batch::kCurvThreads,
          "%dx%d axis %d: points per thread", dx, dy, axis);
    CHECK((chunks - 1) * lpc < nlines && chunks * lpc >= nlines, "%dx%d axis %d: %d chunks of %d",
          dx, dy, axis, chunks, lpc);
    CHECK(batch::curv_chunk_bytes(N, nlines) <= lds, "%dx%d axis %d: LDS", dx, dy, axis);
    std::vector<int> seen(batch::curv_scratch_doubles(dx, dy), 0);
    std::vector<char> z(lds / batch::kCurvPointBytes, 0);  // one flag per double2 point
    const long plane = (long)dx * dy;
    int trips = 0;
    for (int line0 = 0; line0 < nlines; line0 += lpc, trips++) {
        const int nl = std::min(lpc, nlines - line0), pts = nl * N;
        CHECK(pts % 4 == 0, "%dx%d axis %d: radix-4 butterflies", dx, dy, axis);
        std::fill(z.begin(), z.end(), 0);
        for (int g = 0; g < pts / 2; g++) {
            int l, m;
            long e0, e1;
            if (axis == 0) {
                l = g / (N / 2);
                m = g % (N / 2);
                e0 = (long)(line0 + l) * dx + 2 * m;
                e1 = e0 + 1;
            } else {
                m = g / nl;
                l = g - m * nl;
                e0 = (long)(2 * m) * dx + (line0 + l);
                e1 = e0 + dx;
            }
            CHECK(l < nl && m < N / 2, "%dx%d axis %d: lane %d", dx, dy, axis, g);
            for (long e : {e0, e1, e0 + plane, e1 + plane}) seen.at((size_t)e)++;
            // the line's points in LDS: m and N/2 + m (REDFT01), or as doubles
            // m, N - 1 - m of each plane (REDFT10): all within the line
            const size_t base = (size_t)l * (N + batch::kCurvLinePad);
            z.at(base + m)++;
            z.at(base + N / 2 + m)++;
            z.at(base + (N - 1 - m) / 2);
            z.at(base + N / 2 + (N - 1 - m) / 2);
        }
        int filled = 0;
        for (char c : z) filled += c;
        CHECK(filled == pts, "%dx%d axis %d: %d of %d points filled", dx, dy, axis, filled, pts);
    }
    CHECK(trips == chunks, "%dx%d axis %d: trips", dx, dy, axis);
    bool once = true;
    for (int c : seen) once = once && c == 1;
    CHECK(once, "%dx%d axis %d: every scratch element exactly once", dx, dy, axis);
}

static void test_chunks() {
    const int sides[] = {8, 16, 32, 64, 128, 256, 512};
    size_t most = 0;
    for (int dx : sides)
        for (int dy : sides) {
            walk(dx, dy, 0);
            walk(dx, dy, 1);
            const size_t lds = batch::curv_lds_bytes(dx, dy);
            most = std::max(most, lds);
            CHECK(lds + batch::kResidentLdsReserve <= 64 * 1024, "%dx%d: LDS %zu", dx, dy, lds);
            CHECK(batch::curv_scratch_doubles(dx, dy) * sizeof(double) == (size_t)16 * dx * dy,
                  "%dx%d: 16 B per pixel", dx, dy);
        }
    // the documented corners: 256 lines of 8 are the largest chunk; a 64 x 64
    // pass is two chunks of 32 lines; a 512-point line leaves 4 lines a chunk
    CHECK(most == (size_t)256 * 9 * 16, "largest chunk %zu", most);
    CHECK(batch::curv_chunks(64, 64) == 2 && batch::curv_chunk_lines(64, 64) == 32, "64 x 64");
    CHECK(batch::curv_chunks(128, 128) == 8 && batch::curv_chunk_lines(128, 128) == 16, "128 x 128");
    CHECK(batch::curv_chunks(512, 512) == 128 && batch::curv_chunk_lines(512, 512) == 4, "512");
    CHECK(batch::curv_chunks(8, 8) == 1 && batch::curv_chunk_lines(8, 8) == 8, "8 x 8");
    CHECK(batch::curv_chunks(8, 512) == 2 && batch::curv_chunk_lines(8, 512) == 256, "8 x 512");
    CHECK(batch::curv_lds_bytes(64, 64) == (size_t)32 * 65 * 16, "64 x 64 LDS");
}

int main() {
    test_sides();
    test_chunks();
    std::printf("batch_curvature_plan_test: %d checked, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
