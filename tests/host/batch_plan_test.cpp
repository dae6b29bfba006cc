// Stand-alone check of opticalflow2d_amd/csrc/batch_plan.h (host only: no
// device, no libof2d.so): the staging rounds of the batch's boundary copies,
// the argument checks of its analysis calls, the fit rules of the loop's
// on-CU placements and what each kind of loop needs.  The rounds are checked by
// simulating the copies on host buffers of exactly the sizes the driver
// allocates, so an offset or a count that is off by one is an out-of-bounds
// access for AddressSanitizer as well as a failed check.
//   g++ -std=c++17 -I opticalflow2d_amd/csrc tests/host/batch_plan_test.cpp
//   (with -fsanitize=address,undefined for the sanitizer run)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <utility>
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

// the pitch and pair stride of a level as of2d_device.h / of2d_batch.h define
// them (restated: those headers need HIP)
static int pitch_of(int dimx) { return (dimx + 127) / 128 * 128; }
static long stride_of(int dimx, int dimy) { return (long)(dimy + 2) * pitch_of(dimx) + 128; }

static void test_chunk_pairs() {
    const int dims[][2] = {{2, 2}, {16, 12}, {37, 29}, {128, 128}, {256, 256}, {512, 512}, {1, 1}};
    for (const auto &d : dims)
        for (int B : {1, 2, 3, 15, 16, 17, 63, 64, 65, 300, 1024, 65535}) {
            const size_t c = batch::stage_chunk_pairs(B, d[0], d[1]);
            const size_t n0 = (size_t)d[0] * d[1];
            CHECK(c >= 1 && c <= (size_t)B, "1 <= chunk <= B (%dx%d B %d)", d[0], d[1], B);
            CHECK(c == 1 || c * 2 * n0 * sizeof(double) <= ((size_t)64 << 20),
                  "a chunk of more than one pair stays within 64 MiB (%dx%d B %d)", d[0], d[1], B);
            CHECK(c == (size_t)B || (c + 1) * 2 * n0 * sizeof(double) > ((size_t)64 << 20) || c == 1,
                  "the chunk is as large as the buffer allows (%dx%d B %d)", d[0], d[1], B);
        }
}

// move npairs images and motion fields host -> stage -> pitched fields -> stage
// -> host through the rounds; every element must arrive exactly once
static void simulate(int npairs, size_t stage_pairs, int dimx, int dimy) {
    const size_t n0 = (size_t)dimx * dimy;
    const long stride = stride_of(dimx, dimy);
    const int P = pitch_of(dimx);
    std::vector<double> host(npairs * 2 * n0), back(npairs * 2 * n0, -1.0);
    for (size_t k = 0; k < host.size(); k++) host[k] = (double)k + 0.5;
    std::vector<double> stage(stage_pairs * 2 * n0);
    std::vector<double> field((size_t)stride * npairs, 0.0);  // one plane per pair is enough
    double *row0 = field.data() + P;                          // row 0 of pair 0, as BField::p
    const std::vector<batch::StageRound> rounds =
        batch::stage_rounds(npairs, stage_pairs, stride, dimx, dimy);
    int next = 0;
    for (const batch::StageRound &r : rounds) {
        CHECK(r.k0 == next && r.nk >= 1 && (size_t)r.nk <= stage_pairs,
              "rounds are consecutive and fit the buffer (B %d stage %zu)", npairs, stage_pairs);
        next = r.k0 + r.nk;
        CHECK(r.field == (long)r.k0 * stride && r.image == (size_t)r.k0 * n0 &&
                  r.motion == (size_t)r.k0 * 2 * n0,
              "offsets are the first pair's (B %d stage %zu k0 %d)", npairs, stage_pairs, r.k0);
        // images in: host stack -> stage -> fields (d2f's indexing)
        std::memcpy(stage.data(), host.data() + r.image, sizeof(double) * r.nk * n0);
        for (int k = 0; k < r.nk; k++)
            for (int j = 0; j < dimy; j++)
                for (int i = 0; i < dimx; i++)
                    // skip ghost line above pair 0's row 0: row0 already points past it
                    (row0 + r.field)[(long)k * stride + (long)j * P + i] =
                        stage[(size_t)k * n0 + (size_t)j * dimx + i];
        // motion out: fields -> stage (planar, two planes per pair) -> host stack
        for (int k = 0; k < r.nk; k++)
            for (size_t e = 0; e < n0; e++) {
                const double v = (row0 + r.field)[(long)k * stride + (long)(e / dimx) * P +
                                                  (long)(e % dimx)];
                stage[(size_t)k * 2 * n0 + e] = v;
                stage[(size_t)k * 2 * n0 + n0 + e] = -v;
            }
        std::memcpy(back.data() + r.motion, stage.data(), sizeof(double) * 2 * r.nk * n0);
    }
    CHECK(next == npairs, "every pair is moved (B %d stage %zu)", npairs, stage_pairs);
    bool same = true;
    for (int k = 0; k < npairs && same; k++)
        for (size_t e = 0; e < n0 && same; e++) {
            const double want = host[(size_t)k * n0 + e];  // the image stack's pair k
            same = back[(size_t)k * 2 * n0 + e] == want && back[(size_t)k * 2 * n0 + n0 + e] == -want;
        }
    CHECK(same, "every element arrives once, in its pair's slot (B %d stage %zu %dx%d)", npairs,
          stage_pairs, dimx, dimy);
}

static void test_rounds() {
    const int dims[][2] = {{2, 2}, {16, 12}, {37, 29}, {130, 33}};
    for (const auto &d : dims)
        for (int B : {1, 2, 3, 5, 7, 16})
            for (size_t stage : {(size_t)1, (size_t)2, (size_t)3, (size_t)4, (size_t)16, (size_t)64})
                simulate(B, stage, d[0], d[1]);
    // the driver's own pairing: the stage holds stage_chunk_pairs(B) pairs; a
    // shared reference moves one pair through it
    for (int B : {1, 3, 300}) {
        const size_t c = batch::stage_chunk_pairs(B, 16, 12);
        simulate(B, c, 16, 12);
        simulate(1, c, 16, 12);
    }
    CHECK(batch::stage_rounds(0, 4, 100, 4, 4).empty(), "no pairs, no rounds");
    CHECK(batch::stage_rounds(3, 0, 100, 4, 4).empty(), "no buffer, no rounds");
    // offsets of the largest batch stay exact in their types
    const long stride = stride_of(512, 512);
    const auto big = batch::stage_rounds(65535, 16, stride, 512, 512);
    CHECK(big.back().k0 + big.back().nk == 65535, "the last round ends at the last pair");
    CHECK(big.back().field == (long)big.back().k0 * stride && big.back().field > (1L << 32),
          "field offsets beyond 2^32 elements are exact");
    CHECK(big.back().motion == (size_t)big.back().k0 * 2 * 512 * 512,
          "motion offsets beyond 2^32 elements are exact");
}

static void test_refusals() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double inf = std::numeric_limits<double>::infinity();
    CHECK(batch::jacobian_refusal(2, 2) == nullptr, "2 x 2 is the smallest field");
    for (const auto &d : {std::pair<int, int>{1, 5}, {5, 1}, {1, 1}, {0, 4}, {-3, 4}}) {
        CHECK(batch::jacobian_refusal(d.first, d.second) != nullptr, "%d x %d is refused", d.first,
              d.second);
        CHECK(batch::invert_refusal(d.first, d.second, 5, 1e-3) != nullptr, "%d x %d is refused",
              d.first, d.second);
    }
    CHECK(batch::invert_refusal(2, 2, 1, 1e-3) == nullptr, "one update is allowed");
    CHECK(batch::invert_refusal(2, 2, 1, 5e-324) == nullptr, "any positive finite tol is allowed");
    for (int it : {0, -1, std::numeric_limits<int>::min()})
        CHECK(std::strstr(batch::invert_refusal(16, 12, it, 1e-3), "max_iter < 1") != nullptr,
              "max_iter %d is refused", it);
    for (double tol : {0.0, -0.0, -1e-3, nan, inf, -inf})
        CHECK(std::strstr(batch::invert_refusal(16, 12, 5, tol), "tol must be finite") != nullptr,
              "tol %g is refused", tol);
    // the size comes first, then max_iter, then tol: the one-pair entries' order
    CHECK(std::strstr(batch::invert_refusal(1, 12, 0, nan), "dimx >= 2") != nullptr, "size first");
    CHECK(std::strstr(batch::invert_refusal(16, 12, 0, nan), "max_iter") != nullptr,
          "max_iter before tol");
}

// The documented corners of the two on-CU fit rules,
// the byte counts as the document states them, and the instantiation a level
// runs: a compiled one that holds the thread's pixels
static void test_fit_rules() {
    CHECK(batch::kLoopThreads == 1024, "a pair's workgroup has 1024 threads");
    // resident: (dx + 2) x (dy + 2) elements of 8 bytes; 1 KiB reserve of 160 KiB
    CHECK(batch::resident_fits(128, 128), "resident: 128 x 128 fits");
    CHECK(batch::resident_lds_bytes(128, 128) == 135200, "resident: 128 x 128 is 135 200 B");
    CHECK(!batch::resident_fits(129, 128), "resident: 129 x 128 fails");
    CHECK(129 * 128 > 16 * 1024 && batch::resident_lds_bytes(129, 128) + 1024 <= 160 * 1024,
          "resident: 129 x 128 fails on the pixels, not the bytes");
    CHECK(!batch::resident_fits(150, 120), "resident: 150 x 120 fails");
    CHECK(150 * 120 > 16 * 1024 && batch::resident_lds_bytes(150, 120) + 1024 <= 160 * 1024,
          "resident: 150 x 120 fails on the pixels, not the bytes");
    CHECK(!batch::resident_fits(2, 6000), "resident: 2 x 6000 fails");
    CHECK(2 * 6000 <= 16 * 1024 && batch::resident_lds_bytes(2, 6000) + 1024 > 160 * 1024,
          "resident: 2 x 6000 fails on the bytes, not the pixels");
    CHECK(batch::resident_fits(1, 1) && batch::resident_lds_bytes(1, 1) == 72,
          "resident: 1 x 1 fits with its ghost ring");
    // conv_lds: dx * dy + dx + 1 elements of 8 bytes
    CHECK(batch::conv_lds_fits(128, 128), "conv_lds: 128 x 128 fits");
    CHECK(batch::conv_lds_bytes(128, 128) == 132104, "conv_lds: 128 x 128 is 132 104 B");
    CHECK(!batch::conv_lds_fits(129, 128), "conv_lds: 129 x 128 fails");
    CHECK(batch::conv_lds_fits(1, 1), "conv_lds: 1 x 1 fits");
    for (const auto &d : {std::pair<int, int>{0, 4}, {4, 0}, {0, 0}, {-1, 4}, {4, -1}, {-3, -3},
                          {std::numeric_limits<int>::min(), 1}}) {
        CHECK(!batch::resident_fits(d.first, d.second), "resident: %d x %d fails", d.first, d.second);
        CHECK(!batch::conv_lds_fits(d.first, d.second), "conv_lds: %d x %d fails", d.first, d.second);
    }
    for (int dy = 1; dy <= 130; dy++)
        for (int dx = 1; dx <= 130; dx++) {
            const int need = (dx * dy + 1023) / 1024;  // ceil(dx * dy / 1024)
            const int r = batch::resident_ppt(dx, dy), c = batch::conv_lds_ppt(dx, dy);
            CHECK(r == 1 || r == 2 || r == 4 || r == 8 || r == 16,
                  "resident: %d x %d runs a compiled instantiation (%d)", dx, dy, r);
            CHECK(c == 1 || c == 4 || c == 16, "conv_lds: %d x %d runs a compiled instantiation (%d)",
                  dx, dy, c);
            CHECK(!batch::resident_fits(dx, dy) || r >= need,
                  "resident: %d x %d, %d pixels per thread hold %d", dx, dy, r, need);
            CHECK(!batch::conv_lds_fits(dx, dy) || c >= need,
                  "conv_lds: %d x %d, %d pixels per thread hold %d", dx, dy, c, need);
            CHECK(batch::resident_fits(dx, dy) == (dx * dy <= 16384) &&
                      batch::conv_lds_fits(dx, dy) == (dx * dy <= 16384),
                  "%d x %d: up to 130 x 130 only the pixels decide", dx, dy);
        }
}

// What each kind of loop needs of the driver: the kind from the method and
// option "fluid", the workgroup at the widths where elastic_waves steps, the
// launches per loop, and the one on-CU option a kind admits with its fit rule
static void test_loop_kinds() {
    using K = batch::LoopKind;
    CHECK(batch::loop_kind(0, false) == K::HornSchunck && batch::loop_kind(1, false) == K::Curvature &&
              batch::loop_kind(2, false) == K::Elastic && batch::loop_kind(2, true) == K::Fluid &&
              batch::loop_kind(3, false) == K::Demons,
          "the kind follows the method, Fluid is an Elastic batch with its option");
    const K kinds[] = {K::HornSchunck, K::Curvature, K::Elastic, K::Fluid, K::Demons};
    const int waves[][2] = {{1, 1}, {64, 1}, {65, 2}, {512, 8}, {513, 8}, {1024, 8}};
    for (const auto &w : waves) {
        const int dx = w[0];
        CHECK(batch::elastic_threads(dx) == 64 * w[1], "dx %d: %d waves sweep", dx, w[1]);
        CHECK(batch::loop_threads(K::HornSchunck, dx) == batch::kLoopThreads &&
                  batch::loop_threads(K::Demons, dx) == batch::kLoopThreads,
              "dx %d: Horn-Schunck and Demons run kLoopThreads", dx);
        CHECK(batch::loop_threads(K::Curvature, dx) == batch::kCurvThreads,
              "dx %d: Curvature runs kCurvThreads", dx);
        CHECK(batch::loop_threads(K::Elastic, dx) == batch::elastic_threads(dx) &&
                  batch::loop_threads(K::Fluid, dx) == batch::elastic_threads(dx),
              "dx %d: Elastic and Fluid run elastic_threads", dx);
    }
    for (K k : kinds) {
        const bool demons = k == K::Demons;
        CHECK(batch::loop_takes_gradients(k) == !demons, "only Demons skips the gradients pass");
        CHECK(batch::loop_launches(k) == (demons ? 3 : 4), "launches per loop: Demons 3, else 4");
        CHECK(batch::loop_sweeps(k) == (k == K::Elastic || k == K::Fluid), "Elastic and Fluid sweep");
    }
    CHECK(std::strcmp(batch::on_cu_option(K::HornSchunck), "resident") == 0 &&
              std::strcmp(batch::on_cu_option(K::Demons), "conv_lds") == 0,
          "Horn-Schunck admits resident, Demons conv_lds");
    for (K k : {K::Curvature, K::Elastic, K::Fluid}) {
        CHECK(batch::on_cu_option(k) == nullptr, "no on-CU option for the other kinds");
        CHECK(!batch::on_cu_fits(k, 16, 16) && !batch::on_cu_fits(k, 1, 1), "and no level fits");
    }
    for (const auto &d : {std::pair<int, int>{1, 1}, {128, 128}, {129, 128}, {2, 6000}, {0, 4}}) {
        CHECK(batch::on_cu_fits(K::HornSchunck, d.first, d.second) ==
                  batch::resident_fits(d.first, d.second),
              "Horn-Schunck fits by resident_fits (%d x %d)", d.first, d.second);
        CHECK(batch::on_cu_fits(K::Demons, d.first, d.second) ==
                  batch::conv_lds_fits(d.first, d.second),
              "Demons fits by conv_lds_fits (%d x %d)", d.first, d.second);
    }
}

int main() {
    test_chunk_pairs();
    test_rounds();
    test_refusals();
    test_fit_rules();
    test_loop_kinds();
    std::printf("batch_plan_test: %d checked, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
