// Stand-alone check of opticalflow2d_amd/csrc/iter_schedule.h (host only: no
// device, no libof2d.so).  Every property is stated in words and checked by
// exhaustive sweeps or by simulating what the schedule does to the buffers;
// nothing is compared against the header's own output.
//   make -C tests/host && tests/host/iter_schedule_test
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "iter_schedule.h"

namespace sched = of2d::sched;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond, ...)                                \
    do {                                                \
        g_checked++;                                    \
        if (!(cond)) {                                  \
            if (g_failed++ < 20) {                      \
                std::fprintf(stderr, "FAIL: ");         \
                std::fprintf(stderr, __VA_ARGS__);      \
                std::fprintf(stderr, "  [%s]\n", #cond); \
            }                                           \
        }                                               \
    } while (0)

static void test_plan_fused() {
    const bool flags[3][2] = {{false, false}, {false, true}, {true, true}};  // {triples, pairs}
    for (int a = 0; a < 3; a++)
        for (int C = 1; C <= 40; C++)
            for (const auto &f : flags) {
                const bool triples = f[0], pairs = f[1];
                const sched::FusedPlan p = sched::plan_fused(a, C, triples, pairs);
                int t = 0, prev_out = a;
                // holds[b]: the iterate buffer b holds (iterate 0 = the chunk's start state)
                int holds[3] = {-1, -1, -1};
                holds[a] = 0;
                for (const sched::Launch &l : p.launches) {
                    CHECK(l.t == t, "t values are consecutive from 0 (a %d C %d)", a, C);
                    CHECK(l.in == prev_out, "a launch reads what the previous one wrote, the "
                          "first reads a (a %d C %d t %d)", a, C, l.t);
                    CHECK(l.out >= 0 && l.out < 3 && l.out != a,
                          "the start buffer is never written (a %d C %d t %d)", a, C, l.t);
                    CHECK(l.out != l.in, "no launch runs in place (a %d C %d t %d)", a, C, l.t);
                    const int left = C - t;
                    const int want = triples && left >= 3 ? 3 : (pairs && left >= 2 ? 2 : 1);
                    CHECK(l.K == want, "K = 3 while three remain and triples are on, then 2, "
                          "then 1 (a %d C %d t %d: K %d)", a, C, l.t, l.K);
                    if (!pairs)
                        CHECK(l.in == sched::single_src(a, t) && l.out == sched::single_dst(a, t),
                              "without fusing the plan is the single-step rotation (a %d t %d)", a,
                              t);
                    CHECK(holds[l.in] == t, "a launch reads iterate t (a %d C %d t %d)", a, C, t);
                    t += l.K;
                    holds[l.out] = t;
                    prev_out = l.out;
                }
                CHECK(t == C, "the K values sum to C (a %d C %d: %d)", a, C, t);
                CHECK(p.end == prev_out, "the end buffer is the last out (a %d C %d)", a, C);
                CHECK(holds[p.end] == C && holds[a] == 0,
                      "the end buffer holds iterate C, a its start state (a %d C %d)", a, C);
                // a break at t: iterate t + 1 is wanted in single_dst(a, t); when it
                // is not there the rule must ask for the replay (from a, intact)
                for (int tb = 0; tb < C; tb++) {
                    const bool there = holds[sched::single_dst(a, tb)] == tb + 1;
                    const bool replay = sched::fused_replay_needed(pairs, tb, C);
                    CHECK(there || replay, "a lost iterate is replayed (a %d C %d t %d)", a, C, tb);
                    if (!pairs)
                        CHECK(there == !replay, "single steps replay exactly when iteration "
                              "t + 2 overwrote the buffer (a %d C %d t %d)", a, C, tb);
                    else
                        CHECK(replay, "fused chunks always replay (a %d C %d t %d)", a, C, tb);
                }
            }
    // the rotation itself: reads what the previous step wrote, never writes a
    for (int a = 0; a < 3; a++) {
        CHECK(sched::single_src(a, 0) == a, "the first step reads a");
        for (int t = 0; t < 40; t++) {
            CHECK(sched::single_dst(a, t) != a && sched::single_dst(a, t) != sched::single_src(a, t),
                  "a step writes neither a nor its input (a %d t %d)", a, t);
            CHECK(sched::single_src(a, t + 1) == sched::single_dst(a, t),
                  "a step reads the previous step's output (a %d t %d)", a, t);
        }
        for (int b = 0; b < 3; b++) {
            const int o = sched::other(a, b);
            CHECK(o != a && o != b && o >= 0 && o < 3, "other(a, b) is neither (a %d b %d)", a, b);
        }
    }
}

template <int R>
static void test_ring() {
    using Rg = sched::Ring<R>;
    for (int a = 0; a <= R; a++) {
        CHECK(Rg::src(a, 0) == a, "the first iteration reads a (R %d a %d)", R, a);
        for (int t = 0; t <= 4 * R; t++) {
            const int b = Rg::ring(a, t);
            CHECK(b != a && b >= 0 && b <= R, "ring(a, t) is a buffer other than a (R %d a %d t %d)",
                  R, a, t);
            CHECK(Rg::src(a, t + 1) == b, "an iteration reads the previous one's buffer (R %d a %d "
                  "t %d)", R, a, t);
            std::set<int> seen;
            for (int q = t; q < t + R; q++) seen.insert(Rg::ring(a, q));
            CHECK((int)seen.size() == R, "R consecutive iterations write R distinct buffers (R %d "
                  "a %d t %d)", R, a, t);
        }
        for (int C = 1; C <= 4 * R + 1; C++)
            for (int t = 0; t < C; t++) {
                bool reused = false;
                for (int q = t + 1; q <= C - 1; q++) reused = reused || Rg::ring(a, q) == Rg::ring(a, t);
                CHECK(Rg::replay_needed(t, C) == reused, "a replay exactly when a later iteration "
                      "of the chunk reused the buffer (R %d a %d C %d t %d)", R, a, C, t);
            }
    }
    CHECK(Rg::slot(0) == 0, "iterate 0 is in buffer 0 (R %d)", R);
    for (int j = 1; j <= 4 * R; j++) {
        CHECK(Rg::slot(j) >= 1 && Rg::slot(j) <= R, "iterate j >= 1 is in buffers 1..R (R %d j %d)",
              R, j);
        std::set<int> seen;
        for (int q = j; q < j + R; q++) seen.insert(Rg::slot(q));
        CHECK((int)seen.size() == R, "R consecutive iterates sit in R distinct buffers (R %d j %d)",
              R, j);
    }
}

static void test_plan_blocks() {
    for (int niter = 0; niter <= 100; niter++)
        for (int blk : {3, 9, 33}) {
            const std::vector<sched::Block> b = sched::plan_blocks(niter, blk);
            int at = 0, tails = 0;
            for (size_t i = 0; i < b.size(); i++) {
                CHECK(b[i].lo == at && b[i].hi > b[i].lo, "the blocks tile [0, niter) in order "
                      "without a gap (niter %d blk %d block %zu)", niter, blk, i);
                at = b[i].hi;
                if (b[i].tail) {
                    tails++;
                    CHECK(i + 1 == b.size(), "the tail is the last block (niter %d blk %d)", niter,
                          blk);
                    CHECK(b[i].hi - b[i].lo == niter % 3, "the tail holds niter mod 3 iterations "
                          "(niter %d blk %d)", niter, blk);
                } else {
                    CHECK(b[i].lo % 3 == 0 && (b[i].hi - b[i].lo) % 3 == 0,
                          "a block starts on a multiple of three and holds whole triples "
                          "(niter %d blk %d block %zu)", niter, blk, i);
                    CHECK(b[i].hi - b[i].lo <= blk, "a block holds at most blk iterations "
                          "(niter %d blk %d block %zu)", niter, blk, i);
                }
            }
            CHECK(at == niter, "the blocks end at niter (niter %d blk %d)", niter, blk);
            CHECK(tails == (niter % 3 ? 1 : 0), "one tail block exactly when niter is no multiple "
                  "of three (niter %d blk %d)", niter, blk);
        }
    for (int cb = 1; cb <= 200; cb++) {
        const int blk = sched::pipelined_block(cb, 64, 2);
        CHECK(blk % 3 == 0 && blk >= 3, "a block is whole triples (cb %d)", cb);
        CHECK(blk <= 3 * (64 / 2 - 4), "two blocks' groups fit the event ring with four to spare "
              "(cb %d)", cb);
        CHECK(blk >= cb || blk == 3 * (64 / 2 - 4), "cb is only rounded up, unless capped (cb %d)",
              cb);
        CHECK(blk < cb + 3, "cb is rounded up by less than a triple (cb %d)", cb);
    }
}

static unsigned bits(float f) {
    unsigned u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

// sums {diff, prev} with prev = 1 and npx = 1: the error is diff itself
template <class T>
static void test_break_thresholds() {
    const float at = 0.001f, below = std::nextafterf(at, 0.0f), above = std::nextafterf(at, 1.0f);
    const float errs_in[6] = {below, below, above, at, below, above};
    T sums[12];
    for (int i = 0; i < 6; i++) {
        sums[2 * i] = (T)errs_in[i];
        sums[2 * i + 1] = (T)1;
    }
    struct Case {
        int k0;
        bool fixed;
        int want;
        const char *what;
    } cases[] = {
        {0, false, 4, "sub-threshold errors at k = 0 and k = 1 do not break, 0.001f itself and one "
                      "ulp above do not, one ulp below at k = 4 does"},
        {1, false, 1, "from k0 = 1 the error below at k = 1 does not break, the one at k = 2 does"},
        {5, false, 0, "from k0 = 5 the first error below the threshold breaks"},
        {0, true, -1, "a fixed run never breaks"},
        {5, true, -1, "a fixed run never breaks"},
    };
    for (const Case &c : cases) {
        std::vector<float> errs = {42.0f};  // appended to, not cleared
        std::vector<std::pair<int, float>> seen;
        const int t = sched::logger_break(sums, 6, c.k0, 1.0, c.fixed, errs,
                                          [&](int k, float e) { seen.push_back({k, e}); });
        CHECK(t == c.want, "%s (got %d)", c.what, t);
        const size_t n = t >= 0 ? (size_t)t + 1 : 6;
        CHECK(errs.size() == 1 + n && errs[0] == 42.0f,
              "t + 1 errors are appended on a break, C otherwise (%s)", c.what);
        CHECK(seen.size() == n, "every appended error is reported once (%s)", c.what);
        for (size_t i = 0; i < n && i + 1 < errs.size() && i < seen.size(); i++) {
            CHECK(bits(errs[1 + i]) == bits(errs_in[i]), "with prev = npx = 1 the error is diff");
            CHECK(seen[i].first == c.k0 + (int)i && bits(seen[i].second) == bits(errs[1 + i]),
                  "the report carries the iteration and its error");
        }
    }
    // above the threshold everywhere: no break
    T high[8] = {(T)above, (T)1, (T)at, (T)1, (T)0.5f, (T)1, (T)above, (T)1};
    std::vector<float> errs;
    CHECK(sched::logger_break(high, 4, 0, 1.0, false, errs, [](int, float) {}) == -1 &&
              errs.size() == 4,
          "no error below the threshold: no break, C errors");
    // a zero prev norm gives the reference's error 0, which breaks once k > 1
    T zero[6] = {(T)1, (T)0, (T)1, (T)0, (T)1, (T)0};
    errs.clear();
    CHECK(sched::logger_break(zero, 3, 0, 1.0, false, errs, [](int, float) {}) == 2 &&
              errs.size() == 3 && errs[2] == 0.0f,
          "prev norm 0: error 0, a break at k = 2");
}

// the errors are logger_error's own, bit for bit, for float and double sums
template <class T>
static void test_break_errors_are_logger_error() {
    const double npx = 64.0 * 48.0;
    T sums[10] = {(T)3071.25, (T)0.0, (T)812.0625, (T)3071.25, (T)97.3125, (T)2977.5,
                  (T)3.1640625, (T)2981.75, (T)2.9765625, (T)2982.125};
    std::vector<float> errs;
    const int t = sched::logger_break(sums, 5, 0, npx, false, errs, [](int, float) {});
    CHECK(t == 4, "the last of these errors is below the threshold (got %d)", t);
    CHECK(errs.size() == 5, "five errors");
    for (size_t i = 0; i < errs.size(); i++)
        CHECK(bits(errs[i]) == bits(of2d::logger_error(sums[2 * i], sums[2 * i + 1], npx)),
              "error %zu is logger_error of the same sums", i);
    // the reference's formula in float (Logger.cpp:37-39), restated
    for (size_t i = 0; i < errs.size(); i++) {
        const float n = (float)npx, pn = (float)sums[2 * i + 1] / n, dn = (float)sums[2 * i] / n;
        CHECK(bits(errs[i]) == bits(pn == 0 ? 0.0f : dn / pn), "error %zu is (diff / n) / (prev / n) "
              "in float", i);
    }
}

int main() {
    test_plan_fused();
    test_ring<12>();
    test_ring<15>();
    test_plan_blocks();
    test_break_thresholds<float>();
    test_break_thresholds<double>();
    test_break_errors_are_logger_error<float>();
    test_break_errors_are_logger_error<double>();
    std::printf("iter_schedule_test: %d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
