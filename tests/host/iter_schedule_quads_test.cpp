// Stand-alone check of the quad schedule in opticalflow2d_amd/csrc/
// iter_schedule.h (plan_fused with quads, fixed_chunk): host only, beside
// iter_schedule_test.cpp and in its style — every property is stated in words
// and checked by simulating what the plan does to the buffers.
// tests/test_iter_schedule_quads.py compiles and runs it.
#include <cstdio>

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

static void test_plan_quads() {
    for (int a = 0; a < 3; a++)
        for (int C = 0; C <= 120; C++) {
            const sched::FusedPlan p = sched::plan_fused(a, C, true, true, true);
            int t = 0, prev_out = a, nquads = 0;
            int holds[3] = {-1, -1, -1};  // the iterate each buffer holds
            holds[a] = 0;
            for (const sched::Launch &l : p.launches) {
                CHECK(l.t == t, "t values are consecutive from 0 (a %d C %d)", a, C);
                CHECK(l.in == prev_out, "a launch reads what the previous one wrote, the first "
                      "reads a (a %d C %d t %d)", a, C, l.t);
                CHECK(l.out >= 0 && l.out < 3 && l.out != a,
                      "the start buffer is never written (a %d C %d t %d)", a, C, l.t);
                CHECK(l.out != l.in, "no launch runs in place (a %d C %d t %d)", a, C, l.t);
                const int left = C - t;
                const int want = left >= 4 ? 4 : left;
                CHECK(l.K == want, "K = 4 while four remain, then the triple, pair or single step "
                      "that ends the chunk (a %d C %d t %d: K %d)", a, C, l.t, l.K);
                CHECK(holds[l.in] == t, "a launch reads iterate t (a %d C %d t %d)", a, C, t);
                nquads += l.K == 4;
                t += l.K;
                holds[l.out] = t;
                prev_out = l.out;
            }
            CHECK(t == C, "the K values sum to C (a %d C %d: %d)", a, C, t);
            CHECK(nquads == C / 4 && (int)p.launches.size() == C / 4 + (C % 4 != 0),
                  "C / 4 quads and at most one tail launch (a %d C %d)", a, C);
            CHECK(p.end == prev_out, "the end buffer is the last out (a %d C %d)", a, C);
            CHECK(holds[p.end] == C && holds[a] == 0,
                  "the end buffer holds iterate C, a its start state (a %d C %d)", a, C);
            // without quads the flag changes nothing
            const sched::FusedPlan q = sched::plan_fused(a, C, true, true, false);
            const sched::FusedPlan q0 = sched::plan_fused(a, C, true, true);
            bool same = q.launches.size() == q0.launches.size() && q.end == q0.end;
            for (size_t i = 0; same && i < q.launches.size(); i++)
                same = q.launches[i].K == q0.launches[i].K && q.launches[i].t == q0.launches[i].t &&
                       q.launches[i].in == q0.launches[i].in &&
                       q.launches[i].out == q0.launches[i].out && q.launches[i].K <= 3;
            CHECK(same, "quads off is the plan of triples (a %d C %d)", a, C);
        }
}

static void test_fixed_chunk() {
    CHECK(sched::fixed_chunk(true) % 4 == 0, "a quad chunk is whole quads");
    CHECK(sched::fixed_chunk(false) % 3 == 0, "a triple chunk is whole triples");
    CHECK(1000 % sched::fixed_chunk(true) == 0, "1000 iterations are whole quad chunks: no tail");
    // a run of n iterations in chunks: every chunk but the last is whole quads
    for (int n = 1; n <= 1100; n++) {
        int tails = 0, a = 0, done = 0;
        for (int k0 = 0; k0 < n; k0 += sched::fixed_chunk(true)) {
            const int C = n - k0 < sched::fixed_chunk(true) ? n - k0 : sched::fixed_chunk(true);
            const sched::FusedPlan p = sched::plan_fused(a, C, true, true, true);
            for (const sched::Launch &l : p.launches) {
                tails += l.K != 4;
                done += l.K;
            }
            a = p.end;
        }
        CHECK(done == n && tails == (n % 4 != 0), "one tail launch at most in a run (n %d)", n);
    }
}

int main() {
    test_plan_quads();
    test_fixed_chunk();
    std::printf("%d checked, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
