// iter_schedule.h — the iteration schedule of the Logger loops (host only, no
// HIP): which buffer an iteration reads and writes, how a chunk is cut into
// launches, when a break needs a replay, and the break test itself.  The one
// definition for Registration's loops (registration.cpp, solvers.cpp) and the
// slab's (slab.cpp): the multi-rank path is bit-identical to one GPU because
// both walk the same schedule.  tests/host/iter_schedule_test.cpp checks every
// rule below on a CPU.
#pragma once

#include <algorithm>
#include <vector>

namespace of2d {

// Per-iteration Logger norms -> error, exactly the reference's float formula
// (Logger.cpp:37-39, Motion.cpp:47) applied to fp64 sums (the float sums of
// the exact Logger widen exactly).
inline float logger_error(double sum_diff, double sum_prev, double npx) {
    const float n = (float)npx;
    const float prevnorm = (float)sum_prev / n;
    const float diffnorm = (float)sum_diff / n;
    return prevnorm == 0 ? 0.0f : diffnorm / prevnorm;
}

namespace sched {

// ------------------------------------------------------ three-buffer rotation
// Single steps of a chunk that starts in buffer a (0..2): iteration t reads
// single_src(a, t) and writes single_dst(a, t), alternating between the two
// buffers other than a, which is never written inside the chunk.
constexpr int single_src(int a, int t) {
    return t == 0 ? a : (t % 2 == 1 ? (a + 1) % 3 : (a + 2) % 3);
}
constexpr int single_dst(int a, int t) { return t % 2 == 0 ? (a + 1) % 3 : (a + 2) % 3; }
// of the two buffers that are not a, the one that is not b (b == a: the second)
constexpr int other(int a, int b) { return b == (a + 1) % 3 ? (a + 2) % 3 : (a + 1) % 3; }

// ----------------------------------------------------------------- fused plan
// One launch of a chunk: iterations [t, t + K) in one pass from buffer `in`
// to buffer `out` (K = 1: a single step)
struct Launch {
    int K, t, in, out;
};
struct FusedPlan {
    std::vector<Launch> launches;
    int end;  // the buffer holding the chunk's last iterate (a when C == 0)
};
// The launches of a chunk of C iterations from buffer a.  With pairs: triples
// while three iterations remain (if triples), then a pair or a single for the
// tail, alternating between the two buffers other than a.  Without: the single
// steps of the rotation above.  With quads (the unsplit fixed-iteration run,
// which takes no break and replays nothing): four iterations per launch while
// four remain, then the same triple, pair or single for the tail.
inline FusedPlan plan_fused(int a, int C, bool triples, bool pairs, bool quads = false) {
    FusedPlan p;
    p.end = a;
    p.launches.reserve((size_t)std::max(C, 0));  // one allocation: the loops plan every chunk
    for (int t = 0; t < C;) {
        const int K = !pairs ? 1
                      : quads && C - t >= 4 ? 4
                      : triples && C - t >= 3 ? 3
                                              : std::min(2, C - t);
        const int out = pairs ? other(a, p.end) : single_dst(a, t);
        p.launches.push_back({K, t, p.end, out});
        p.end = out;
        t += K;
    }
    return p;
}
// Iterations per chunk of a fixed-iteration run.  It has no break to replay, so
// a chunk only sets how often the partial rows are reduced: 33 triples, or 25
// quads (1000 iterations: ten whole chunks, no tail).
constexpr int fixed_chunk(bool quads) { return quads ? 100 : 99; }
// A break at chunk-local iteration t of C: is iterate t + 1 gone from
// single_dst(a, t)?  Fused launches never wrote it there; single steps
// overwrote it with iterate t + 3.  The replay runs single steps 0..t from a.
constexpr bool fused_replay_needed(bool pairs, int t, int C) { return pairs || t + 2 <= C - 1; }

// ----------------------------------------------------------------------- ring
// The exact Logger keeps every iterate in memory for its norms: R buffers
// besides the chunk's start buffer a (0..R), which is kept for a replay.
template <int R>
struct Ring {
    // iteration t writes the (t mod R)-th buffer other than a
    static constexpr int ring(int a, int t) { return t % R < a ? t % R : t % R + 1; }
    // and reads the previous iteration's
    static constexpr int src(int a, int t) { return t == 0 ? a : ring(a, t - 1); }
    // a break at chunk-local t of C: iteration t + R reused iteration t's buffer
    static constexpr bool replay_needed(int t, int C) { return t + R <= C - 1; }
    // the pipelined loop never leaves buffer 0: iterate 0 in buffer 0, iterate
    // j >= 1 in buffer 1 + (j - 1) mod R
    static constexpr int slot(int j) { return src(0, j); }
};

// --------------------------------------------------- pipelined loop's blocks
// Iterations per host decision block: cb rounded up to whole triples, and few
// enough groups that no event of a block being read is recorded again before
// it is (events: the event ring's length, in_flight: blocks enqueued at once)
constexpr int pipelined_block(int cb, int events, int in_flight) {
    return std::min(3 * ((cb + 2) / 3), 3 * (events / in_flight - 4));
}
struct Block {
    int lo, hi;  // iterations [lo, hi)
    bool tail;   // the one or two single steps after the last whole triple
};
// niter iterations as blocks of at most blk (a multiple of three) iterations
// in whole triples, then the tail of niter % 3 iterations as a block of its own
inline std::vector<Block> plan_blocks(int niter, int blk) {
    std::vector<Block> b;
    const int ntrip = niter / 3 * 3;
    for (int lo = 0; lo < ntrip; lo += blk) b.push_back({lo, std::min(lo + blk, ntrip), false});
    if (niter > ntrip) b.push_back({ntrip, niter, true});
    return b;
}

// ------------------------------------------------------------------ the break
// The errors of a chunk's C iterations (k0: the chunk's first; sums: {diff,
// prev} per iteration, fp64 partial sums or the exact Logger's floats) onto
// errs, each reported to on_error(k, err); returns the chunk-local iteration
// whose error takes the reference's break, or -1 (always -1 when fixed: a
// fixed_iters run reads its errors and takes no break).
template <class T, class OnError>
int logger_break(const T *sums, int C, int k0, double npx, bool fixed, std::vector<float> &errs,
                 OnError &&on_error) {
    for (int t = 0; t < C; t++) {
        const int k = k0 + t;
        const float err = logger_error(sums[2 * t], sums[2 * t + 1], npx);
        errs.push_back(err);
        on_error(k, err);
        if (!fixed && err < 0.001f && k > 1) return t;  // ImageRegistrationOpticalFlow.cpp:131-134
    }
    return -1;
}

}  // namespace sched
}  // namespace of2d
