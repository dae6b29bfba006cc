// batch_plan.h — the host arithmetic of the batch's boundary copies and of its
// analysis calls (batch.cpp, capi.cpp) that needs no device: the staging
// rounds, a pair's offsets in them, and the argument checks.  Plain C++ (no
// HIP header), so that tests/host/batch_plan_test.cpp exercises it on the CPU,
// with sanitizers too.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace of2d {
namespace batch {

// pairs per staging round of the boundary copies: the staging buffer holds two
// doubles per pixel (a motion field) of that many pairs, 64 MiB at most
inline size_t stage_chunk_pairs(int nbatch, int dimx, int dimy) {
    const size_t n0 = (size_t)dimx * (size_t)dimy;
    return std::min<size_t>((size_t)nbatch, std::max<size_t>(1, ((size_t)8 << 20) / (2 * n0)));
}

// One staging round: pairs [k0, k0 + nk); their first element in the pitched
// fields (field), in a host stack of images (image) and of planar motion
// fields (motion)
struct StageRound {
    int k0 = 0, nk = 0;
    long field = 0;
    size_t image = 0, motion = 0;
};
// the rounds that move npairs pairs through a staging buffer of stage_pairs,
// in ascending order, every pair exactly once; stride: pair_stride(dimx, dimy)
inline std::vector<StageRound> stage_rounds(int npairs, size_t stage_pairs, long stride, int dimx,
                                            int dimy) {
    std::vector<StageRound> v;
    if (npairs < 1 || stage_pairs < 1) return v;
    const size_t n0 = (size_t)dimx * (size_t)dimy;
    const int step = (int)std::min<size_t>(stage_pairs, (size_t)npairs);
    for (int k0 = 0; k0 < npairs; k0 += step) {
        StageRound r;
        r.k0 = k0;
        r.nk = std::min(step, npairs - k0);
        r.field = (long)k0 * stride;
        r.image = (size_t)k0 * n0;
        r.motion = (size_t)k0 * 2 * n0;
        v.push_back(r);
    }
    return v;
}

// nullptr or why the call is refused (the one-pair entries' wording)
inline const char *jacobian_refusal(int dimx, int dimy) {
    if (dimx < 2 || dimy < 2) return "jacobian: the field needs dimx >= 2 and dimy >= 2";
    return nullptr;
}
inline const char *invert_refusal(int dimx, int dimy, int max_iter, double tol) {
    if (dimx < 2 || dimy < 2) return "invert: the field needs dimx >= 2 and dimy >= 2";
    if (max_iter < 1) return "invert: max_iter < 1";
    if (!std::isfinite(tol) || tol <= 0.0) return "invert: tol must be finite and > 0";
    return nullptr;
}

}  // namespace batch
}  // namespace of2d
