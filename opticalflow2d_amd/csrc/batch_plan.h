// batch_plan.h — the host arithmetic of the batch's boundary copies and of its
// analysis calls (batch.cpp, capi.cpp) that needs no device: the staging
// rounds, a pair's offsets in them, the argument checks, the fit rules of the
// loop's on-CU placements with the instantiation a level runs, and what each
// kind of loop needs of the driver (LoopKind).  Plain C++ (no
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

// ---- the loop's workgroup and its two on-CU placements (DESIGN.md §4.6.5,
// §4.6.6).  waves of a pair's workgroup in the loop kernels (1024 threads at
// every level)
constexpr int kLoopWaves = 16;
constexpr int kLoopThreads = 64 * kLoopWaves;
// A level runs on the CU when one predicate on its size holds: its float2
// elements in LDS (8 bytes each; the kernels assert it) plus
// kResidentLdsReserve bytes for the kernel's static LDS (block_sums' scratch
// and the flags) fit the CU's 160 KiB, and a thread of the 1024 owns at most
// as many pixels as the largest instantiation holds.  Batch::estimate chooses
// the kernel by it and Batch::info reports it (placement 1).
constexpr int kResidentLdsBudget = 160 * 1024;
constexpr int kResidentLdsReserve = 1024;
constexpr size_t kLdsElementBytes = 8;
inline bool on_cu_fits(int dx, int dy, size_t lds_bytes, int max_ppt) {
    return dx >= 1 && dy >= 1 && lds_bytes + kResidentLdsReserve <= (size_t)kResidentLdsBudget &&
           (long)dx * dy <= (long)max_ppt * kLoopThreads;
}
// pixels of a thread that owns the most
inline int loop_ppt(int dx, int dy) {
    return (int)(((long)dx * dy + kLoopThreads - 1) / kLoopThreads);
}

// option "resident": the iterate's one LDS copy, (dx + 2) x (dy + 2) with its
// ghost ring; dI, It and the new values of 16 pixels are 80 of the 128
// registers a lane of such a workgroup may have.  Every level up to 128 x 128
// fits (135 200 B, 16 pixels); 150 x 120 fails on the pixels and 2 x 6000 on
// the bytes
constexpr int kResidentMaxPpt = 16;
inline size_t resident_lds_bytes(int dx, int dy) {
    return (size_t)(dx + 2) * (size_t)(dy + 2) * kLdsElementBytes;
}
inline bool resident_fits(int dx, int dy) {
    return on_cu_fits(dx, dy, resident_lds_bytes(dx, dy), kResidentMaxPpt);
}
// the instantiation of hs_resident_kernel a fitting level runs
inline int resident_ppt(int dx, int dy) {
    const int p = loop_ppt(dx, dy);
    return p <= 1 ? 1 : p <= 2 ? 2 : p <= 4 ? 4 : p <= 8 ? 8 : kResidentMaxPpt;
}

// option "conv_lds": the dense plane, dx * dy pixels at pitch dx without ghost
// lines plus dx + 1 zeroed elements that accumulate_px's unconditional b[1],
// b[P], b[P + 1] loads reach from the last pixels; the new values of 16 pixels
// are 32 registers.  Every level up to 128 x 128 fits (132 104 B); 129 x 128
// fails on the pixels
constexpr int kConvLdsMaxPpt = 16;
inline size_t conv_lds_bytes(int dx, int dy) {
    return ((size_t)dx * (size_t)dy + (size_t)dx + 1) * kLdsElementBytes;
}
inline bool conv_lds_fits(int dx, int dy) {
    return on_cu_fits(dx, dy, conv_lds_bytes(dx, dy), kConvLdsMaxPpt);
}
// the instantiation of demons_lds_kernel a fitting level runs
inline int conv_lds_ppt(int dx, int dy) {
    const int p = loop_ppt(dx, dy);
    return p <= 1 ? 1 : p <= 4 ? 4 : kConvLdsMaxPpt;
}

// ---- the Curvature loop (batch_curvature_kernels.hip).
// Both sides of every level are a fast-transform length: a power of two in
// [kCurvNMin, kCurvNMax] (OF2D_DCT_NMIN, OF2D_BATCH_CURV_NMAX)
// A pair's workgroup is kCurvThreads, half the other loops': a chunk of lines
// (below) is 512 radix-4 butterflies per pass, one per thread
constexpr int kCurvWaves = 8;
constexpr int kCurvThreads = 64 * kCurvWaves;
constexpr int kCurvNMin = 8;
constexpr int kCurvNMax = 512;
inline bool curv_side_ok(int n) {
    return n >= kCurvNMin && n <= kCurvNMax && (n & (n - 1)) == 0;
}
inline bool curv_level_ok(int dx, int dy) { return curv_side_ok(dx) && curv_side_ok(dy); }
// A pair's fp64 scratch at a level: the plane pair x | y, dense (element
// (i, j) of a plane at i + j * dx), 16 B per pixel; no transposed copy
inline size_t curv_scratch_doubles(int dx, int dy) { return 2 * (size_t)dx * (size_t)dy; }
// A pass along an axis moves its lines through LDS in chunks of whole lines, a
// line of n elements being n double2 points (16 B each: n/2 complex points per
// plane).  A chunk holds at most kCurvChunkPoints points of lines, that is
// kCurvPointsPerThread per thread: dct_inv_pre keeps a thread's points in
// registers across its barrier, and more of them (8 were tried) cost more
// registers than a lane has.  The lines are spread evenly over the fewest
// chunks that allows.  In LDS a line is followed by kCurvLinePad unused
// points: along y a wave's lanes walk across the chunk's columns, and a line
// stride of n points would put them all on one bank.  The largest chunk, 256
// lines of 8, is 36 KiB: within the 64 KiB a launch gets without asking
constexpr size_t kCurvPointBytes = 16;
constexpr int kCurvLinePad = 1;
constexpr int kCurvPointsPerThread = 4;
constexpr int kCurvChunkPoints = kCurvPointsPerThread * kCurvThreads;
inline int curv_chunks(int n, int nlines) {
    const int most = kCurvChunkPoints / n;  // lines that fit
    return (nlines + most - 1) / most;
}
inline int curv_chunk_lines(int n, int nlines) {
    const int c = curv_chunks(n, nlines);
    return (nlines + c - 1) / c;
}
inline size_t curv_chunk_bytes(int n, int nlines) {
    return (size_t)curv_chunk_lines(n, nlines) * (size_t)(n + kCurvLinePad) * kCurvPointBytes;
}
// dynamic LDS of a level's launch: the larger of its two axes' chunks (lines
// along x: dx long, dy of them; along y: dy long, dx of them)
inline size_t curv_lds_bytes(int dx, int dy) {
    return std::max(curv_chunk_bytes(dx, dy), curv_chunk_bytes(dy, dx));
}

// ---- the Elastic loop (batch_elastic_kernels.hip).  The
// SOR sweep relaxes i-outer, j-inner in place, so pixel (i, j) depends on
// pixels of smaller 2 i + j only and every pixel with 2 i + j = t can be
// relaxed at once: step t of the sweep.  A pair's workgroup has one thread per
// column up to kElasticMaxWaves waves; in a wider level thread tid takes the
// columns tid, tid + T, ...  (constexpr: the kernel calls these too)
constexpr int kElasticMaxWaves = 8;
constexpr int elastic_waves(int dx) {
    const int w = (dx + 63) / 64;
    return w < 1 ? 1 : (w > kElasticMaxWaves ? kElasticMaxWaves : w);
}
constexpr int elastic_threads(int dx) { return 64 * elastic_waves(dx); }
// the sweep's steps are t = kElasticFirstStep (pixel (1, 1)) ...
// elastic_last_step (pixel (dx - 2, dy - 2)); none when a side is below 3
constexpr int kElasticFirstStep = 3;
constexpr int elastic_last_step(int dx, int dy) {
    return (dx < 3 || dy < 3) ? kElasticFirstStep - 1 : 2 * (dx - 2) + (dy - 2);
}
// the columns with an interior row at step t: 1 <= t - 2 i <= dy - 2 and
// 1 <= i <= dx - 2, that is [elastic_col_lo, elastic_col_hi] (empty when lo > hi)
constexpr int elastic_col_lo(int t, int dy) {
    const int lo = (t - dy + 3) >> 1;  // ceil((t - (dy - 2)) / 2), an arithmetic shift
    return lo < 1 ? 1 : lo;
}
constexpr int elastic_col_hi(int t, int dx) {
    const int hi = (t - 1) >> 1;
    return hi > dx - 2 ? dx - 2 : hi;
}
// thread tid's first column at or after lo: the next ones are T further on
constexpr int elastic_first_col(int tid, int lo, int T) {
    const int r = tid - lo % T;
    return lo + (r < 0 ? r + T : r);
}

// ---- what a kind of loop needs of the driver (batch.cpp): the one place that
// knows.  The kind follows from of2d_batch_create's method (0 Diffusion, 1
// Curvature, 2 Elastic, 3 Thirion's Demons) and option "fluid" of an Elastic batch
enum class LoopKind { HornSchunck, Curvature, Elastic, Fluid, Demons };
constexpr LoopKind loop_kind(int reg, bool fluid) {
    if (reg == 2) return fluid ? LoopKind::Fluid : LoopKind::Elastic;
    return reg == 3 ? LoopKind::Demons : reg == 1 ? LoopKind::Curvature : LoopKind::HornSchunck;
}
// Elastic's sweep, which Fluid runs on its velocity: the force plane, elastic_threads
constexpr bool loop_sweeps(LoopKind k) { return k == LoopKind::Elastic || k == LoopKind::Fluid; }
// threads of a pair's workgroup at a dx-wide level (Batch::info)
constexpr int loop_threads(LoopKind k, int dx) {
    if (loop_sweeps(k)) return elastic_threads(dx);
    return k == LoopKind::Curvature ? kCurvThreads : kLoopThreads;
}
// the gradients pass before a loop (Demons differentiates the image it warps
// itself), and with it a loop's launches: warp, gradients, loop, accumulate
constexpr bool loop_takes_gradients(LoopKind k) { return k != LoopKind::Demons; }
constexpr int loop_launches(LoopKind k) { return loop_takes_gradients(k) ? 4 : 3; }
// the on-CU option a handle of the kind admits (nullptr: none) and its fit rule
constexpr const char *on_cu_option(LoopKind k) {
    return k == LoopKind::HornSchunck ? "resident" : k == LoopKind::Demons ? "conv_lds" : nullptr;
}
inline bool on_cu_fits(LoopKind k, int dx, int dy) {
    if (k == LoopKind::HornSchunck) return resident_fits(dx, dy);
    return k == LoopKind::Demons && conv_lds_fits(dx, dy);
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
