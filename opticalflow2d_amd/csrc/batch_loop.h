// batch_loop.h — the frame the batch's seven loop kernels share (hs_loop_kernel,
// hs_resident_kernel, demons_loop_kernel, demons_lds_kernel, curv_loop_kernel,
// elastic_loop_kernel, fluid_loop_kernel).
//
// One workgroup of kLoopThreads (Curvature: kCurvThreads; Elastic and Fluid:
// elastic_threads(dx)) runs the whole loop of pair blockIdx.x:
//   entry   loop_entry: the pair's iters and errs slots; a pair whose status
//           has kStatusDivZero from an earlier loop runs nothing and reports 0
//           iterations
//   body    the kernel's own stages, thread t on pixels t, t + T, ... in
//           ascending linear index (for_pixels), then with CONV the fp64
//           Logger sums of (u' - u) and u in that order and block_sums
//   decide  thread 0: s_stop = loop_decide(...), logger_error's float
//           arithmetic and the reference's break (err < 0.001f && iteration >
//           1, ImageRegistrationOpticalFlow.cpp:131-134).  These are fp64 sums
//           (the "logger_fp64" semantics of the one-pair path), not the
//           reference's float running sum: an error can differ from the
//           reference's in its last bits, and a break that hangs on them can
//           fall one iteration apart
//   break   loop_break: the barrier that completes the iterate and publishes
//           the decision; without CONV exactly niter iterations run
//   exit    loop_exit: the iteration count, and kStatusDivZero for a pair of
//           which a thread met a zero denominator (bad != 0; coord2d.h:95-100),
//           one atomicOr per wave
// All of it is force-inlined: the kernels compile to what their own copies did.
// The sweep that elastic_loop_kernel and fluid_loop_kernel run in their body,
// with what orders its steps, is batch_sweep.h.
#pragma once

#include "of2d_device.h"

namespace of2d {
namespace batch {

// what every loop launch takes, whatever the regulariser
struct LoopCommon {
    float2 *u0, *u1;   // the iterate's two buffers; iteration t reads u[t & 1]
    unsigned *status;  // [B]
    int *iters;        // [B][nloops]: iterations run by this loop
    float *errs;       // [B][nloops][maxn] (convergence on)
    long stride;
    int dx, dy, P, niter;
    int nloops, loop, maxn;
};

struct PairSlots {
    int *iters;
    float *errs;  // nullptr without CONV
    float nf;     // logger_error: (float)npx
};
// false: the pair failed in an earlier loop; the kernel returns at once
template <bool CONV>
__device__ __forceinline__ bool loop_entry(const LoopCommon &a, long pair, int tid, PairSlots &p) {
    p.iters = a.iters + pair * a.nloops + a.loop;
    if (a.status[pair] & kStatusDivZero) {
        if (tid == 0) *p.iters = 0;
        return false;
    }
    p.errs = CONV ? a.errs + (pair * a.nloops + a.loop) * (long)a.maxn : nullptr;
    p.nf = (float)(double)(a.dx * a.dy);
    return true;
}

// logger_error (registration.cpp) on the device, by one thread, from the
// block's sums: records iteration it's error and returns the stop flag
__device__ __forceinline__ int loop_decide(double diff, double prev, const PairSlots &p, int it) {
    const float prevnorm = (float)prev / p.nf;
    const float diffnorm = (float)diff / p.nf;
    const float err = prevnorm == 0 ? 0.0f : diffnorm / prevnorm;
    p.errs[it] = err;
    return (err < 0.001f && it > 1) ? 1 : 0;
}

// the iterate is complete (and the decision published) for every thread;
// true: the pair leaves the loop
template <bool CONV>
__device__ __forceinline__ bool loop_break(const int &s_stop) {
    __syncthreads();
    if constexpr (CONV) return s_stop != 0;
    return false;
}

__device__ __forceinline__ void loop_exit(const LoopCommon &a, long pair, int tid, int lane,
                                          const PairSlots &p, int n, int bad) {
    if (tid == 0) *p.iters = n;
    if (__any(bad) && lane == 0) atomicOr(a.status + pair, kStatusDivZero);
}

// f(idx, i, j, o) for the thread's pixels of a dx-wide image at pitch P:
// idx = tid, tid + T, ... below npx, (i, j) the pixel, o = j * P + i
template <int T, class F>
__device__ __forceinline__ void for_pixels(int tid, int npx, int dx, int P, F &&f) {
    for (int idx = tid; idx < npx; idx += T) {
        const int j = idx / dx, i = idx - j * dx;
        f(idx, i, j, (long)j * P + i);
    }
}

}  // namespace batch
}  // namespace of2d
