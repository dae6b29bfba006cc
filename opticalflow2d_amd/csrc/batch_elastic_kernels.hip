// batch_elastic_kernels.hip — B independent Elastic registrations of one size
// (of2d_batch.h): the whole loop of
// OpticalFlowElastic::get_update (OpticalFlowElastic.cpp:13-19) for one pair in
// one workgroup, where the one-pair path takes a pack, a sweep of one wave per
// 63-column strip with hand-offs through memory, and a Logger pass per
// iteration (solvers.cpp, loop_elastic).
//
// An iteration, the iterate ping-ponging between the pair's two buffers as in
// the other loops (iteration t reads u[t & 1]):
//   1. force and copy, in for_pixels order: b = dI * ((It + u.x dI.x) + u.y
//      dI.y) (OpticalFlow.cpp:15-39; force_px's lines, sor_px.h) into the
//      pair's slice of the scratch plane f, and u_out <- u_in: the sweep never
//      writes the border, which keeps its values
//   2. the SOR sweep in place on u_out in the reference's order (sor_sweep,
//      batch_sweep.h, which the Fluid loop runs on its velocity): step t
//      relaxes every pixel with 2 i + j = t, which read NEW values of smaller
//      t and OLD ones of larger t only (batch_plan.h, sor_px.h).  A step's
//      pixels are no neighbours of each other, so the order inside a step is
//      free; between steps stands step_sync
//   3. with convergence on, the fp64 Logger sums of (u_out - u_in) and u_in in
//      for_pixels order, block_sums and the decision, as hs_loop_kernel's
//
// No workgroup waits for another and nothing polls.  Every barrier is reached
// by all threads: the step count depends on the level only, and the break goes
// through LDS (loop_break).  Entry, convergence, break and exit are the loop
// frame's (batch_loop.h); Elastic has no division, so no pair ever fails.
// Compiled with -ffp-contract=off: the iterates are the one-pair path's and
// the oracle's bit for bit.
#include "of2d_batch.h"

#include "batch_sweep.h"

namespace of2d {
namespace batch {

template <int WAVES, bool CONV>
__global__ __launch_bounds__(64 * WAVES) void elastic_loop_kernel(ElasticLoopArgs a) {
    constexpr int T = 64 * WAVES;
    const long pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    PairSlots ps;
    if (!loop_entry<CONV>(a, pair, tid, ps)) return;
    float2 *u0 = a.u0 + pair * a.stride, *u1 = a.u1 + pair * a.stride;
    const float2 *__restrict__ dI = a.dI + pair * a.stride;
    const float *__restrict__ It = a.It + pair * a.stride;
    float2 *f = a.f + pair * a.stride;
    const int dx = a.dx, dy = a.dy, P = a.P, npx = dx * dy;
    const int tlast = elastic_last_step(dx, dy);
    const SorCoef k = a.k;
    __shared__ int s_stop;
    int n = 0;
    for (int it = 0; it < a.niter; ++it) {
        const float2 *src = (it & 1) ? u1 : u0;
        float2 *dst = (it & 1) ? u0 : u1;
        for_pixels<T>(tid, npx, dx, P, [&](int, int, int, long o) {
            const float2 m = src[o], g = dI[o];
            // force_px's lines (sor_px.h), kept: the call moves the kernel's code
            const float sc = (It[o] + m.x * g.x) + m.y * g.y;
            f[o] = make_float2(g.x * sc, g.y * sc);
            dst[o] = m;
        });
        step_sync<WAVES>();
        sor_sweep<WAVES>(dst, f, k, dx, dy, P, tid, tlast);
        n = it + 1;
        if constexpr (CONV) {
            double v[2] = {0.0, 0.0};
            for_pixels<T>(tid, npx, dx, P,
                          [&](int, int, int, long o) { logger_add(dst[o], src[o], v[0], v[1]); });
            block_sums<2, WAVES>(v, wave, lane);
            if (tid == 0) s_stop = loop_decide(v[0], v[1], ps, it);
        }
        if (loop_break<CONV>(s_stop)) break;
    }
    loop_exit(a, pair, tid, lane, ps, n, 0);
}

void launch_elastic_loop(const ElasticLoopArgs &a, int B, bool conv, hipStream_t st) {
    launch_by_waves(a, B, st, [conv](auto w) -> void (*)(ElasticLoopArgs) {
        constexpr int W = decltype(w)::value;
        return conv ? elastic_loop_kernel<W, true> : elastic_loop_kernel<W, false>;
    });
}

}  // namespace batch
}  // namespace of2d
