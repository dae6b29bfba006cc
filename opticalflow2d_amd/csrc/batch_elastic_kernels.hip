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
//      dI.y) (OpticalFlow.cpp:15-39, the floats of sor_pack_kernel) into the
//      pair's slice of the scratch plane f, and u_out <- u_in: the sweep never
//      writes the border, which keeps its values
//   2. the SOR sweep in place on u_out, in the reference's order.  The
//      reference relaxes i-outer, j-inner, so pixel (i, j) reads NEW values at
//      (i-1, j-1), (i-1, j), (i-1, j+1), (i, j-1) and OLD ones at (i, j+1) and
//      (i+1, .): every pixel with 2 i + j = t depends on smaller t only.  Step
//      t relaxes them all, thread tid the columns tid, tid + T, ... that have
//      an interior row j = t - 2 i at this step (batch_plan.h, elastic_col_lo /
//      _hi), with the per-pixel arithmetic of sor_px.h.  A step's pixels are no
//      neighbours of each other, so the order inside a step is free; between
//      steps stands one workgroup barrier, which a level of one wave (dx <= 64)
//      does not need: the wave's loads and stores reach memory in program
//      order
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

#include "sor_px.h"

namespace of2d {
namespace batch {

namespace {
// what orders a stage or a sweep step before the next.  One wave: its lanes
// exchange values through memory, which its vector-memory instructions reach in
// program order; the wavefront-scope fences keep the compiler from moving a
// load across the stores of the step before it, and cost no instruction
template <int WAVES>
__device__ __forceinline__ void step_sync() {
    if constexpr (WAVES == 1) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}
}  // namespace

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
            const float sc = (It[o] + m.x * g.x) + m.y * g.y;
            f[o] = make_float2(g.x * sc, g.y * sc);
            dst[o] = m;
        });
        step_sync<WAVES>();
        for (int t = kElasticFirstStep; t <= tlast; ++t) {
            const int lo = elastic_col_lo(t, dy), hi = elastic_col_hi(t, dx);
            for (int i = elastic_first_col(tid, lo, T); i <= hi; i += T) {
                const int j = t - 2 * i;  // interior: 1 <= j <= dy - 2
                const float2 *c = dst + (long)j * P + i;
                const float2 nw = sor_px(k, c[0], f[(long)j * P + i], c[-1], c[1], c[P], c[-P],
                                         c[P - 1], c[-P - 1], c[P + 1], c[-P + 1]);
                dst[(long)j * P + i] = nw;
            }
            step_sync<WAVES>();
        }
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

namespace {
template <int WAVES>
void launch_waves(const ElasticLoopArgs &a, int B, bool conv, hipStream_t st) {
    if (conv)
        hipLaunchKernelGGL((elastic_loop_kernel<WAVES, true>), dim3(B), dim3(64 * WAVES), 0, st, a);
    else
        hipLaunchKernelGGL((elastic_loop_kernel<WAVES, false>), dim3(B), dim3(64 * WAVES), 0, st,
                           a);
}
}  // namespace

void launch_elastic_loop(const ElasticLoopArgs &a, int B, bool conv, hipStream_t st) {
    static_assert(kElasticMaxWaves == 8, "one instantiation per workgroup size below");
    switch (elastic_waves(a.dx)) {
        case 1: launch_waves<1>(a, B, conv, st); break;
        case 2: launch_waves<2>(a, B, conv, st); break;
        case 3: launch_waves<3>(a, B, conv, st); break;
        case 4: launch_waves<4>(a, B, conv, st); break;
        case 5: launch_waves<5>(a, B, conv, st); break;
        case 6: launch_waves<6>(a, B, conv, st); break;
        case 7: launch_waves<7>(a, B, conv, st); break;
        default: launch_waves<8>(a, B, conv, st); break;
    }
    OF2D_HIP(hipGetLastError());
}

}  // namespace batch
}  // namespace of2d
