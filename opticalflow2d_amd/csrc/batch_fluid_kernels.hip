// batch_fluid_kernels.hip — B independent viscous-fluid registrations of one
// size (of2d_batch.h): the whole loop of
// ImageRegistrationFluid::estimate_motion_at_current_resolution
// (ImageRegistrationFluid.cpp:94-125) with OpticalFlowFluid::get_update
// (OpticalFlowFluid.cpp:123-140) for one pair in one workgroup, the regrid
// included, where the one-pair path takes six or more launches per iteration
// and a host-mapped report (solvers.cpp, loop_fluid).
//
// The frame is the Elastic loop's (batch_elastic_kernels.hip): elastic_threads(dx)
// threads, global memory, the pair's slices only; the estimate ping-pongs
// between the pair's two buffers (iteration t reads u[t & 1] and writes the
// other).  An iteration, with a step_sync or a workgroup barrier between stages:
//   1. force, in for_pixels order: b = dI ((It + u.x dI.x) + u.y dI.y) of the
//      estimate u into the pair's slice of f
//   2. the SOR sweep of the pair's VELOCITY in place, the Elastic batch's
//      (sor_sweep, batch_sweep.h); the border is never written and stays 0
//   3. the increment R = (v - dudx v.x) - dudy v.y into f (the force is spent;
//      pixel o is written and read back by the same thread) and the workgroup's
//      maximum of Motion::maxabs' term; maxabs = sqrt(max), dt = 0.65f / maxabs
//   4. u' = u + R dt where dt < 65, else u, into the other buffer; with
//      convergence on the fp64 Logger sums of (u' - prev) and prev in
//      for_pixels order, block_sums
//   5. the workgroup's minimum of the Jacobian of u' (jacobian_px)
//   6. thread 0 decides: break when convergence is on, err < 0.001f and it > 1
//      (loop_decide); otherwise regrid when the minimum is below 0.5f; it writes
//      the iteration's record {maxabs, dt, jmin, regridded}.  Both decisions go
//      through LDS, so every barrier is reached by every thread
//   7. on a regrid: motion <- accumulate(motion, u') into the level's other
//      motion buffer (accumulate reads the old motion at interpolated
//      positions) with Iaux <- warp(Imov, motion); after a barrier the copy
//      back, so that the level's current buffer is one for all pairs, and dI,
//      It <- gradients(Iref, Iaux)
// After a regrid the next iteration reads its estimate as +0 while the
// buffer's content, the pre-regrid estimate, serves as the Logger's prev
// (Logger.cpp:45; fluid_zero_est of the one-pair loop).  prev is the buffer the
// iteration reads in every case: zero in a loop's first iteration.  When the
// last iteration run regridded, the estimate launch_accumulate then takes is
// zeroed, as loop_fluid leaves it.
//
// No workgroup waits for another, nothing polls, no flag lives in memory.
// Fluid has no division, so no pair ever fails.  Compiled with
// -ffp-contract=off: motion, counts and records are the one-pair path's and
// the oracle's bit for bit.
#include "of2d_batch.h"

#include "batch_sweep.h"
#include "field_px.h"
#include "fluid_px.h"

namespace of2d {
namespace batch {

// the stages read neighbours that other lanes wrote (the increment u, the
// Jacobian u', the gradients Iaux), a sweep step's pattern: step_sync orders them
template <int WAVES, bool CONV>
__global__ __launch_bounds__(64 * WAVES) void fluid_loop_kernel(FluidLoopArgs a) {
    constexpr int T = 64 * WAVES;
    const long pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    PairSlots ps;
    if (!loop_entry<CONV>(a, pair, tid, ps)) return;
    float2 *u0 = a.u0 + pair * a.stride, *u1 = a.u1 + pair * a.stride;
    float2 *dI = a.dI + pair * a.stride;
    float *It = a.It + pair * a.stride;
    float2 *f = a.f + pair * a.stride;
    float2 *vel = a.vel + pair * a.stride;
    float2 *mo = a.m_cur + pair * a.stride, *mn = a.m_other + pair * a.stride;
    const float *Iref = a.Iref + pair * a.sref;
    const float *Imov = a.Imov + pair * a.stride;
    float *Iaux = a.Iaux + pair * a.stride;
    float *log = a.log + (pair * a.nloops + a.loop) * (long)a.maxn * kFluidLogFloats;
    const int dx = a.dx, dy = a.dy, P = a.P, npx = dx * dy;
    const int tlast = elastic_last_step(dx, dy);
    const SorCoef k = a.k;
    const float2 zero = make_float2(0.0f, 0.0f);
    __shared__ int s_stop, s_regrid;
    __shared__ float s_max[WAVES], s_min[WAVES];
    int n = 0;
    bool zu = false;  // the estimate reads as +0: the iteration before regridded
    for (int it = 0; it < a.niter; ++it) {
        const float2 *src = (it & 1) ? u1 : u0;
        float2 *dst = (it & 1) ? u0 : u1;
        // 1. force
        for_pixels<T>(tid, npx, dx, P, [&](int, int, int, long o) {
            f[o] = force_px(zu ? zero : src[o], dI[o], It[o]);
        });
        step_sync<WAVES>();
        // 2. the sweep of the velocity
        sor_sweep<WAVES>(vel, f, k, dx, dy, P, tid, tlast);
        // 3. increment, maximum, time step
        float m = 0.0f;
        for_pixels<T>(tid, npx, dx, P, [&](int, int i, int j, long o) {
            const FluidGrad d =
                zu ? fluid_gradients_zero() : fluid_gradients_px(src, o, i, j, dx, dy, P);
            const float2 r = fluid_increment_px(vel[o], d);
            f[o] = r;
            m = fluid_maxabs_px(m, r);
        });
        m = wave_max(m);
        if (lane == 0) s_max[wave] = m;
        __syncthreads();
        m = s_max[0];
#pragma unroll
        for (int w = 1; w < WAVES; w++) m = (m < s_max[w]) ? s_max[w] : m;
        const float2 ts = fluid_timestep(m);  // {maxabs, dt}
        // 4. integrate, Logger sums
        double v[2] = {0.0, 0.0};
        for_pixels<T>(tid, npx, dx, P, [&](int, int, int, long o) {
            const float2 pv = src[o];
            const float2 un = fluid_integrate_px(zu ? zero : pv, f[o], ts.y);
            dst[o] = un;
            if constexpr (CONV) logger_add(un, pv, v[0], v[1]);
        });
        if constexpr (CONV)
            block_sums<2, WAVES>(v, wave, lane);  // its barrier completes u'
        else
            step_sync<WAVES>();
        // 5. the minimum Jacobian of u'
        float jm = __builtin_inff();
        for_pixels<T>(tid, npx, dx, P, [&](int, int i, int j, long) {
            const float q = jacobian_px(dst, i, j, dx, dy, P);
            jm = (q < jm) ? q : jm;
        });
        jm = wave_min(jm);
        if (lane == 0) s_min[wave] = jm;
        __syncthreads();
        // 6. decide and record
        n = it + 1;
        if (tid == 0) {
            jm = s_min[0];
#pragma unroll
            for (int w = 1; w < WAVES; w++) jm = (s_min[w] < jm) ? s_min[w] : jm;
            int stop = 0;
            if constexpr (CONV) stop = loop_decide(v[0], v[1], ps, it);
            const int rg = (!stop && jm < 0.5f) ? 1 : 0;
            s_stop = stop;
            s_regrid = rg;
            float *rec = log + (long)it * kFluidLogFloats;
            rec[0] = ts.x;
            rec[1] = ts.y;
            rec[2] = jm;
            rec[3] = rg ? 1.0f : 0.0f;
        }
        const bool brk = loop_break<CONV>(s_stop);
        zu = s_regrid != 0;
        if (brk) break;
        // 7. regrid
        if (zu) {
            for_pixels<T>(tid, npx, dx, P, [&](int, int i, int j, long o) {
                const float2 mv = accumulate_px(mo, dst[o], mo[o], i, j, dx, dy, P);
                mn[o] = mv;
                Iaux[o] = warp_px(Imov, mv, Imov[o], i, j, dx, dy, P);
            });
            step_sync<WAVES>();
            for_pixels<T>(tid, npx, dx, P, [&](int, int i, int j, long o) {
                mo[o] = mn[o];
                gradients_px(Iref, Iaux, dI, It, o, i, j, dx, dy, P);
            });
            step_sync<WAVES>();
        }
    }
    // the estimate after a regrid in the last iteration run is zero (a break
    // excludes a regrid); the regrid's reads of it lie before its last barrier
    if (zu) {
        float2 *last = (n & 1) ? u1 : u0;
        for_pixels<T>(tid, npx, dx, P, [&](int, int, int, long o) { last[o] = zero; });
    }
    loop_exit(a, pair, tid, lane, ps, n, 0);
}

void launch_fluid_loop(const FluidLoopArgs &a, int B, bool conv, hipStream_t st) {
    launch_by_waves(a, B, st, [conv](auto w) -> void (*)(FluidLoopArgs) {
        constexpr int W = decltype(w)::value;
        return conv ? fluid_loop_kernel<W, true> : fluid_loop_kernel<W, false>;
    });
}

}  // namespace batch
}  // namespace of2d
