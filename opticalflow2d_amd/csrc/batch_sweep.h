// batch_sweep.h — the SOR sweep the batch's Elastic and Fluid loops share
// (elastic_loop_kernel on the iterate, fluid_loop_kernel on the velocity;
// DESIGN.md §4.6.8): what orders two steps, the sweep (batch_plan.h's steps,
// sor_px.h's pixel; force-inlined), and the launch by a level's width.
#pragma once

#include <type_traits>

#include "batch_plan.h"
#include "of2d_device.h"
#include "sor_px.h"

namespace of2d {
namespace batch {

// what orders a stage or a sweep step before the next: lanes read what other
// lanes wrote.  One wave: its lanes exchange values through memory, which its
// vector-memory instructions reach in program order; the wavefront-scope
// fences keep the compiler from moving a load across the stores of the step
// before it, and cost no instruction
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

// one sweep in place on the dx x dy field x at pitch P with right-hand side f:
// steps kElasticFirstStep .. tlast = elastic_last_step(dx, dy), thread tid of
// 64 * WAVES the columns tid, tid + T, ... with an interior row at the step, a
// step_sync after every step; the border is never written.  The kernel passes
// tlast, evaluated before its iteration loop: evaluated here it moves its code
template <int WAVES>
__device__ __forceinline__ void sor_sweep(float2 *x, const float2 *f, const SorCoef &k, int dx,
                                          int dy, int P, int tid, int tlast) {
    constexpr int T = 64 * WAVES;
    for (int t = kElasticFirstStep; t <= tlast; ++t) {
        const int lo = elastic_col_lo(t, dy), hi = elastic_col_hi(t, dx);
        for (int i = elastic_first_col(tid, lo, T); i <= hi; i += T) {
            const int j = t - 2 * i;  // interior: 1 <= j <= dy - 2
            const float2 *c = x + (long)j * P + i;
            const float2 nw = sor_px(k, c[0], f[(long)j * P + i], c[-1], c[1], c[P], c[-P],
                                     c[P - 1], c[-P - 1], c[P + 1], c[-P + 1]);
            x[(long)j * P + i] = nw;
        }
        step_sync<WAVES>();
    }
}

// launches kernel(integral_constant<int, WAVES>) -> void (*)(Args), one
// workgroup of elastic_threads(a.dx) per pair, for the WAVES of a's width
template <class Args, class Kernel>
void launch_by_waves(const Args &a, int B, hipStream_t st, Kernel kernel) {
    static_assert(kElasticMaxWaves == 8, "one instantiation per workgroup size below");
    const int w = elastic_waves(a.dx);
    void (*k)(Args);
    switch (w) {
        case 1: k = kernel(std::integral_constant<int, 1>{}); break;
        case 2: k = kernel(std::integral_constant<int, 2>{}); break;
        case 3: k = kernel(std::integral_constant<int, 3>{}); break;
        case 4: k = kernel(std::integral_constant<int, 4>{}); break;
        case 5: k = kernel(std::integral_constant<int, 5>{}); break;
        case 6: k = kernel(std::integral_constant<int, 6>{}); break;
        case 7: k = kernel(std::integral_constant<int, 7>{}); break;
        default: k = kernel(std::integral_constant<int, 8>{}); break;
    }
    hipLaunchKernelGGL(k, dim3(B), dim3(64 * w), 0, st, a);
    OF2D_HIP(hipGetLastError());
}

}  // namespace batch
}  // namespace of2d
