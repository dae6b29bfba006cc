// sor_px.h — one pixel of the SOR sweep of OpticalFlowElastic::SOR_iteration
// (OpticalFlowElastic.cpp:37-50; OpticalFlowFluid.cpp:27-35 is the same
// expression on the velocity) and of its right-hand side, the force, for every
// kernel that holds the pixel's values itself: the batch's sweep
// (batch_sweep.h) and the plain one-pair kernels (fluid_kernels.hip).
// Compiled with -ffp-contract=off:
//   x' = (1 - w) x + w / (-6 mu - 2 lambda) * (b - mu (R + L + U + D)
//        - (mu + lambda) (R + L + 0.25 (RU - LU - RD + LD).yx))
// R, L: the neighbours at i + 1, i - 1; U, D: at j + 1, j - 1; the reference
// relaxes i-outer, j-inner in place, so L, LU, LD and D are NEW values and R,
// RU, RD and U are OLD ones.
//
// The copies that remain (in fluid_kernels.hip but for the last), the same
// operations in the same association: sor_px in sor_strip_kernel's step (packed fp32 in its
// register window) and force_px in fluid_step_kernel (between its LDS tiles),
// both hand-scheduled and run by benchmark configuration 4; force_px in
// sor_pack_kernel and in elastic_loop_kernel (batch_elastic_kernels.hip), whose
// measured instruction streams the call would change.
#pragma once

#include <hip/hip_runtime.h>

namespace of2d {

// the per-pixel constants evaluated once on the host with the reference's
// float operations (OpticalFlowFluid.cpp:27)
struct SorCoef {
    float A;   // 1 - omega
    float B;   // omega / (-6 mu - 2 lambda)
    float M;   // mu
    float ML;  // mu + lambda
};
inline SorCoef sor_coef(float mu, float lambda, float omega) {
    SorCoef k;
    k.A = 1.0f - omega;
    k.B = omega / (-6 * mu - 2 * lambda);
    k.M = mu;
    k.ML = mu + lambda;
    return k;
}

// OpticalFlow::get_force (OpticalFlow.cpp:15-39), Elastic's and Fluid's alike
// (once fluid_force_px): f = dI ((It + u.x dI.x) + u.y dI.y); u is +0 after a regrid
__device__ __forceinline__ float2 force_px(float2 u, float2 g, float it) {
    const float sc = (it + u.x * g.x) + u.y * g.y;
    return make_float2(g.x * sc, g.y * sc);
}

__device__ __forceinline__ float2 sor_px(const SorCoef &k, float2 C, float2 b, float2 L, float2 R,
                                         float2 U, float2 D, float2 LU, float2 LD, float2 RU,
                                         float2 RD) {
    const float rlx = R.x + L.x, rly = R.y + L.y;
    const float s1x = (rlx + U.x) + D.x, s1y = (rly + U.y) + D.y;
    const float tx = ((RU.x - LU.x) - RD.x) + LD.x, ty = ((RU.y - LU.y) - RD.y) + LD.y;
    // the x component takes the mixed term of y and the reverse
    const float s2x = rlx + 0.25f * ty, s2y = rly + 0.25f * tx;
    return make_float2(k.A * C.x + k.B * ((b.x - k.M * s1x) - k.ML * s2x),
                       k.A * C.y + k.B * ((b.y - k.M * s1y) - k.ML * s2y));
}

}  // namespace of2d
