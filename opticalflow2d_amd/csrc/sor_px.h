// sor_px.h — one pixel of the SOR sweep of OpticalFlowElastic::SOR_iteration
// (OpticalFlowElastic.cpp:37-50; OpticalFlowFluid.cpp:27-35 is the same
// expression on the velocity), for the kernels that hold the pixel's nine
// values themselves: the batch's Elastic loop (batch_elastic_kernels.hip) and
// its Fluid loop's velocity sweep (batch_fluid_kernels.hip).  The one-pair sweep
// (fluid_kernels.hip, sor_strip_kernel) keeps its own copy of these lines in
// its register window; the two must stay the same operations in the same
// association, compiled with -ffp-contract=off:
//   x' = (1 - w) x + w / (-6 mu - 2 lambda) * (b - mu (R + L + U + D)
//        - (mu + lambda) (R + L + 0.25 (RU - LU - RD + LD).yx))
// R, L: the neighbours at i + 1, i - 1; U, D: at j + 1, j - 1; the reference
// relaxes i-outer, j-inner in place, so L, LU, LD and D are NEW values and R,
// RU, RD and U are OLD ones.
#pragma once

#include <hip/hip_runtime.h>

namespace of2d {

// the per-pixel constants evaluated once on the host with the reference's
// float operations, as launch_sor_traced evaluates them
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
