// fluid_px.h — the per-pixel expressions of one iteration of
// OpticalFlowFluid::get_update (OpticalFlowFluid.cpp:123-140) around the
// velocity sweep, for every kernel that holds the pixel's values itself: the
// batch's Fluid loop (batch_fluid_kernels.hip) and the plain one-pair kernels
// (fluid_kernels.hip: increment_kernel, timestep_kernel).  The force and the
// sweep's pixel are sor_px.h's, which Elastic shares; the Jacobian of the
// integrated estimate is jacobian_px (field_px.h).  -ffp-contract=off.
//
// The copies that remain, in fluid_kernels.hip, the same operations in the
// same association: sor_increment_worker (the gradients, the increment and
// maxabs' term from the rows it loads before its wait) and fluid_step_kernel
// (the integration and the new estimate's gradients from its LDS tile), both
// hand-scheduled and run by benchmark configuration 4.
#pragma once

#include <hip/hip_runtime.h>

namespace of2d {

struct FluidGrad {
    float2 dx, dy;
};
// partial_x / partial_y of the estimate (gradients.h:9-32): one-sided on the
// borders, (a - b) / 2.0f inside; dimx, dimy >= 2.  idx = j * P + i
__device__ __forceinline__ FluidGrad fluid_gradients_px(const float2 *u, long idx, int i, int j,
                                                        int dimx, int dimy, int P) {
    FluidGrad d;
    if (i == 0) {
        const float2 a = u[idx + 1], b = u[idx];
        d.dx = make_float2(a.x - b.x, a.y - b.y);
    } else if (i == dimx - 1) {
        const float2 a = u[idx], b = u[idx - 1];
        d.dx = make_float2(a.x - b.x, a.y - b.y);
    } else {
        const float2 a = u[idx + 1], b = u[idx - 1];
        d.dx = make_float2((a.x - b.x) / 2.0f, (a.y - b.y) / 2.0f);
    }
    if (j == 0) {
        const float2 a = u[idx + P], b = u[idx];
        d.dy = make_float2(a.x - b.x, a.y - b.y);
    } else if (j == dimy - 1) {
        const float2 a = u[idx], b = u[idx - P];
        d.dy = make_float2(a.x - b.x, a.y - b.y);
    } else {
        const float2 a = u[idx + P], b = u[idx - P];
        d.dy = make_float2((a.x - b.x) / 2.0f, (a.y - b.y) / 2.0f);
    }
    return d;
}
// the gradients of the zero estimate that follows a regrid: +0, as from a
// zeroed buffer
__device__ __forceinline__ FluidGrad fluid_gradients_zero() {
    return FluidGrad{make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f)};
}

// R = (v - dudx v.x) - dudy v.y (OpticalFlowFluid.cpp:84)
__device__ __forceinline__ float2 fluid_increment_px(float2 v, const FluidGrad &d) {
    return make_float2((v.x - d.dx.x * v.x) - d.dy.x * v.y, (v.y - d.dx.y * v.x) - d.dy.y * v.y);
}
// Motion::maxabs (Motion.cpp:51-58) squares .y twice: m <- max(m, (float)(y y
// + y y)) in double, a NaN term dropped
__device__ __forceinline__ float fluid_maxabs_px(float m, float2 r) {
    const double y = (double)r.y;
    const float q = (float)(y * y + y * y);
    return (m < q) ? q : m;
}
// maxabs = sqrt(max), dt = dumax / maxabs with dumax = 0.65f
// (OpticalFlowFluid.h:32, .cpp:92-95); maxabs 0 gives dt = inf
__device__ __forceinline__ float2 fluid_timestep(float m) {
    const float maxabs = sqrtf(m);
    const float dumax = 0.65f;
    return make_float2(maxabs, dumax / maxabs);
}
// u' = u + R dt where dt < 65, else u (OpticalFlowFluid.cpp:115, :135-137)
__device__ __forceinline__ float2 fluid_integrate_px(float2 u, float2 r, float dt) {
    return dt < 65.0f ? make_float2(u.x + r.x * dt, u.y + r.y * dt) : u;
}

}  // namespace of2d
