// batch_demons_px.h — the per-pixel bodies of the batched Demons loop, shared by
// its two kernels (batch_demons_kernels.hip: every field in global memory;
// batch_demons_lds_kernels.hip: the convolved field in LDS): one definition of
// each expression, so both give the same bits.
#pragma once

#include "of2d_batch.h"

namespace of2d {
namespace batch {

// Field<vector2d>::convolute (Field.tpp:209-269) at pixel (i, j) of the
// pitched field f: the direct kw x kw sum over the taps whose LINEAR index
// lin + ii + jj * dimx lies in [0, N) (a tap past an x edge is the
// neighbouring j-line's pixel), ii outer / jj inner, fp32 products and sums
// with (float) weights; divided by (float) of the fp64 sum of the valid
// weights (wfull where every tap is valid: the same additions in the same
// order).  false: the weight sum is 0 and the reference leaves the pixel.
// KW > 0: the width at compile time (the taps unrolled, the weights in scalar
// registers); KW == 0: the runtime width kw_rt.  The same operations in the
// same order either way.  Every tap read is a pixel (row in [0, dy), column in
// [0, dx)), so a dense field (P == dx, no ghost lines) serves as well.
template <int KW>
__device__ __forceinline__ bool conv_direct(const float2 *__restrict__ f, const DemonsTable &k,
                                            int kw_rt, int i, int j, int dx, int dy, int P,
                                            float2 &out) {
    const int kw = KW > 0 ? KW : kw_rt;
    const int c = (kw - 1) / 2;
    const long N = (long)dx * dy, lin = (long)j * dx + i;
    const bool interior = (lin - c - (long)c * dx >= 0) && (lin + c + (long)c * dx < N);
    float vx = 0.0f, vy = 0.0f;
    double weight = 0.0;
#pragma unroll
    for (int ii = -c; ii <= c; ii++) {
        // column i + ii of j-line j + jj is pixel (col, j + jj + r)
        int col = i + ii, r = 0;
        while (col < 0) {  // once unless c > dx
            col += dx;
            r -= 1;
        }
        while (col >= dx) {
            col -= dx;
            r += 1;
        }
        const float *kf = k.kf + (ii + c);
        if (interior) {
            const float2 *p = f + (long)(j + r - c) * P + col;
#pragma unroll
            for (int q = 0; q <= 2 * c; q++) {  // q = jj + c
                const float2 t = p[(long)q * P];
                const float w = kf[q * kw];
                vx = vx + t.x * w;
                vy = vy + t.y * w;
            }
        } else {
            const double *kd = k.kd + (ii + c);
#pragma unroll
            for (int q = 0; q <= 2 * c; q++) {
                const int row = j + r + q - c;
                // 0 <= col < dx: row * dx + col is in [0, N) iff the row is
                if ((unsigned)row >= (unsigned)dy) continue;  // Field.tpp:245-247
                const float2 t = f[(long)row * P + col];
                const float w = kf[q * kw];
                vx = vx + t.x * w;
                vy = vy + t.y * w;
                weight += kd[q * kw];
            }
        }
    }
    if (interior) weight = k.wfull;
    if (weight == 0) return false;
    const float wf = (float)weight;  // coord2d::operator/(const T&) with T = float
    out = make_float2(vx / wf, vy / wf);
    return true;
}

// The correction at pixel (i, j), o = j * P + i, of the warped image W:
// gradients.h:9-32 (central / 2.0f, one-sided on the borders; with one column
// f[idx + 1] is the next j-line's pixel, as gradients_px has it), It = W - Iref
// (Demons.cpp:57), then IterativeSolver.cpp:22-56 / Demons.cpp:34-63:
//   dI * It / (dI.x^2 + dI.y^2 + It*It*sigma_isq/sigma_xsq) * -1
// bad: set where the denominator is exactly 0 (coord2d.h:95-100)
__device__ __forceinline__ float2 demons_corr_px(const float *W, float iref, long o, int i, int j,
                                                 int dx, int dy, int P, float sigma_isq,
                                                 float sigma_xsq, bool &bad) {
    const float w0 = W[o];
    float gx, gy;
    if (i == 0)
        gx = (dx > 1 ? W[o + 1] : (j < dy - 1 ? W[o + P] : 0.0f)) - w0;
    else if (i == dx - 1)
        gx = w0 - W[o - 1];
    else
        gx = (W[o + 1] - W[o - 1]) / 2.0f;
    if (j == 0)
        gy = W[o + P] - w0;
    else if (j == dy - 1)
        gy = w0 - W[o - P];
    else
        gy = (W[o + P] - W[o - P]) / 2.0f;
    const float It = w0 - iref;
    const float t = (It * It) * sigma_isq;
    const float den = (gx * gx + gy * gy) + t / sigma_xsq;
    bad |= den == 0.0f;
    return make_float2(((gx * It) / den) * -1.0f, ((gy * It) / den) * -1.0f);
}

// Motion::maxabs's term of one vector (Motion.cpp:51-58: .y squared twice, in
// double) as maxabs_partial_kernel has it; the comparison drops a NaN term as
// std::max does
__device__ __forceinline__ float maxabs_fold(float mx, float2 c) {
    const double y = (double)c.y;
    const float s = (float)(y * y + y * y);
    return (mx < s) ? s : mx;
}

// Motion::exp's squaring count from the field's maxabs (exp_prepare_kernel's
// expressions, Motion.cpp:253-261): a NaN or out-of-int ceil converts to
// INT_MIN as on x86-64
__device__ __forceinline__ int exp_squarings(float mx) {
    const float ma = sqrtf(mx);
    const float c = ceilf(1.0f + log2f(ma));
    const int nsq =
        (c == c && c > -2147483648.0f && c < 2147483648.0f) ? (int)c : (int)0x80000000;
    return nsq < 0 ? 0 : nsq;
}

}  // namespace batch
}  // namespace of2d
