// field_px.h — the per-pixel bodies of the field primitives (field_kernels.hip),
// shared with the batched passes (batch_kernels.hip): one definition of each
// reference loop's arithmetic, so a pair of a batch sees exactly the operations
// the one-pair kernels perform.  (accumulate_px: of2d_device.h.)
#pragma once

#include "of2d_device.h"

namespace of2d {

// Field<float>::downSample (src/Field.tpp:75-143): box average over the
// integer factor dimin/dimout, ii outer / jj inner; *out is left as it is when
// no tap is valid.
__device__ __forceinline__ void downsample_image_px(const float *__restrict__ in, int dxi, int dyi,
                                                    int Pi, float *__restrict__ out, int dxo,
                                                    int dyo, int i, int j) {
    const int fx = dxi / dxo, fy = dyi / dyo;
    float val = 0.0f;
    int p = 0;
    for (int ii = 0; ii < fx; ii++)
        for (int jj = 0; jj < fy; jj++) {
            // (no tap lies past the end: j * fy + jj <= dyo * fy - 1 <= dyi - 1
            // for fy = dyi / dyo, so the reference's k >= sizein skip never fires)
            const int y = j * fy + jj;
            val += in[(long)y * Pi + i * fx + ii];
            p++;
        }
    if (p != 0) *out = val / (float)p;
}

// Motion::downSample (src/Motion.cpp:87-111): Field<vector2d>::downSample then
// every component scaled by dimout/dimin (float ratio).
__device__ __forceinline__ void downsample_motion_px(const float2 *__restrict__ in, int dxi,
                                                     int dyi, int Pi, float2 *__restrict__ out,
                                                     int dxo, int dyo, int i, int j, float rx,
                                                     float ry) {
    const int fx = dxi / dxo, fy = dyi / dyo;
    float vx = 0.0f, vy = 0.0f;
    int p = 0;
    for (int ii = 0; ii < fx; ii++)
        for (int jj = 0; jj < fy; jj++) {
            // (no tap lies past the end: j * fy + jj <= dyo * fy - 1 <= dyi - 1
            // for fy = dyi / dyo, so the reference's k >= sizein skip never fires)
            const int y = j * fy + jj;
            const float2 a = in[(long)y * Pi + i * fx + ii];
            vx = vx + a.x;
            vy = vy + a.y;
            p++;
        }
    float2 o = *out;
    if (p != 0) o = make_float2(vx / (float)p, vy / (float)p);
    o.x *= rx;
    o.y *= ry;
    *out = o;
}

// Motion::upSample (src/Motion.cpp:61-85) = Field<vector2d>::upSample
// (src/Field.tpp:145-206, bilinear renormalised by the valid weight) then
// every component scaled by dimout/dimin.
__device__ __forceinline__ void upsample_motion_px(const float2 *__restrict__ in, int dxi, int dyi,
                                                   int Pi, float2 *__restrict__ out, int dxo,
                                                   int dyo, int i, int j, float rx, float ry) {
    float2 o = *out;
    const float px = (float)i * (float)dxi / (float)dxo;
    const int dx = (int)floorf(px);
    const float fx = px - (float)dx;
    const float py = (float)j * (float)dyi / (float)dyo;
    const int dy = (int)floorf(py);
    const float fy = py - (float)dy;
    const unsigned lin = (unsigned)dx + (unsigned)dy * (unsigned)dxi;
    if (lin < (unsigned)dxi * (unsigned)dyi) {
        const float2 *b = in + (long)dy * Pi + dx;
        float vx = (b[0].x * (1 - fx)) * (1 - fy);
        float vy = (b[0].y * (1 - fx)) * (1 - fy);
        float w = (1 - fx) * (1 - fy);
        const bool ax = (unsigned)dx < (unsigned)(dxi - 1);
        const bool ay = (unsigned)dy < (unsigned)(dyi - 1);
        if (ax) {
            vx = vx + (b[1].x * fx) * (1 - fy);
            vy = vy + (b[1].y * fx) * (1 - fy);
            w += fx * (1 - fy);
        }
        if (ay) {
            vx = vx + (b[Pi].x * (1 - fx)) * fy;
            vy = vy + (b[Pi].y * (1 - fx)) * fy;
            w += (1 - fx) * fy;
        }
        if (ax && ay) {
            vx = vx + (b[Pi + 1].x * fx) * fy;
            vy = vy + (b[Pi + 1].y * fx) * fy;
            w += fx * fy;
        }
        if (w != 0) o = make_float2(vx / w, vy / w);
    }
    o.x *= rx;
    o.y *= ry;
    *out = o;
}

// Image::warp2d (src/Image.cpp:119-182): pull-back bilinear sample of src at
// (i + u.x, j + u.y); out-of-range floor keeps the original pixel; at the
// right/top edge only in-range taps are used, renormalised by their weight.
//
// Branch-free: the taps are loaded unconditionally (an out-of-range tap
// pattern reads element 0; g[1], g[P], g[P+1] of an in-image pixel stay in the
// allocation: pitch padding and the zeroed ghost j-line below the last row)
// and the reference's conditional terms are selects.
__device__ __forceinline__ float warp_px(const float *__restrict__ src, float2 m, float own, int i,
                                         int j, int dimx, int dimy, int P) {
    const float px = (float)i + m.x;
    const int dx = floor_int(px);
    const float fx = px - (float)dx;
    const float py = (float)j + m.y;
    const int dy = floor_int(py);
    const float fy = py - (float)dy;
    const bool ok = !(dx < 0 || dx >= dimx || dy < 0 || dy >= dimy);
    const bool ax = dx < dimx - 1, ay = dy < dimy - 1;
    const float *b = src + (ok ? ((unsigned)dy * (unsigned)P + (unsigned)dx) : 0u);
    const float t00 = b[0], t10 = b[1], t01 = b[P], t11 = b[P + 1];
    float val = (t00 * (1 - fx)) * (1 - fy);
    float w = (1 - fx) * (1 - fy);
    const float v10 = val + (t10 * fx) * (1 - fy), w10 = w + fx * (1 - fy);
    val = ax ? v10 : val;
    w = ax ? w10 : w;
    const float v01 = val + (t01 * (1 - fx)) * fy, w01 = w + (1 - fx) * fy;
    val = ay ? v01 : val;
    w = ay ? w01 : w;
    const float v11 = val + (t11 * fx) * fy, w11 = w + fx * fy;
    val = (ax && ay) ? v11 : val;
    w = (ax && ay) ? w11 : w;
    // val / w is val itself when w rounds to exactly 1 (demons_kernels.hip
    // warp_batch): divide only in the waves where some lane needs it
    float q = val;
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(ok && w != 1.0f) != 0, 0)) q = val / w;
    return (ok && w != 0) ? q : own;
}

// IterativeSolver::set_derivatives (IterativeSolver.cpp:22-56):
//   dI = (partial_x, partial_y)(Iaux)  gradients.h:9-32 (central /2.0f,
//   one-sided on the borders); It = Iaux - Iref.  idx = j * P + i; jg: the
//   global j-line of row j (the border rule uses the global index).
__device__ __forceinline__ void gradients_px(const float *__restrict__ Iref,
                                             const float *__restrict__ Ia,
                                             float2 *__restrict__ dI, float *__restrict__ It,
                                             long idx, int i, int jg, int dimx, int dimy, int P) {
    float gx, gy;
    if (i == 0)
        // f[idx + 1] in the reference's unpitched array: with one column that
        // is the pixel of the next j-line (one past the array on the last
        // j-line, read as 0 here), not the pitch padding
        gx = (dimx > 1 ? Ia[idx + 1] : (jg < dimy - 1 ? Ia[idx + P] : 0.0f)) - Ia[idx];
    else if (i == dimx - 1)
        gx = Ia[idx] - Ia[idx - 1];
    else
        gx = (Ia[idx + 1] - Ia[idx - 1]) / 2.0f;
    if (jg == 0)
        gy = Ia[idx + P] - Ia[idx];
    else if (jg == dimy - 1)
        gy = Ia[idx] - Ia[idx - P];
    else
        gy = (Ia[idx + P] - Ia[idx - P]) / 2.0f;
    dI[idx] = make_float2(gx, gy);
    It[idx] = Ia[idx] - Iref[idx];
}

// Image::jacobian (src/Image.cpp:189-218): the determinant of id + u at pixel
// (i, j), (1 + dudx.x)(1 + dudy.y) - dudx.y * dudy.x, with partial_x /
// partial_y of the motion (gradients.h:9-32: central /2.0f, one-sided on the
// borders).  dimx, dimy >= 2.  jacobian_kernel (analysis_kernels.hip) evaluates
// the same expression from its LDS tile.
__device__ __forceinline__ float jacobian_px(const float2 *__restrict__ u, int i, int j, int dimx,
                                             int dimy, int P) {
    const long idx = (long)j * P + i;
    const float2 m = u[idx];
    float2 dx, dy;
    if (i == 0) {
        const float2 a = u[idx + 1];
        dx = make_float2(a.x - m.x, a.y - m.y);
    } else if (i == dimx - 1) {
        const float2 b = u[idx - 1];
        dx = make_float2(m.x - b.x, m.y - b.y);
    } else {
        const float2 a = u[idx + 1], b = u[idx - 1];
        dx = make_float2((a.x - b.x) / 2.0f, (a.y - b.y) / 2.0f);
    }
    if (j == 0) {
        const float2 a = u[idx + P];
        dy = make_float2(a.x - m.x, a.y - m.y);
    } else if (j == dimy - 1) {
        const float2 b = u[idx - P];
        dy = make_float2(m.x - b.x, m.y - b.y);
    } else {
        const float2 a = u[idx + P], b = u[idx - P];
        dy = make_float2((a.x - b.x) / 2.0f, (a.y - b.y) / 2.0f);
    }
    return (1.0f + dx.x) * (1.0f + dy.y) - dx.y * dy.x;
}

}  // namespace of2d
