// analysis_kernels.hip — deformation analysis of a motion field on gfx950:
// the Jacobian determinant map with fused statistics, the inverse field by a
// fixed-point iteration whose stop is decided on the device, and the
// similarity of two images (DESIGN.md "Deformation analysis").
//
// The Jacobian and the composition restate the reference pixel for pixel in
// the same fp32 operation order (-ffp-contract=off), so the map and every
// iterate of the inverse are bit-identical to the oracle's.  All three are
// HBM-bound passes; every reduction goes through per-block partials combined
// in a fixed order (integer atomics only), so results do not depend on the
// order in which blocks run.
#include "of2d_device.h"

#include <algorithm>
#include <cstring>

namespace of2d {

// (wave_sum, wave_min, wave_max and the order of every sum below: the shared
// helpers of of2d_device.h, "Logger sums")

// ------------------------------------------------------------ Jacobian
// A block of 256 threads takes a kJacW x kJacH pixel tile: the tile of u plus
// a one-pixel ring goes through LDS (pixels outside the image read as 0 and
// are never used: the borders take one-sided differences), then each thread
// evaluates four consecutive pixels of two rows and stores each run as one
// float4 (rows of the pitched map are 16-B aligned).
namespace {
constexpr int kJacW = 128, kJacH = 16;
// LDS column of tile column c (ring included): one float2 of padding per 32,
// so that the 32 lanes of a ds_read_b64 group, four pixels apart, fall on
// distinct bank pairs
__device__ __forceinline__ int jac_col(int c) { return c + (c >> 5); }
constexpr int kJacLdsW = kJacW + 2 + (kJacW + 2) / 32 + 1;
}  // namespace

__global__ __launch_bounds__(256) void jacobian_kernel(const float2 *__restrict__ u, int dimx,
                                                       int dimy, int P, float *__restrict__ jac,
                                                       JacPartial *__restrict__ part) {
    __shared__ float2 t[kJacH + 2][kJacLdsW];
    const int i0 = blockIdx.x * kJacW, j0 = blockIdx.y * kJacH;
    for (int s = threadIdx.x; s < (kJacH + 2) * (kJacW + 2); s += 256) {
        const int r = s / (kJacW + 2), c = s - r * (kJacW + 2);
        const int i = i0 + c - 1, j = j0 + r - 1;
        float2 v = make_float2(0.0f, 0.0f);
        if (i >= 0 && i < dimx && j >= 0 && j < dimy) v = u[(long)j * P + i];
        t[r][jac_col(c)] = v;
    }
    __syncthreads();
    const int cx = (threadIdx.x & 31) * 4, ry = threadIdx.x >> 5;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    double sum = 0.0;
    unsigned le0 = 0, lt05 = 0;
#pragma unroll
    for (int h = 0; h < kJacH / 8; h++) {
        const int rr = ry + 8 * h, j = j0 + rr;
        if (j >= dimy || i0 + cx >= dimx) continue;
        const int r = rr + 1;
        float q[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int i = i0 + cx + e, c = cx + e + 1;
            q[e] = 0.0f;
            if (i >= dimx) continue;
            const float2 m = t[r][jac_col(c)];
            // partial_x / partial_y of the motion (gradients.h:9-32)
            float2 dx, dy;
            if (i == 0) {
                const float2 a = t[r][jac_col(c + 1)];
                dx = make_float2(a.x - m.x, a.y - m.y);
            } else if (i == dimx - 1) {
                const float2 b = t[r][jac_col(c - 1)];
                dx = make_float2(m.x - b.x, m.y - b.y);
            } else {
                const float2 a = t[r][jac_col(c + 1)], b = t[r][jac_col(c - 1)];
                dx = make_float2((a.x - b.x) / 2.0f, (a.y - b.y) / 2.0f);
            }
            if (j == 0) {
                const float2 a = t[r + 1][jac_col(c)];
                dy = make_float2(a.x - m.x, a.y - m.y);
            } else if (j == dimy - 1) {
                const float2 b = t[r - 1][jac_col(c)];
                dy = make_float2(m.x - b.x, m.y - b.y);
            } else {
                const float2 a = t[r + 1][jac_col(c)], b = t[r - 1][jac_col(c)];
                dy = make_float2((a.x - b.x) / 2.0f, (a.y - b.y) / 2.0f);
            }
            const float v = (1.0f + dx.x) * (1.0f + dy.y) - dx.y * dy.x;  // Image.cpp:189-218
            q[e] = v;
            mn = (v < mn) ? v : mn;
            mx = (v > mx) ? v : mx;
            sum += (double)v;
            le0 += (v <= 0.0f) ? 1u : 0u;
            lt05 += (v < 0.5f) ? 1u : 0u;
        }
        if (jac)
            *reinterpret_cast<float4 *>(jac + (long)j * P + i0 + cx) =
                make_float4(q[0], q[1], q[2], q[3]);
    }
    // the block's partial: wave trees, then the four waves in order
    mn = wave_min(mn);
    mx = wave_max(mx);
    sum = wave_sum(sum);
    le0 = wave_sum(le0);
    lt05 = wave_sum(lt05);
    __shared__ JacPartial red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = JacPartial{mn, mx, sum, le0, lt05};
    __syncthreads();
    if (threadIdx.x == 0) {
        JacPartial p = red[0];
        for (int w = 1; w < 4; w++) {
            p.mn = (red[w].mn < p.mn) ? red[w].mn : p.mn;
            p.mx = (red[w].mx > p.mx) ? red[w].mx : p.mx;
            p.sum += red[w].sum;
            p.le0 += red[w].le0;
            p.lt05 += red[w].lt05;
        }
        part[(long)blockIdx.y * gridDim.x + blockIdx.x] = p;
    }
}

// one 1024-thread block: strided per-thread partials, wave trees, the 16 waves
// in order
__global__ __launch_bounds__(1024) void jacobian_reduce_kernel(const JacPartial *__restrict__ part,
                                                               int nb, double npx,
                                                               double *__restrict__ stats) {
    float mn = __builtin_inff(), mx = -__builtin_inff();
    double sum = 0.0, le0 = 0.0, lt05 = 0.0;  // counts are exact in fp64 (< 2^53)
    for (int b = threadIdx.x; b < nb; b += 1024) {
        const JacPartial p = part[b];
        mn = (p.mn < mn) ? p.mn : mn;
        mx = (p.mx > mx) ? p.mx : mx;
        sum += p.sum;
        le0 += (double)p.le0;
        lt05 += (double)p.lt05;
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    sum = wave_sum(sum);
    le0 = wave_sum(le0);
    lt05 = wave_sum(lt05);
    __shared__ float rf[2][16];
    __shared__ double rd[3][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        rf[0][wave] = mn;
        rf[1][wave] = mx;
        rd[0][wave] = sum;
        rd[1][wave] = le0;
        rd[2][wave] = lt05;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; w++) {
            mn = (rf[0][w] < mn) ? rf[0][w] : mn;
            mx = (rf[1][w] > mx) ? rf[1][w] : mx;
            sum += rd[0][w];
            le0 += rd[1][w];
            lt05 += rd[2][w];
        }
        stats[0] = (double)mn;
        stats[1] = (double)mx;
        stats[2] = sum / npx;
        stats[3] = le0;
        stats[4] = lt05;
    }
}

int jacobian_nblocks(int dimx, int dimy) {
    return ((dimx + kJacW - 1) / kJacW) * ((dimy + kJacH - 1) / kJacH);
}

void launch_jacobian(const float2 *u, int dimx, int dimy, int P, float *jac, JacPartial *part,
                     double *stats, hipStream_t st) {
    if (dimx < 2 || dimy < 2)
        throw std::invalid_argument("jacobian: the field needs dimx >= 2 and dimy >= 2");
    const dim3 g((dimx + kJacW - 1) / kJacW, (dimy + kJacH - 1) / kJacH);
    hipLaunchKernelGGL(jacobian_kernel, g, dim3(256), 0, st, u, dimx, dimy, P, jac, part);
    OF2D_HIP(hipGetLastError());
    hipLaunchKernelGGL(jacobian_reduce_kernel, dim3(1), dim3(1024), 0, st, part,
                       jacobian_nblocks(dimx, dimy), (double)dimx * (double)dimy, stats);
    OF2D_HIP(hipGetLastError());
}

// ------------------------------------------------------------ similarity
// 64 x 4 threads take kSimW x 4 pixel tiles, four consecutive pixels per lane
// as one float4 of each image, in a grid-stride loop over a capped grid.
namespace {
constexpr int kSimW = 256, kSimH = 4;
inline int sim_tiles(int dimx, int dimy) {
    return ((dimx + kSimW - 1) / kSimW) * ((dimy + kSimH - 1) / kSimH);
}
}  // namespace

__global__ __launch_bounds__(256) void similarity_kernel(const float *__restrict__ a,
                                                         const float *__restrict__ b, int dimx,
                                                         int dimy, int P,
                                                         SimPartial *__restrict__ part) {
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    float mn[2] = {__builtin_inff(), __builtin_inff()};
    float mx[2] = {-__builtin_inff(), -__builtin_inff()};
    const int nbx = (dimx + kSimW - 1) / kSimW, nt = nbx * ((dimy + kSimH - 1) / kSimH);
    for (int t = blockIdx.x; t < nt; t += gridDim.x) {
        const int i = (t % nbx) * kSimW + threadIdx.x * 4, j = (t / nbx) * kSimH + threadIdx.y;
        if (i >= dimx || j >= dimy) continue;
        const long idx = (long)j * P + i;  // i + 3 < P: both are multiples of 4
        const float4 va = *reinterpret_cast<const float4 *>(a + idx);
        const float4 vb = *reinterpret_cast<const float4 *>(b + idx);
        const float xa[4] = {va.x, va.y, va.z, va.w}, xb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (i + e >= dimx) continue;
            const double x = (double)xa[e], y = (double)xb[e], d = x - y;
            s[0] += x;
            s[1] += y;
            s[2] += x * x;
            s[3] += y * y;
            s[4] += x * y;
            s[5] += d * d;
            mn[0] = (xa[e] < mn[0]) ? xa[e] : mn[0];
            mx[0] = (xa[e] > mx[0]) ? xa[e] : mx[0];
            mn[1] = (xb[e] < mn[1]) ? xb[e] : mn[1];
            mx[1] = (xb[e] > mx[1]) ? xb[e] : mx[1];
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) s[k] = wave_sum(s[k]);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        mn[k] = wave_min(mn[k]);
        mx[k] = wave_max(mx[k]);
    }
    __shared__ SimPartial red[4];
    const int tid = threadIdx.y * 64 + threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (lane == 0) {
        for (int k = 0; k < 6; k++) red[wave].s[k] = s[k];
        for (int k = 0; k < 2; k++) {
            red[wave].mn[k] = mn[k];
            red[wave].mx[k] = mx[k];
        }
    }
    __syncthreads();
    if (tid == 0) {
        SimPartial p = red[0];
        for (int w = 1; w < 4; w++) {
            for (int k = 0; k < 6; k++) p.s[k] += red[w].s[k];
            for (int k = 0; k < 2; k++) {
                p.mn[k] = (red[w].mn[k] < p.mn[k]) ? red[w].mn[k] : p.mn[k];
                p.mx[k] = (red[w].mx[k] > p.mx[k]) ? red[w].mx[k] : p.mx[k];
            }
        }
        part[blockIdx.x] = p;
    }
}

__global__ __launch_bounds__(256) void similarity_reduce_kernel(
    const SimPartial *__restrict__ part, int nb, double npx, double *__restrict__ out) {
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    float mn[2] = {__builtin_inff(), __builtin_inff()};
    float mx[2] = {-__builtin_inff(), -__builtin_inff()};
    for (int b = threadIdx.x; b < nb; b += 256) {
        const SimPartial p = part[b];
        for (int k = 0; k < 6; k++) s[k] += p.s[k];
        for (int k = 0; k < 2; k++) {
            mn[k] = (p.mn[k] < mn[k]) ? p.mn[k] : mn[k];
            mx[k] = (p.mx[k] > mx[k]) ? p.mx[k] : mx[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) s[k] = wave_sum(s[k]);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        mn[k] = wave_min(mn[k]);
        mx[k] = wave_max(mx[k]);
    }
    __shared__ SimPartial red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        for (int k = 0; k < 6; k++) red[wave].s[k] = s[k];
        for (int k = 0; k < 2; k++) {
            red[wave].mn[k] = mn[k];
            red[wave].mx[k] = mx[k];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        SimPartial p = red[0];
        for (int w = 1; w < 4; w++) {
            for (int k = 0; k < 6; k++) p.s[k] += red[w].s[k];
            for (int k = 0; k < 2; k++) {
                p.mn[k] = (red[w].mn[k] < p.mn[k]) ? red[w].mn[k] : p.mn[k];
                p.mx[k] = (red[w].mx[k] > p.mx[k]) ? red[w].mx[k] : p.mx[k];
            }
        }
        out[0] = p.s[5] / npx;
        // the sums' covariance form; a constant image (its extrema coincide)
        // has no correlation
        const double va = p.s[2] - p.s[0] * p.s[0] / npx, vb = p.s[3] - p.s[1] * p.s[1] / npx;
        const double cab = p.s[4] - p.s[0] * p.s[1] / npx;
        const bool flat = p.mn[0] == p.mx[0] || p.mn[1] == p.mx[1] || !(va > 0.0) || !(vb > 0.0);
        out[1] = flat ? __builtin_nan("") : cab / sqrt(va * vb);
    }
}

int similarity_nblocks(int dimx, int dimy) { return std::min(sim_tiles(dimx, dimy), kCappedGrid); }

void launch_similarity(const float *a, const float *b, int dimx, int dimy, int P,
                       SimPartial *part, double *out, hipStream_t st) {
    if (dimx < 1 || dimy < 1) throw std::invalid_argument("similarity: empty image");
    const int nb = similarity_nblocks(dimx, dimy);
    hipLaunchKernelGGL(similarity_kernel, dim3(nb), dim3(64, 4), 0, st, a, b, dimx, dimy, P, part);
    OF2D_HIP(hipGetLastError());
    hipLaunchKernelGGL(similarity_reduce_kernel, dim3(1), dim3(256), 0, st, part, nb,
                       (double)dimx * (double)dimy, out);
    OF2D_HIP(hipGetLastError());
}

// ------------------------------------------------------------ inverse field
// One update of the fixed-point iteration, 64 x 4 threads on a 64 x 16 pixel
// tile (four rows per thread).  |r| is compared as the bits of the
// non-negative float: an integer maximum, exact and independent of order (and
// a NaN, above every number, keeps the loop from reporting convergence).
namespace {
constexpr int kInvRows = 4;  // rows per thread
}

__global__ __launch_bounds__(256) void invert_step_kernel(const float2 *__restrict__ u,
                                                          const float2 *__restrict__ vin,
                                                          float2 *__restrict__ vout, int dimx,
                                                          int dimy, int P, int k, float tol,
                                                          unsigned *__restrict__ ctl,
                                                          int max_iter) {
    if (k > 0) {
        // stopped by an earlier launch, or by this one: every block takes the
        // same decision from words the previous launches wrote
        if (ctl[0] <= (unsigned)k) return;
        if (__uint_as_float(ctl[k]) < tol) {  // m of update k - 1
            if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0)
                ctl[0] = (unsigned)k;
            return;
        }
    }
    const int i = blockIdx.x * 64 + threadIdx.x;
    unsigned mb = 0u, oob = 0u;
#pragma unroll
    for (int q = 0; q < kInvRows; q++) {
        const int j = blockIdx.y * (4 * kInvRows) + 4 * q + threadIdx.y;
        if (i >= dimx || j >= dimy) continue;
        const long idx = (long)j * P + i;
        const float2 v = vin[idx];
        const int dx = floor_int((float)i + v.x), dy = floor_int((float)j + v.y);
        const bool ok = !(dx < 0 || dx >= dimx || dy < 0 || dy >= dimy);
        const float2 r = accumulate_px(u, v, make_float2(0.0f, 0.0f), i, j, dimx, dimy, P);
        vout[idx] = make_float2(v.x - r.x, v.y - r.y);
        const unsigned bx = __float_as_uint(fabsf(r.x)), by = __float_as_uint(fabsf(r.y));
        mb = bx > mb ? bx : mb;
        mb = by > mb ? by : mb;
        oob += ok ? 0u : 1u;
    }
    mb = wave_max(mb);
    oob = wave_sum(oob);
    __shared__ unsigned red[2][4];
    const int tid = threadIdx.y * 64 + threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (lane == 0) {
        red[0][wave] = mb;
        red[1][wave] = oob;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; w++) {
            mb = red[0][w] > mb ? red[0][w] : mb;
            oob += red[1][w];
        }
        // (the plain read may be stale, that is lower: one atomic too many)
        if (mb > ctl[1 + k]) atomicMax(&ctl[1 + k], mb);
        if (oob) atomicAdd(&ctl[1 + max_iter + k], oob);
    }
}

void launch_invert_step(const float2 *u, const float2 *vin, float2 *vout, int dimx, int dimy,
                        int P, int k, float tol, unsigned *ctl, int max_iter, hipStream_t st) {
    if (dimx < 2 || dimy < 2 || k < 0 || k >= max_iter)
        throw std::invalid_argument("invert: dimx, dimy >= 2 and 0 <= k < max_iter");
    const dim3 g((dimx + 63) / 64, (dimy + 4 * kInvRows - 1) / (4 * kInvRows));
    hipLaunchKernelGGL(invert_step_kernel, g, dim3(64, 4), 0, st, u, vin, vout, dimx, dimy, P, k,
                       tol, ctl, max_iter);
    OF2D_HIP(hipGetLastError());
}

InvertResult invert_field(const float2 *u, float2 *v0, float2 *v1, int dimx, int dimy, int P,
                          int max_iter, float tol, unsigned *ctl, float *residuals,
                          hipStream_t st) {
    if (max_iter < 1) throw std::invalid_argument("invert: max_iter < 1");
    OF2D_HIP(hipMemsetAsync(ctl, 0, invert_ctl_words(max_iter) * sizeof(unsigned), st));
    OF2D_HIP(hipMemsetAsync(ctl, 0x7f, sizeof(unsigned), st));  // kInvertRunning
    std::vector<unsigned> h(1 + (size_t)max_iter, 0u);
    auto as_float = [](unsigned b) {
        float f;
        memcpy(&f, &b, sizeof f);
        return f;
    };
    float2 *buf[2] = {v0, v1};
    int k = 0;
    for (;;) {
        const int kend = std::min(k + kInvertChunk, max_iter);
        for (; k < kend; k++)
            launch_invert_step(u, buf[k & 1], buf[(k + 1) & 1], dimx, dimy, P, k, tol, ctl,
                               max_iter, st);
        // the chunk's report: the stop word and every m so far
        OF2D_HIP(hipMemcpyAsync(h.data(), ctl, (1 + (size_t)k) * sizeof(unsigned),
                                hipMemcpyDeviceToHost, st));
        OF2D_HIP(hipStreamSynchronize(st));
        if (h[0] != kInvertRunning || as_float(h[k]) < tol || k == max_iter) break;
    }
    InvertResult res;
    res.iterations = h[0] != kInvertRunning ? (int)h[0] : k;
    res.residual = as_float(h[res.iterations]);
    res.converged = res.residual < tol;
    OF2D_HIP(hipMemcpyAsync(&res.oob, ctl + max_iter + res.iterations, sizeof(unsigned),
                            hipMemcpyDeviceToHost, st));
    OF2D_HIP(hipStreamSynchronize(st));
    res.v = buf[res.iterations & 1];
    if (residuals)
        for (int t = 0; t < max_iter; t++)
            residuals[t] = t < res.iterations ? as_float(h[1 + (size_t)t]) : 0.0f;
    return res;
}

}  // namespace of2d
