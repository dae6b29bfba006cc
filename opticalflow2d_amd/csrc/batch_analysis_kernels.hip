// batch_analysis_kernels.hip — deformation analysis of every pair of a batch
// in one launch each (of2d_batch.h): the Jacobian
// determinant map with its statistics, the inverse field with its whole
// fixed-point loop, and the similarity of two image stacks.
//
// The shape is the loop kernels' (batch_kernels.hip): one workgroup of
// kLoopThreads per pair, blockIdx.x the pair, thread t on pixels t, t + T, ...
// in ascending linear index, __syncthreads() the only synchronisation; no
// workgroup waits for another and there are no float atomics.  A thread
// without a pixel (fewer pixels than threads is a normal case) brings the
// neutral element to every reduction.  Every fp64 sum is the thread's pixels
// in ascending order, then the block_sums tree; minima, maxima and the integer
// counts do not depend on order.  The per-pixel arithmetic is the one-pair
// kernels' (jacobian_px, accumulate_px, analysis_kernels.hip's similarity
// terms), compiled with -ffp-contract=off and IEEE division: the maps and
// every iterate of the inverse are bit-identical to the one-pair path's.
#include "of2d_batch.h"

#include "field_px.h"

namespace of2d {
namespace batch {

namespace {
constexpr int kT = kLoopThreads;
// K minima and K maxima over the workgroup, valid in its first thread; one
// barrier, one call per kernel (the LDS array is the instantiation's)
template <int K>
__device__ __forceinline__ void block_extrema(float (&mn)[K], float (&mx)[K], int wave, int lane) {
#pragma unroll
    for (int k = 0; k < K; k++) {
        mn[k] = wave_min(mn[k]);
        mx[k] = wave_max(mx[k]);
    }
    __shared__ float red[2][K][kLoopWaves];
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            red[0][k][wave] = mn[k];
            red[1][k][wave] = mx[k];
        }
    }
    __syncthreads();
    if (wave == 0 && lane == 0) {
        for (int w = 1; w < kLoopWaves; w++)
#pragma unroll
            for (int k = 0; k < K; k++) {
                mn[k] = (red[0][k][w] < mn[k]) ? red[0][k][w] : mn[k];
                mx[k] = (red[1][k][w] > mx[k]) ? red[1][k][w] : mx[k];
            }
    }
}
}  // namespace

// ------------------------------------------------------------ Jacobian
__global__ __launch_bounds__(kT) void batch_jacobian_kernel(JacobianArgs a) {
    const long pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float2 *__restrict__ u = a.u + pair * a.stride;
    float *__restrict__ jac = a.jac ? a.jac + pair * a.stride : nullptr;
    const int dx = a.dx, dy = a.dy, P = a.P, npx = dx * dy;
    float mn[1] = {__builtin_inff()}, mx[1] = {-__builtin_inff()};
    double s[3] = {0.0, 0.0, 0.0};  // sum J, count(J <= 0), count(J < 0.5f): exact in fp64
    for (int idx = tid; idx < npx; idx += kT) {
        const int j = idx / dx, i = idx - j * dx;
        const float v = jacobian_px(u, i, j, dx, dy, P);
        if (jac) jac[(long)j * P + i] = v;
        mn[0] = (v < mn[0]) ? v : mn[0];
        mx[0] = (v > mx[0]) ? v : mx[0];
        s[0] += (double)v;
        s[1] += (v <= 0.0f) ? 1.0 : 0.0;
        s[2] += (v < 0.5f) ? 1.0 : 0.0;
    }
    block_sums<3, kLoopWaves>(s, wave, lane);
    block_extrema<1>(mn, mx, wave, lane);
    if (tid == 0) {
        double *st = a.stats + 5 * pair;
        st[0] = (double)mn[0];
        st[1] = (double)mx[0];
        st[2] = s[0] / (double)npx;
        st[3] = s[1];
        st[4] = s[2];
    }
}

void launch_batch_jacobian(const JacobianArgs &a, int B, hipStream_t st) {
    if (a.dx < 2 || a.dy < 2)
        throw std::invalid_argument("jacobian: the field needs dimx >= 2 and dimy >= 2");
    hipLaunchKernelGGL(batch_jacobian_kernel, dim3(B), dim3(kT), 0, st, a);
    OF2D_HIP(hipGetLastError());
}

// ------------------------------------------------------------ inverse field
// invert_field's loop (analysis_kernels.hip) for one pair: v_0 = 0, update k
// is v <- v - r_k with r_k = accumulate(u, v), 0 where floor(x + v) is outside
// the grid (floor_int: a NaN coordinate is outside), m_k the largest bit
// pattern of |r_k|'s components (a NaN sorts above every number).  The update
// is always applied; the workgroup leaves after the first k with m_k < tol or
// after max_iter updates, whatever the other pairs do.  A thread reads its own
// pixel of v only (u alone is gathered), so v is updated in place; the barriers
// are for the reduction and for the decision, which the first thread takes and
// publishes through LDS.
__global__ __launch_bounds__(kT) void batch_invert_kernel(InvertArgs a) {
    const long pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float2 *__restrict__ u = a.u + pair * a.stride;
    float2 *__restrict__ v = a.v + pair * a.stride;
    float *res = a.residuals ? a.residuals + pair * a.max_iter : nullptr;
    const int dx = a.dx, dy = a.dy, P = a.P, npx = dx * dy;
    __shared__ unsigned red[2][kLoopWaves];
    __shared__ int s_stop;
    unsigned m_last = 0u, oob_last = 0u;  // the first thread's: the last update's
    int n = 0;
    for (int k = 0; k < a.max_iter; ++k) {
        unsigned mb = 0u, oob = 0u;
        for (int idx = tid; idx < npx; idx += kT) {
            const int j = idx / dx, i = idx - j * dx;
            const long o = (long)j * P + i;
            const float2 c = k ? v[o] : make_float2(0.0f, 0.0f);  // v_0 = 0
            const int fx = floor_int((float)i + c.x), fy = floor_int((float)j + c.y);
            const bool ok = !(fx < 0 || fx >= dx || fy < 0 || fy >= dy);
            const float2 r = accumulate_px(u, c, make_float2(0.0f, 0.0f), i, j, dx, dy, P);
            v[o] = make_float2(c.x - r.x, c.y - r.y);
            const unsigned bx = __float_as_uint(fabsf(r.x)), by = __float_as_uint(fabsf(r.y));
            mb = bx > mb ? bx : mb;
            mb = by > mb ? by : mb;
            oob += ok ? 0u : 1u;
        }
        mb = wave_max(mb);
        oob = wave_sum(oob);
        if (lane == 0) {
            red[0][wave] = mb;
            red[1][wave] = oob;
        }
        __syncthreads();
        n = k + 1;
        if (tid == 0) {
            for (int w = 1; w < kLoopWaves; w++) {
                mb = red[0][w] > mb ? red[0][w] : mb;
                oob += red[1][w];
            }
            m_last = mb;
            oob_last = oob;
            if (res) res[k] = __uint_as_float(mb);
            s_stop = (__uint_as_float(mb) < a.tol) ? 1 : 0;
        }
        // the update's barrier: the decision is published, red[] is free again
        __syncthreads();
        if (s_stop) break;
    }
    if (res)
        for (int k = n + tid; k < a.max_iter; k += kT) res[k] = 0.0f;
    if (tid == 0) {
        double *info = a.info + 4 * pair;
        const float m = __uint_as_float(m_last);
        info[0] = (double)n;
        info[1] = (double)m;
        info[2] = (double)oob_last;
        info[3] = (m < a.tol) ? 1.0 : 0.0;
    }
}

void launch_batch_invert(const InvertArgs &a, int B, hipStream_t st) {
    if (a.dx < 2 || a.dy < 2)
        throw std::invalid_argument("invert: the field needs dimx >= 2 and dimy >= 2");
    if (a.max_iter < 1) throw std::invalid_argument("invert: max_iter < 1");
    hipLaunchKernelGGL(batch_invert_kernel, dim3(B), dim3(kT), 0, st, a);
    OF2D_HIP(hipGetLastError());
}

// ------------------------------------------------------------ similarity
// similarity_kernel's sums and extrema per pair, then similarity_reduce_kernel's
// {mse, ncc} (the covariance form; NaN when an image's extrema coincide or a
// variance is not > 0).
__global__ __launch_bounds__(kT) void batch_similarity_kernel(SimilarityArgs a) {
    const long pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *__restrict__ xa = a.a + pair * a.sa;
    const float *__restrict__ xb = a.b + pair * a.sb;
    const int dx = a.dx, dy = a.dy, P = a.P, npx = dx * dy;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    float mn[2] = {__builtin_inff(), __builtin_inff()};
    float mx[2] = {-__builtin_inff(), -__builtin_inff()};
    for (int idx = tid; idx < npx; idx += kT) {
        const int j = idx / dx, i = idx - j * dx;
        const long o = (long)j * P + i;
        const float fa = xa[o], fb = xb[o];
        const double x = (double)fa, y = (double)fb, d = x - y;
        s[0] += x;
        s[1] += y;
        s[2] += x * x;
        s[3] += y * y;
        s[4] += x * y;
        s[5] += d * d;
        mn[0] = (fa < mn[0]) ? fa : mn[0];
        mx[0] = (fa > mx[0]) ? fa : mx[0];
        mn[1] = (fb < mn[1]) ? fb : mn[1];
        mx[1] = (fb > mx[1]) ? fb : mx[1];
    }
    block_sums<6, kLoopWaves>(s, wave, lane);
    block_extrema<2>(mn, mx, wave, lane);
    if (tid == 0) {
        const double n = (double)npx;
        double *out = a.out + pair * a.so;
        out[0] = s[5] / n;
        const double va = s[2] - s[0] * s[0] / n, vb = s[3] - s[1] * s[1] / n;
        const double cab = s[4] - s[0] * s[1] / n;
        const bool flat = mn[0] == mx[0] || mn[1] == mx[1] || !(va > 0.0) || !(vb > 0.0);
        out[1] = flat ? __builtin_nan("") : cab / sqrt(va * vb);
    }
}

void launch_batch_similarity(const SimilarityArgs &a, int B, hipStream_t st) {
    if (a.dx < 1 || a.dy < 1) throw std::invalid_argument("similarity: empty image");
    hipLaunchKernelGGL(batch_similarity_kernel, dim3(B), dim3(kT), 0, st, a);
    OF2D_HIP(hipGetLastError());
}

}  // namespace batch
}  // namespace of2d
