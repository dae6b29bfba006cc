// batch_kernels.hip — B independent Horn-Schunck registrations of one size
// (of2d_batch.h).
//
// The loop kernel: one workgroup per pair runs the niter Jacobi iterations of
// OpticalFlowDiffusion::get_update for its pair, the iterate ping-ponging
// between the pair's two buffers in global memory, with __syncthreads() as the
// only synchronisation: no workgroup waits for another, and with more pairs
// than resident workgroups the grid simply has more blocks.  The per-pixel
// arithmetic is hs::update_px and the quasi-Laplacian rule of hs_jacobi_impl.h
// (q = 0 on the border), compiled with -ffp-contract=off and IEEE division:
// the iterates are bit-identical to the one-pair kernels' and the oracle's.
// Entry, convergence, break and exit are the loop frame's (batch_loop.h).
//
// The passes around the loop are the per-pixel bodies of field_kernels.hip
// (field_px.h, accumulate_px) with the pair as grid dimension z.
#include "of2d_batch.h"

#include "field_px.h"
#include "hs_jacobi_impl.h"

namespace of2d {
namespace batch {

namespace {
constexpr int kBx = 64, kBy = 4;
inline dim3 grid3d(int dx, int dy, int B) {
    return dim3((dx + kBx - 1) / kBx, (dy + kBy - 1) / kBy, B);
}
#define OF2D_BPX_PROLOGUE(DX, DY)                         \
    const int i = blockIdx.x * kBx + threadIdx.x;         \
    const int j = blockIdx.y * kBy + threadIdx.y;         \
    const long pair = blockIdx.z;                         \
    if (i >= (DX) || j >= (DY)) return;
__device__ __forceinline__ bool failed(const unsigned *status, long pair) {
    return status && (status[pair] & kStatusDivZero);
}
}  // namespace

// ------------------------------------------------------------ the loop
template <int WAVES, bool CONV>
__global__ __launch_bounds__(64 * WAVES) void hs_loop_kernel(LoopArgs a) {
    constexpr int T = 64 * WAVES;
    const long pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    PairSlots ps;
    if (!loop_entry<CONV>(a, pair, tid, ps)) return;
    float2 *u0 = a.u0 + pair * a.stride, *u1 = a.u1 + pair * a.stride;
    const float2 *__restrict__ dI = a.dI + pair * a.stride;
    const float *__restrict__ It = a.It + pair * a.stride;
    const int dx = a.dx, dy = a.dy, P = a.P, npx = dx * dy;
    __shared__ int s_stop;
    unsigned bad = 0;
    int n = 0;
    for (int it = 0; it < a.niter; ++it) {
        const float2 *src = (it & 1) ? u1 : u0;
        float2 *dst = (it & 1) ? u0 : u1;
        double v[2] = {0.0, 0.0};
        for_pixels<T>(tid, npx, dx, P, [&](int, int i, int j, long o) {
            // the neighbours of a border pixel lie in the pitch padding or a
            // ghost j-line of the pair's own field; q is zeroed there
            const float2 l = src[o - 1], r = src[o + 1], um = src[o - P], up = src[o + P];
            float2 q;
            // gradients.h:77-79: (((u[i-1] + u[i+1]) + u[j-1]) + u[j+1]) / 4.0f
            q.x = (((l.x + r.x) + um.x) + up.x) / 4.0f;
            q.y = (((l.y + r.y) + um.y) + up.y) / 4.0f;
            q = hs::zero_if(j == 0 || j == dy - 1 || i == 0 || i == dx - 1, q);  // :73-76
            const float2 g = dI[o];
            const float2 nw = hs::update_px(q, g.x, g.y, It[o], a.alphasq, bad);
            if constexpr (CONV) logger_add(nw, src[o], v[0], v[1]);
            dst[o] = nw;
        });
        n = it + 1;
        if constexpr (CONV) {
            block_sums<2, WAVES>(v, wave, lane);
            if (tid == 0) s_stop = loop_decide(v[0], v[1], ps, it);
        }
        if (loop_break<CONV>(s_stop)) break;
    }
    loop_exit(a, pair, tid, lane, ps, n, (int)bad);
}

void launch_hs_loop(const LoopArgs &a, int B, bool conv, hipStream_t st) {
    if (conv)
        hipLaunchKernelGGL((hs_loop_kernel<kLoopWaves, true>), dim3(B), dim3(kLoopThreads), 0, st,
                           a);
    else
        hipLaunchKernelGGL((hs_loop_kernel<kLoopWaves, false>), dim3(B), dim3(kLoopThreads), 0, st,
                           a);
    OF2D_HIP(hipGetLastError());
}

// ------------------------------------------------------------ boundary I/O
__global__ void d2f_kernel(const double *__restrict__ in, int dimx, int dimy,
                           float *__restrict__ out, long so, int P) {
    OF2D_BPX_PROLOGUE(dimx, dimy)
    out[pair * so + (long)j * P + i] = (float)in[pair * dimx * dimy + (long)j * dimx + i];
}
void launch_d2f(const double *in, int npairs, int dimx, int dimy, float *out, long so, int P,
                hipStream_t st) {
    hipLaunchKernelGGL(d2f_kernel, grid3d(dimx, dimy, npairs), dim3(kBx, kBy), 0, st, in, dimx,
                       dimy, out, so, P);
    OF2D_HIP(hipGetLastError());
}

__global__ void f2d_kernel(const float *__restrict__ in, long si, int P, int dimx, int dimy,
                           double *__restrict__ out) {
    OF2D_BPX_PROLOGUE(dimx, dimy)
    out[pair * dimx * dimy + (long)j * dimx + i] = (double)in[pair * si + (long)j * P + i];
}
void launch_f2d(const float *in, long si, int P, int dimx, int dimy, double *out, int npairs,
                hipStream_t st) {
    hipLaunchKernelGGL(f2d_kernel, grid3d(dimx, dimy, npairs), dim3(kBx, kBy), 0, st, in, si, P,
                       dimx, dimy, out);
    OF2D_HIP(hipGetLastError());
}

// Motion::copy_motion_to_input per pair: planar, x-plane first
__global__ void motion_to_planar_kernel(const float2 *__restrict__ m, long sm, int P, int dimx,
                                        int dimy, double *__restrict__ out) {
    OF2D_BPX_PROLOGUE(dimx, dimy)
    const float2 v = m[pair * sm + (long)j * P + i];
    const long n = (long)dimx * dimy, k = pair * 2 * n + (long)j * dimx + i;
    out[k] = (double)v.x;
    out[k + n] = (double)v.y;
}
void launch_motion_to_planar(const float2 *m, long sm, int P, int dimx, int dimy, double *out,
                             int npairs, hipStream_t st) {
    hipLaunchKernelGGL(motion_to_planar_kernel, grid3d(dimx, dimy, npairs), dim3(kBx, kBy), 0, st,
                       m, sm, P, dimx, dimy, out);
    OF2D_HIP(hipGetLastError());
}

// ------------------------------------------------------------ pyramid
__global__ void downsample_image_kernel(const float *__restrict__ in, long si, int dxi, int dyi,
                                        int Pi, float *__restrict__ out, long so, int dxo,
                                        int dyo, int Po) {
    OF2D_BPX_PROLOGUE(dxo, dyo)
    downsample_image_px(in + pair * si, dxi, dyi, Pi, out + pair * so + (long)j * Po + i, dxo,
                        dyo, i, j);
}
void launch_downsample_image(const float *in, long si, int dxi, int dyi, int Pi, float *out,
                             long so, int dxo, int dyo, int Po, int B, hipStream_t st) {
    hipLaunchKernelGGL(downsample_image_kernel, grid3d(dxo, dyo, B), dim3(kBx, kBy), 0, st, in, si,
                       dxi, dyi, Pi, out, so, dxo, dyo, Po);
    OF2D_HIP(hipGetLastError());
}

__global__ void downsample_motion_kernel(const float2 *__restrict__ in, long si, int dxi, int dyi,
                                         int Pi, float2 *__restrict__ out, long so, int dxo,
                                         int dyo, int Po, float rx, float ry,
                                         const unsigned *__restrict__ status) {
    OF2D_BPX_PROLOGUE(dxo, dyo)
    if (failed(status, pair)) return;
    downsample_motion_px(in + pair * si, dxi, dyi, Pi, out + pair * so + (long)j * Po + i, dxo,
                         dyo, i, j, rx, ry);
}
void launch_downsample_motion(const float2 *in, long si, int dxi, int dyi, int Pi, float2 *out,
                              long so, int dxo, int dyo, int Po, int B, const unsigned *status,
                              hipStream_t st) {
    const float rx = (float)dxo / (float)dxi, ry = (float)dyo / (float)dyi;
    hipLaunchKernelGGL(downsample_motion_kernel, grid3d(dxo, dyo, B), dim3(kBx, kBy), 0, st, in,
                       si, dxi, dyi, Pi, out, so, dxo, dyo, Po, rx, ry, status);
    OF2D_HIP(hipGetLastError());
}

__global__ void upsample_motion_kernel(const float2 *__restrict__ in, long si, int dxi, int dyi,
                                       int Pi, float2 *__restrict__ out, long so, int dxo, int dyo,
                                       int Po, float rx, float ry,
                                       const unsigned *__restrict__ status) {
    OF2D_BPX_PROLOGUE(dxo, dyo)
    if (failed(status, pair)) return;
    upsample_motion_px(in + pair * si, dxi, dyi, Pi, out + pair * so + (long)j * Po + i, dxo, dyo,
                       i, j, rx, ry);
}
void launch_upsample_motion(const float2 *in, long si, int dxi, int dyi, int Pi, float2 *out,
                            long so, int dxo, int dyo, int Po, int B, const unsigned *status,
                            hipStream_t st) {
    const float rx = (float)dxo / (float)dxi, ry = (float)dyo / (float)dyi;
    hipLaunchKernelGGL(upsample_motion_kernel, grid3d(dxo, dyo, B), dim3(kBx, kBy), 0, st, in, si,
                       dxi, dyi, Pi, out, so, dxo, dyo, Po, rx, ry, status);
    OF2D_HIP(hipGetLastError());
}

// ------------------------------------------------------------ warp, gradients, composition
__global__ void warp_kernel(const float *__restrict__ src, const float2 *__restrict__ u,
                            float *__restrict__ dst, long stride, int dimx, int dimy, int P,
                            const unsigned *__restrict__ status) {
    OF2D_BPX_PROLOGUE(dimx, dimy)
    if (failed(status, pair)) return;
    const float *s = src + pair * stride;
    const long idx = (long)j * P + i;
    dst[pair * stride + idx] = warp_px(s, u[pair * stride + idx], s[idx], i, j, dimx, dimy, P);
}
void launch_warp(const float *src, const float2 *u, float *dst, long stride, int dimx, int dimy,
                 int P, int B, const unsigned *status, hipStream_t st) {
    hipLaunchKernelGGL(warp_kernel, grid3d(dimx, dimy, B), dim3(kBx, kBy), 0, st, src, u, dst,
                       stride, dimx, dimy, P, status);
    OF2D_HIP(hipGetLastError());
}

__global__ void gradients_kernel(const float *__restrict__ Iref, long sref,
                                 const float *__restrict__ Ia, float2 *__restrict__ dI,
                                 float *__restrict__ It, long stride, int dimx, int dimy, int P,
                                 const unsigned *__restrict__ status) {
    OF2D_BPX_PROLOGUE(dimx, dimy)
    if (failed(status, pair)) return;
    gradients_px(Iref + pair * sref, Ia + pair * stride, dI + pair * stride, It + pair * stride,
                 (long)j * P + i, i, j, dimx, dimy, P);
}
void launch_gradients(const float *Iref, long sref, const float *Iaux, float2 *dI, float *It,
                      long stride, int dimx, int dimy, int P, int B, const unsigned *status,
                      hipStream_t st) {
    hipLaunchKernelGGL(gradients_kernel, grid3d(dimx, dimy, B), dim3(kBx, kBy), 0, st, Iref, sref,
                       Iaux, dI, It, stride, dimx, dimy, P, status);
    OF2D_HIP(hipGetLastError());
}

__global__ void accumulate_kernel(const float2 *__restrict__ mo, const float2 *__restrict__ v0,
                                  const float2 *__restrict__ v1, float2 *__restrict__ mn,
                                  long stride, int dimx, int dimy, int P,
                                  const int *__restrict__ iters, int nloops, int loop,
                                  const unsigned *__restrict__ status) {
    OF2D_BPX_PROLOGUE(dimx, dimy)
    if (failed(status, pair)) return;
    const float2 *v = ((iters[pair * nloops + loop] & 1) ? v1 : v0) + pair * stride;
    const float2 *m = mo + pair * stride;
    const long idx = (long)j * P + i;
    mn[pair * stride + idx] = accumulate_px(m, v[idx], m[idx], i, j, dimx, dimy, P);
}
void launch_accumulate(const float2 *m_old, const float2 *v0, const float2 *v1, float2 *m_new,
                       long stride, int dimx, int dimy, int P, int B, const int *iters,
                       int nloops, int loop, const unsigned *status, hipStream_t st) {
    hipLaunchKernelGGL(accumulate_kernel, grid3d(dimx, dimy, B), dim3(kBx, kBy), 0, st, m_old, v0,
                       v1, m_new, stride, dimx, dimy, P, iters, nloops, loop, status);
    OF2D_HIP(hipGetLastError());
}

__global__ void zero_failed_kernel(float2 *__restrict__ m, long stride,
                                   const unsigned *__restrict__ status) {
    const long pair = blockIdx.x;
    if (!(status[pair] & kStatusDivZero)) return;
    float2 *p = m + pair * stride;
    for (long k = threadIdx.x; k < stride; k += blockDim.x) p[k] = make_float2(0.0f, 0.0f);
}
void launch_zero_failed(float2 *m, long stride, int B, const unsigned *status, hipStream_t st) {
    hipLaunchKernelGGL(zero_failed_kernel, dim3(B), dim3(256), 0, st, m, stride, status);
    OF2D_HIP(hipGetLastError());
}

}  // namespace batch
}  // namespace of2d
