// batch_curvature_kernels.hip — B independent Curvature registrations of one
// size (of2d_batch.h): the whole loop of
// OpticalFlowCurvature::get_update (OpticalFlowCurvature.cpp:144-167) for one
// pair in one workgroup, where the one-pair path takes eight launches per
// iteration (rhs, transpose / lines / transpose / lines forward, the same
// backward, construct; solvers.cpp, loop_curvature).
//
// Every level's sides are fast-transform lengths (batch_plan.h, curv_level_ok).
// An iteration, with a barrier between stages:
//   1. rhs = u - tau f as double planes x | y   (curv_rhs_kernel's floats)
//   2. REDFT10 along y          3. REDFT10 along x, times the eigenvalues E
//   4. REDFT01 along y          5. REDFT01 along x
//   6. u' = (float)Z / (4.0f n) into the other iterate buffer, with the
//      Logger terms                             (curv_construct_kernel's floats)
// The plane pair lives in the pair's dense fp64 scratch slice in global memory
// (16 B per pixel) and each pass moves its lines through LDS in chunks of
// whole lines (curv_chunk_lines).  The per-line arithmetic is dct_px.h's, the
// one-pair dct_lines_kernel's: fp64 with -ffp-contract=off, a line's result
// depends on that line only, so the iterates are the one-pair fast path's bit
// for bit.  Along y there is no transposed copy: a chunk is a bundle of
// adjacent columns, lane after lane on adjacent columns (a row segment of
// 8 B per lane in global memory), and the LDS lines are padded by one point
// (kCurvLinePad) so that those lanes fall on different banks.
//
// No workgroup waits for another.  Every barrier is reached by all threads:
// the chunk loops' trip counts depend on the level only, and the break goes
// through LDS (loop_break).  Entry, convergence, break and exit are the loop
// frame's (batch_loop.h); Curvature has no zero denominator (4.0f * n > 0).
#include "of2d_batch.h"

#include "dct_px.h"

namespace of2d {
namespace batch {

namespace {
// REDFT10 (KIND 0; along x times E) or REDFT01 (KIND 1) of every line of the
// plane pair X | X + plane along AXIS (0: x, the dy rows; 1: y, the dx
// columns), in place, lpc lines per chunk through z.  Ends with a barrier
template <int KIND, int AXIS>
__device__ __forceinline__ void curv_pass(double *X, long plane, int dx, int dy, int logN, int lpc,
                                          const double2 *__restrict__ tw,
                                          const double *__restrict__ E, double2 *z, int tid) {
    constexpr int T = kCurvThreads, PAD = kCurvLinePad;
    const int N = AXIS ? dy : dx, nlines = AXIS ? dx : dy, half = N >> 1;
    for (int line0 = 0; line0 < nlines; line0 += lpc) {
        const int nl = min(lpc, nlines - line0), pts = nl * N;
        // two elements per plane per lane.  Along x a lane's pair is one 16-B
        // segment of its row; along y lanes run across the columns first
#pragma unroll 1
        for (int g = tid; g < (pts >> 1); g += T) {
            int l, m;
            double2 a, b;
            if (AXIS == 0) {
                l = g >> (logN - 1);
                m = g & (half - 1);
                const double *pa = X + (long)(line0 + l) * dx + 2 * m;
                a = *reinterpret_cast<const double2 *>(pa);
                b = *reinterpret_cast<const double2 *>(pa + plane);
            } else {
                m = g / nl;
                l = g - m * nl;
                const double *pa = X + (long)(2 * m) * dx + (line0 + l);
                a = make_double2(pa[0], pa[dx]);
                b = make_double2(pa[plane], pa[plane + dx]);
            }
            dct_put<KIND, PAD>(z, l, m, N, a, b);
        }
        __syncthreads();
        if (KIND == 1) dct_inv_pre<PAD, kCurvPointsPerThread>(z, pts, N, logN, tw, tid, T);
        dct_fft<PAD>(z, pts, N, logN, tw, tid, T);
#pragma unroll 1
        for (int g = tid; g < (pts >> 1); g += T) {
            int l, m;
            if (AXIS == 0) {
                l = g >> (logN - 1);
                m = g & (half - 1);
            } else {
                m = g / nl;
                l = g - m * nl;
            }
            double ya[2], yb[2];
            dct_get<KIND, PAD>(z, l, m, N, tw, ya, yb);
            if (AXIS == 0) {
                const long off = (long)(line0 + l) * dx + 2 * m;
                if (KIND == 0) dct_scale(ya, yb, *reinterpret_cast<const double2 *>(E + off));
                *reinterpret_cast<double2 *>(X + off) = make_double2(ya[0], ya[1]);
                *reinterpret_cast<double2 *>(X + off + plane) = make_double2(yb[0], yb[1]);
            } else {
                double *pa = X + (long)(2 * m) * dx + (line0 + l);
                pa[0] = ya[0];
                pa[dx] = ya[1];
                pa[plane] = yb[0];
                pa[plane + dx] = yb[1];
            }
        }
        __syncthreads();  // the chunk is in the scratch and z is free again
    }
}
}  // namespace

template <bool CONV>
__global__ __launch_bounds__(kCurvThreads) void curv_loop_kernel(CurvLoopArgs a) {
    constexpr int T = kCurvThreads, WAVES = kCurvWaves;
    extern __shared__ double2 z[];
    const long pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    PairSlots ps;
    if (!loop_entry<CONV>(a, pair, tid, ps)) return;
    float2 *u0 = a.u0 + pair * a.stride, *u1 = a.u1 + pair * a.stride;
    const float2 *__restrict__ dI = a.dI + pair * a.stride;
    const float *__restrict__ It = a.It + pair * a.stride;
    const int dx = a.dx, dy = a.dy, P = a.P, npx = dx * dy;
    double *X = a.X + pair * a.sx;
    const long plane = npx;
    const float tau = a.tau, div = a.div;
    __shared__ int s_stop;
    int n = 0;
    for (int it = 0; it < a.niter; ++it) {
        const float2 *src = (it & 1) ? u1 : u0;
        float2 *dst = (it & 1) ? u0 : u1;
        // rhs = u - tau * f with f = dI * ((It + u.x dI.x) + u.y dI.y)
        // (OpticalFlow.cpp:15-39, OpticalFlowCurvature.cpp:75-97): float
        // arithmetic, stored as double
        for_pixels<T>(tid, npx, dx, P, [&](int idx, int, int, long o) {
            const float2 m = src[o], g = dI[o];
            const float sc = (It[o] + m.x * g.x) + m.y * g.y;
            const float fx = g.x * sc, fy = g.y * sc;
            X[idx] = (double)(m.x - tau * fx);
            X[plane + idx] = (double)(m.y - tau * fy);
        });
        __syncthreads();
        // the oracle's axis order: y first; forward with E, then inverse
        curv_pass<0, 1>(X, plane, dx, dy, a.logy, a.ly, a.twy, nullptr, z, tid);
        curv_pass<0, 0>(X, plane, dx, dy, a.logx, a.lx, a.twx, a.E, z, tid);
        curv_pass<1, 1>(X, plane, dx, dy, a.logy, a.ly, a.twy, nullptr, z, tid);
        curv_pass<1, 0>(X, plane, dx, dy, a.logx, a.lx, a.twx, nullptr, z, tid);
        // u' = vector2d(Z.x, Z.y) / (4.0f * n) (OpticalFlowCurvature.cpp:106-125:
        // the double -> float conversion, then coord2d::operator/ in float)
        double v[2] = {0.0, 0.0};
        for_pixels<T>(tid, npx, dx, P, [&](int idx, int, int, long o) {
            const float2 nw = make_float2((float)X[idx] / div, (float)X[plane + idx] / div);
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
    loop_exit(a, pair, tid, lane, ps, n, 0);
}

void launch_curv_loop(const CurvLoopArgs &a, int B, bool conv, hipStream_t st) {
    static_assert(sizeof(double2) == kCurvPointBytes, "batch_plan.h counts LDS in double2 points");
    if (!curv_level_ok(a.dx, a.dy))
        throw std::invalid_argument("curv_loop: a side is not a power of two in [8, 512]");
    const size_t lds = curv_lds_bytes(a.dx, a.dy);
    if (conv)
        hipLaunchKernelGGL((curv_loop_kernel<true>), dim3(B), dim3(kCurvThreads), lds, st, a);
    else
        hipLaunchKernelGGL((curv_loop_kernel<false>), dim3(B), dim3(kCurvThreads), lds, st, a);
    OF2D_HIP(hipGetLastError());
}

}  // namespace batch
}  // namespace of2d
