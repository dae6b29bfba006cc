// batch_demons_lds_kernels.hip — the batched Thirion's Demons loop with the
// field its two convolutions read kept in LDS (option "conv_lds", of2d_batch.h,
// DESIGN.md §4.6.6).
//
// One workgroup of kLoopThreads per pair, as demons_loop_kernel
// (batch_demons_kernels.hip), and the same pixel-to-thread mapping: thread t
// owns pixels t, t + T, ... in ascending linear index, PPT of them at most (the
// template parameter, so the register arrays below are statically indexed).
// The stages, their expressions and their operand order are that kernel's
// (batch_demons_px.h, field_px.h, accumulate_px); what differs is where the
// correction and the motion before the last smoothing live: not in the pair's
// global corr and mid slices but in ONE dense float2 plane in LDS, pixel
// (i, j) at element j * dx + i, followed by dx + 1 zeroed elements (the
// unconditional b[1], b[P], b[P + 1] loads of accumulate_px reach them from the
// last pixels and discard them by select).  A value that replaces the plane's
// is computed into the owner's registers, and stored after a barrier, when
// every thread has read its taps; a second barrier publishes it:
//   1  W = warp_px(Iaux, u) to the pair's global W slice             barrier
//   2  the correction from W and Iref into the plane                 barrier
//   3  c~ = plane (*) G(sigma_fluid), 4  m = the update of u by c~ (gathers
//      the global iterate), into registers          barrier, store, barrier
//   5  u' = plane (*) G(sigma_diffusion) to the other global buffer of the
//      iterate, the Logger terms against u; block_sums, decision, barrier
// EXP (diffeomorphic): c~ and the thread's maxabs term into registers (3),
// block_max and the count (3a), the scaling in registers and the store (3b),
// each squaring accumulate_px(plane, c, c, ...) into registers, then barrier,
// store, barrier (3c; the last one's store is step 4's), then m (4).
// __syncthreads() is the only synchronisation; no workgroup waits for another.
// Entry, convergence, break and exit are the loop frame's (batch_loop.h) and
// the divide-by-zero exit after stage 2 is demons_loop_kernel's, so iterates,
// errors and counts equal that kernel's bit for bit.
#include <utility>

#include "batch_demons_px.h"
#include "field_px.h"

namespace of2d {
namespace batch {

namespace {

// The thread's number for pixel k of an unrolled stage, made opaque and
// dependent on a value of pixel k - 1.  A pixel's coordinates, its taps'
// addresses and its border tests are the same in every iteration of the loop;
// without this the compiler forms them for all PPT pixels once before the loop
// and keeps them, or runs the PPT pixels of a stage side by side, which the 128
// registers of a 1024-thread workgroup's lane do not hold beside the PPT new
// values (it spilled to scratch).  With it they are formed afresh, one pixel
// after the other; a pixel's kw * kw taps are still in flight together
__device__ __forceinline__ int pixel_tid(int tid, float after) {
    asm volatile("" : "+v"(tid) : "v"(after));
    return tid;
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>) in order:
// the stages that hold a convolution are too long for the unroller, and a loop
// it leaves rolled indexes the register array dynamically (scratch)
template <class F, int... K>
__device__ __forceinline__ void each_pixel(F &&f, std::integer_sequence<int, K...>) {
    (f(std::integral_constant<int, K>{}), ...);
}

template <int PPT, bool CONV, int KW, bool EXP>
__global__ __launch_bounds__(kLoopThreads) void demons_lds_kernel(DemonsLoopArgs a) {
    constexpr int T = kLoopThreads;
    // the plane: dx * dy pixels and dx + 1 zeros
    extern __shared__ __attribute__((aligned(16))) float2 s_f[];
    __shared__ int s_stop, s_bad;
    const long pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    PairSlots ps;
    if (!loop_entry<CONV>(a, pair, tid, ps)) return;
    float2 *u0 = a.u0 + pair * a.stride, *u1 = a.u1 + pair * a.stride;
    const float *__restrict__ Iref = a.Iref + pair * a.sref;
    const float *__restrict__ Iaux = a.Iaux + pair * a.stride;
    float *W = a.W + pair * a.stride;
    const int dx = a.dx, dy = a.dy, P = a.P, npx = dx * dy, kw = a.kw;
    if (tid == 0) s_stop = s_bad = 0;  // published by the barrier after stage 1
    for (int c = tid; c <= dx; c += T) s_f[npx + c] = make_float2(0.0f, 0.0f);
    int n = 0;
    bool bad = false;
    for (int it = 0; it < a.niter; ++it) {
        const float2 *src = (it & 1) ? u1 : u0;
        float2 *dst = (it & 1) ? u0 : u1;
        // 1. the moving image by the iterate
        for (int idx = tid; idx < npx; idx += T) {
            const int j = idx / dx, i = idx - j * dx;
            const long o = (long)j * P + i;
            W[o] = warp_px(Iaux, src[o], Iaux[o], i, j, dx, dy, P);
        }
        __syncthreads();
        // 2. the correction into the plane (its last readers, stage 5 of the
        // iteration before, are behind that iteration's last barrier)
        for (int idx = tid; idx < npx; idx += T) {
            const int j = idx / dx, i = idx - j * dx;
            const long o = (long)j * P + i;
            s_f[idx] =
                demons_corr_px(W, Iref[o], o, i, j, dx, dy, P, a.sigma_isq, a.sigma_xsq, bad);
        }
        if (bad) s_bad = 1;
        __syncthreads();
        if (s_bad) break;  // block-uniform: the reference throws here
        float2 m[PPT];     // the thread's pixels' next values of the plane
        if constexpr (EXP) {
            __shared__ int s_nsq;
            // 3. the smoothed correction, and Motion::maxabs
            float mx = 0.0f;
            each_pixel(
                [&](auto K) __attribute__((always_inline)) {
                    constexpr int k = decltype(K)::value;
                    const int idx = pixel_tid(tid, k ? m[k ? k - 1 : 0].x : 0.0f) + k * T;
                    m[k] = make_float2(0.0f, 0.0f);
                    if (idx < npx) {
                        const int j = idx / dx, i = idx - j * dx;
                        float2 c;
                        if (!conv_direct<KW>(s_f, a.fluid, kw, i, j, dx, dy, dx, c)) c = s_f[idx];
                        m[k] = c;
                        mx = maxabs_fold(mx, c);
                    }
                },
                std::make_integer_sequence<int, PPT>{});
            // 3a. the block's maximum (a thread without a pixel brings 0) and
            // the squaring count; behind the barrier inside every thread has
            // read its taps of the correction
            mx = block_max<kLoopWaves>(mx, wave, lane);
            if (tid == 0) s_nsq = exp_squarings(mx);
            __syncthreads();
            const int nsq = s_nsq;  // block-uniform
            if (nsq > 0) {          // Motion::exp returns early otherwise
                // 3b. Field<vector2d>::operator*=((float)std::pow(2, -nsq)),
                // exact, and the scaled field into the plane
                const float sc = ldexpf(1.0f, -nsq);
#pragma unroll
                for (int k = 0; k < PPT; k++) {
                    const int idx = tid + k * T;
                    if (idx < npx) {
                        m[k].x *= sc;
                        m[k].y *= sc;
                        s_f[idx] = m[k];
                    }
                }
                __syncthreads();
                // 3c. u <- u o u: a squaring gathers from the plane, dense
                // (pitch dx), the own pixel from the registers that hold it
                for (int q = 0; q < nsq; ++q) {
#pragma unroll
                    for (int k = 0; k < PPT; k++) {
                        const int idx = pixel_tid(tid, k ? m[k - 1].x : 0.0f) + k * T;
                        if (idx < npx) {
                            const int j = idx / dx, i = idx - j * dx;
                            m[k] = accumulate_px(s_f, m[k], m[k], i, j, dx, dy, dx);
                        }
                    }
                    __syncthreads();
                    if (q + 1 == nsq) break;  // step 4 reads the own pixel only
#pragma unroll
                    for (int k = 0; k < PPT; k++) {
                        const int idx = tid + k * T;
                        if (idx < npx) s_f[idx] = m[k];
                    }
                    __syncthreads();
                }
            }
            // 4. motion->accumulate(*correspondence): the gather is from src;
            // no thread reads the plane any more
#pragma unroll
            for (int k = 0; k < PPT; k++) {
                const int idx = pixel_tid(tid, k ? m[k - 1].x : 0.0f) + k * T;
                if (idx < npx) {
                    const int j = idx / dx, i = idx - j * dx;
                    const long o = (long)j * P + i;
                    m[k] = accumulate_px(src, m[k], src[o], i, j, dx, dy, P);
                    s_f[idx] = m[k];
                }
            }
        } else {
            // 3 + 4. the smoothed correction and the motion update
            each_pixel(
                [&](auto K) __attribute__((always_inline)) {
                    constexpr int k = decltype(K)::value;
                    const int idx = pixel_tid(tid, k ? m[k ? k - 1 : 0].x : 0.0f) + k * T;
                    m[k] = make_float2(0.0f, 0.0f);
                    if (idx < npx) {
                        const int j = idx / dx, i = idx - j * dx;
                        const long o = (long)j * P + i;
                        float2 c;
                        if (!conv_direct<KW>(s_f, a.fluid, kw, i, j, dx, dy, dx, c)) c = s_f[idx];
                        const float2 own = src[o];
                        float2 v = own;  // another enum value: no update
                        if (a.mode == 0)
                            v = accumulate_px(src, c, own, i, j, dx, dy, P);
                        else if (a.mode == 1)
                            v = make_float2(own.x + c.x, own.y + c.y);  // Field::operator+=
                        m[k] = v;
                    }
                },
                std::make_integer_sequence<int, PPT>{});
            __syncthreads();  // every thread has read its taps of the correction
#pragma unroll
            for (int k = 0; k < PPT; k++) {
                const int idx = tid + k * T;
                if (idx < npx) s_f[idx] = m[k];
            }
        }
        __syncthreads();
        // 5. the smoothed motion into the other buffer, and the Logger's terms
        double v[2] = {0.0, 0.0};
        for (int idx = tid; idx < npx; idx += T) {
            const int j = idx / dx, i = idx - j * dx;
            const long o = (long)j * P + i;
            float2 nw;
            if (!conv_direct<KW>(s_f, a.diff, kw, i, j, dx, dy, dx, nw)) nw = s_f[idx];
            if constexpr (CONV) logger_add(nw, src[o], v[0], v[1]);
            dst[o] = nw;
        }
        n = it + 1;
        if constexpr (CONV) {
            block_sums<2, kLoopWaves>(v, wave, lane);
            if (tid == 0) s_stop = loop_decide(v[0], v[1], ps, it);
        }
        if (loop_break<CONV>(s_stop)) break;
    }
    loop_exit(a, pair, tid, lane, ps, n, bad);
}

template <int PPT, bool CONV, int KW, bool EXP>
void launch_one(const DemonsLoopArgs &a, int B, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL((demons_lds_kernel<PPT, CONV, KW, EXP>), dim3(B), dim3(kLoopThreads), lds,
                       st, a);
}
template <int PPT, bool CONV, int KW>
void launch_exp(const DemonsLoopArgs &a, int B, size_t lds, hipStream_t st) {
    if (a.diffeomorphic)
        launch_one<PPT, CONV, KW, true>(a, B, lds, st);
    else
        launch_one<PPT, CONV, KW, false>(a, B, lds, st);
}
// the usual widths are compiled in; every other one takes the runtime loops
template <int PPT, bool CONV>
void launch_width(const DemonsLoopArgs &a, int B, size_t lds, hipStream_t st) {
    switch (a.kw) {
        case 3: launch_exp<PPT, CONV, 3>(a, B, lds, st); break;
        case 5: launch_exp<PPT, CONV, 5>(a, B, lds, st); break;
        case 7: launch_exp<PPT, CONV, 7>(a, B, lds, st); break;
        default: launch_exp<PPT, CONV, 0>(a, B, lds, st); break;
    }
}
template <int PPT>
void launch_ppt(const DemonsLoopArgs &a, int B, bool conv, size_t lds, hipStream_t st) {
    if (conv)
        launch_width<PPT, true>(a, B, lds, st);
    else
        launch_width<PPT, false>(a, B, lds, st);
}

// only the PPT 16 instantiations can ask for more than the default limit
template <bool CONV, int KW>
bool admit(bool ok) {
    const size_t most = kResidentLdsBudget - kResidentLdsReserve;
    for (const void *k : {(const void *)demons_lds_kernel<kConvLdsMaxPpt, CONV, KW, false>,
                          (const void *)demons_lds_kernel<kConvLdsMaxPpt, CONV, KW, true>})
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most) !=
            hipSuccess)
            ok = false;
    return ok;
}

}  // namespace

bool conv_lds_prepare() {
    bool ok = true;
    ok = admit<false, 3>(ok);
    ok = admit<true, 3>(ok);
    ok = admit<false, 5>(ok);
    ok = admit<true, 5>(ok);
    ok = admit<false, 7>(ok);
    ok = admit<true, 7>(ok);
    ok = admit<false, 0>(ok);
    ok = admit<true, 0>(ok);
    if (!ok) (void)hipGetLastError();  // the caller falls back to placement 0
    return ok;
}

void launch_demons_lds(const DemonsLoopArgs &a, int B, bool conv, hipStream_t st) {
    if (!conv_lds_fits(a.dx, a.dy))
        throw std::invalid_argument("launch_demons_lds: the level does not fit");
    const size_t lds = conv_lds_bytes(a.dx, a.dy);
    switch (conv_lds_ppt(a.dx, a.dy)) {
        case 1: launch_ppt<1>(a, B, conv, lds, st); break;
        case 4: launch_ppt<4>(a, B, conv, lds, st); break;
        default: launch_ppt<kConvLdsMaxPpt>(a, B, conv, lds, st); break;
    }
    OF2D_HIP(hipGetLastError());
}

}  // namespace batch
}  // namespace of2d
