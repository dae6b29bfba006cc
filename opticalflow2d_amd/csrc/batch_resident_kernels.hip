// batch_resident_kernels.hip — the batched Horn-Schunck loop with the pair's
// iterate, dI and It kept on the CU (option "resident", of2d_batch.h,
// DESIGN.md §4.6.5).
//
// One workgroup of kLoopThreads per pair, as hs_loop_kernel (batch_kernels.hip),
// and the same pixel-to-thread mapping: thread t owns pixels t, t + T, ... in
// ascending linear index, PPT of them at most (the template parameter, so the
// register arrays below are statically indexed).  What differs is where the
// data lives across the iterations of the loop:
//   - the iterate: one float2 copy in LDS, (dx + 2) x (dy + 2) with a zeroed
//     ghost ring, so the four neighbour taps stay unconditional and
//     hs::zero_if discards q on the border as in the global-memory kernel;
//   - dI, It: loaded once before the first iteration into the registers of the
//     thread that owns the pixel;
//   - the new values of an iteration: in the owner's registers until every
//     thread has read its neighbours (a barrier), then stored to LDS (a second
//     barrier).  One copy instead of two ping-pong copies is what lets a
//     128 x 128 level fit (130 * 130 * 8 B = 135 200 B).
// __syncthreads() is the only synchronisation; no workgroup waits for another.
//
// The arithmetic is hs_loop_kernel's, expression for expression (the
// quasi-Laplacian in its operand order, hs::update_px, -ffp-contract=off, IEEE
// division), and entry, Logger sums, decision, break and exit are the loop
// frame's (batch_loop.h): iterates, errors and iteration counts equal
// placement 0's bit for bit.  At the end the last iterate goes to the global
// buffer u[iterations & 1], pixels only, where launch_accumulate expects it.
#include "of2d_batch.h"

#include "hs_jacobi_impl.h"

namespace of2d {
namespace batch {

namespace {
// a pixel's LDS index (below 2^15: resident_fits) with bit 15 set on the border
// (0: the thread has no such pixel; a pixel's index is at least dx + 3)
constexpr unsigned kBorderBit = 0x8000u;
// Pixel k's half of its packed word.  The empty asm makes the word opaque in
// every iteration: without it the compiler unpacks all PPT indices, their
// neighbours' addresses and the border masks once before the loop and keeps
// them in registers, which the 128 of a 1024-thread workgroup's lane do not
// hold beside dI, It and the new values at PPT 16 (it spilled to scratch)
__device__ __forceinline__ unsigned pixel_word(unsigned packed, int k) {
    asm volatile("" : "+v"(packed));
    return (packed >> ((k & 1) * 16)) & 0xffffu;
}
// The same for a pixel's gradient at PPT 16: what the compiler would otherwise
// keep per pixel across the loop (update_px's denominator, twice, and its zero
// test) is 48 registers, and the kernel spilled.  The smaller instantiations
// have the room and keep those values
template <int PPT>
__device__ __forceinline__ float2 gradient_words(float2 g) {
    if constexpr (PPT > 8) asm volatile("" : "+v"(g.x), "+v"(g.y));
    return g;
}
}  // namespace

template <int PPT, bool CONV>
__global__ __launch_bounds__(kLoopThreads) void hs_resident_kernel(LoopArgs a) {
    constexpr int T = kLoopThreads;
    extern __shared__ float2 s_u[];  // the iterate: (dx + 2) x (dy + 2), ghost ring 0
    __shared__ int s_stop;
    const long pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    PairSlots ps;
    if (!loop_entry<CONV>(a, pair, tid, ps)) return;
    float2 *u0 = a.u0 + pair * a.stride, *u1 = a.u1 + pair * a.stride;
    const float2 *__restrict__ dI = a.dI + pair * a.stride;
    const float *__restrict__ It = a.It + pair * a.stride;
    const int dx = a.dx, dy = a.dy, P = a.P, npx = dx * dy;
    const int W = dx + 2, nlds = W * (dy + 2);

    for (int c = tid; c < nlds; c += T) s_u[c] = make_float2(0.0f, 0.0f);
    __syncthreads();
    // the thread's pixels: gradients to registers, the start iterate to LDS
    float2 g[PPT], nw[PPT];
    float t[PPT];
    unsigned pk[(PPT + 1) / 2];  // two pixels' LDS index and border bit per word
#pragma unroll
    for (int h = 0; h < (PPT + 1) / 2; h++) pk[h] = 0;
#pragma unroll
    for (int k = 0; k < PPT; k++) {
        const int idx = tid + k * T;
        g[k] = nw[k] = make_float2(0.0f, 0.0f);
        t[k] = 0.0f;
        if (idx < npx) {
            const int j = idx / dx, i = idx - j * dx;
            const long o = (long)j * P + i;
            const unsigned c = (unsigned)((j + 1) * W + (i + 1));
            const bool border = j == 0 || j == dy - 1 || i == 0 || i == dx - 1;
            pk[k >> 1] |= (c | (border ? kBorderBit : 0u)) << ((k & 1) * 16);
            g[k] = dI[o];
            t[k] = It[o];
            s_u[c] = u0[o];
        }
    }
    __syncthreads();

    unsigned bad = 0;
    int n = 0;
    for (int it = 0; it < a.niter; ++it) {
        double v[2] = {0.0, 0.0};
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            const unsigned w = pixel_word(pk[k >> 1], k);
            const int c = (int)(w & (kBorderBit - 1));
            if (c) {
                const float2 l = s_u[c - 1], r = s_u[c + 1], um = s_u[c - W], up = s_u[c + W];
                float2 q;
                // gradients.h:77-79: (((u[i-1] + u[i+1]) + u[j-1]) + u[j+1]) / 4.0f
                q.x = (((l.x + r.x) + um.x) + up.x) / 4.0f;
                q.y = (((l.y + r.y) + um.y) + up.y) / 4.0f;
                q = hs::zero_if((w & kBorderBit) != 0, q);  // :73-76
                const float2 gk = gradient_words<PPT>(g[k]);
                nw[k] = hs::update_px(q, gk.x, gk.y, t[k], a.alphasq, bad);
                if constexpr (CONV) logger_add(nw[k], s_u[c], v[0], v[1]);
            }
        }
        n = it + 1;
        // every thread has read its neighbours (block_sums holds a barrier)
        if constexpr (CONV)
            block_sums<2, kLoopWaves>(v, wave, lane);
        else
            __syncthreads();
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            const unsigned c = pixel_word(pk[k >> 1], k) & (kBorderBit - 1);
            if (c) s_u[c] = nw[k];
        }
        // the decision follows the stores: the order §4.6.5's registers hold for
        if constexpr (CONV) {
            if (tid == 0) s_stop = loop_decide(v[0], v[1], ps, it);
        }
        if (loop_break<CONV>(s_stop)) break;
    }
    // the last iterate to the buffer launch_accumulate reads from the count
    float2 *dst = (n & 1) ? u1 : u0;
    // (the pixel numbers formed afresh: kept from the set-up across the loop
    // they cost PPT registers)
    int tid_out = tid;
    asm volatile("" : "+v"(tid_out));
#pragma unroll
    for (int k = 0; k < PPT; k++) {
        const int idx = tid_out + k * T;
        if (idx < npx) {
            const int j = idx / dx, i = idx - j * dx;
            dst[(long)j * P + i] = s_u[(j + 1) * W + (i + 1)];
        }
    }
    loop_exit(a, pair, tid, lane, ps, n, (int)bad);
}

namespace {
template <class F>
void for_each_resident_kernel(F f) {
    f((const void *)hs_resident_kernel<1, false>);
    f((const void *)hs_resident_kernel<1, true>);
    f((const void *)hs_resident_kernel<2, false>);
    f((const void *)hs_resident_kernel<2, true>);
    f((const void *)hs_resident_kernel<4, false>);
    f((const void *)hs_resident_kernel<4, true>);
    f((const void *)hs_resident_kernel<8, false>);
    f((const void *)hs_resident_kernel<8, true>);
    f((const void *)hs_resident_kernel<16, false>);
    f((const void *)hs_resident_kernel<16, true>);
}

template <int PPT>
void launch_ppt(const LoopArgs &a, int B, bool conv, size_t lds, hipStream_t st) {
    if (conv)
        hipLaunchKernelGGL((hs_resident_kernel<PPT, true>), dim3(B), dim3(kLoopThreads), lds, st,
                           a);
    else
        hipLaunchKernelGGL((hs_resident_kernel<PPT, false>), dim3(B), dim3(kLoopThreads), lds, st,
                           a);
}
}  // namespace

bool resident_prepare() {
    bool ok = true;
    for_each_resident_kernel([&](const void *k) {
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                kResidentLdsBudget - kResidentLdsReserve) != hipSuccess)
            ok = false;
    });
    if (!ok) (void)hipGetLastError();  // the caller falls back to placement 0
    return ok;
}

void launch_hs_resident(const LoopArgs &a, int B, bool conv, hipStream_t st) {
    if (!resident_fits(a.dx, a.dy))
        throw std::invalid_argument("launch_hs_resident: the level does not fit");
    const size_t lds = resident_lds_bytes(a.dx, a.dy);
    switch (resident_ppt(a.dx, a.dy)) {
        case 1: launch_ppt<1>(a, B, conv, lds, st); break;
        case 2: launch_ppt<2>(a, B, conv, lds, st); break;
        case 4: launch_ppt<4>(a, B, conv, lds, st); break;
        case 8: launch_ppt<8>(a, B, conv, lds, st); break;
        default: launch_ppt<kResidentMaxPpt>(a, B, conv, lds, st); break;
    }
    OF2D_HIP(hipGetLastError());
}

}  // namespace batch
}  // namespace of2d
