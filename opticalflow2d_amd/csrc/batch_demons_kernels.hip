// batch_demons_kernels.hip — B independent Thirion's Demons registrations of
// one size (of2d_batch.h).
//
// The loop kernel: one workgroup per pair runs the niter iterations of
// DemonsThirions::get_update (src/regularization/Demons/DemonsThirions.cpp:
// 18-42) for its pair, with __syncthreads() as the only synchronisation.  An
// iteration is five stages through the pair's slices in global memory, a
// barrier after each (a stage reads its predecessor's values at other pixels):
//   1  W    = warp2d(Iaux, u)                        Image.cpp:119-182 (warp_px)
//   2  c    = -dI It / (|dI|^2 + It^2 si^2 / sx^2)   IterativeSolver.cpp:22-56,
//             with dI = grad(W), It = W - Iref       Demons.cpp:34-63
//   3  c   <- c (*) G(sigma_fluid)                   Field.tpp:209-269
//   4  mid  = accumulate(u, c) | u + c | u           DemonsThirions.cpp:33-38,
//                                                    Motion.cpp:113-178
//   5  u'   = mid (*) G(sigma_diffusion), plus the Logger sums against u
// Stages 3 and 4 are one pass: the update gathers u, not c.  Thread t takes
// pixels t, t + T, ... in ascending linear index in every stage.
//
// The per-pixel arithmetic restates the one-pair kernels' (demons_kernels.hip:
// demons_corr without the power-of-two multiply, whose bits are the
// division's; conv_px without the LDS tile; the borders of
// demons_force_kernel) and shares warp_px and accumulate_px with them,
// compiled with -ffp-contract=off and IEEE division: the iterates are
// bit-identical to the one-pair path's and the oracle's.
//
// Entry, convergence, break and exit are the loop frame's (batch_loop.h).
//
// A zero denominator (coord2d.h:95-100) sets the pair's kStatusDivZero; the
// workgroup learns it at the barrier after stage 2 and leaves the loop.
//
// EXP (option "diffeomorphic"): DemonsDiffeomorphic::get_update
// (DemonsDiffeomorphic.cpp:15-35), which is the Composition update with
// correspondence->exp() (Motion.cpp:247-275) between stages 3 and 4:
//   3   mid  = c (*) G(sigma_fluid), and the thread's maximum of Motion::maxabs
//   3a  nsq  = max(0, (int)ceil(1 + log2(sqrt(block maximum)))), through LDS
//   3b  mid *= 2^-nsq                                (only if nsq > 0)
//   3c  nsq squarings u <- u o u, mid -> corr -> mid -> ...
//   4   mid  = accumulate(u, E), E the buffer that holds the last squaring
// each followed by a barrier.  nsq is the pair's own, read from LDS after a
// barrier by every thread, so the branches and the loop it governs are
// block-uniform; for finite floats it is at most 65.  The expressions are
// maxabs_partial_kernel's, exp_prepare_kernel's and exp_scale_kernel's
// (demons_kernels.hip); the squaring is accumulate_px (see there).
#include "batch_demons_px.h"
#include "field_px.h"

namespace of2d {
namespace batch {

namespace {

template <int WAVES, bool CONV, int KW, bool EXP>
__global__ __launch_bounds__(64 * WAVES) void demons_loop_kernel(DemonsLoopArgs a) {
    constexpr int T = 64 * WAVES;
    const long pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    PairSlots ps;
    if (!loop_entry<CONV>(a, pair, tid, ps)) return;
    float2 *u0 = a.u0 + pair * a.stride, *u1 = a.u1 + pair * a.stride;
    const float *__restrict__ Iref = a.Iref + pair * a.sref;
    const float *__restrict__ Iaux = a.Iaux + pair * a.stride;
    float *W = a.W + pair * a.stride;
    float2 *C = a.corr + pair * a.stride, *M = a.mid + pair * a.stride;
    const int dx = a.dx, dy = a.dy, P = a.P, npx = dx * dy, kw = a.kw;
    // f(idx, i, j, o) for the thread's pixels (batch_loop.h)
    const auto pixels = [&](auto &&f) __attribute__((always_inline)) {
        for_pixels<T>(tid, npx, dx, P, f);
    };
    __shared__ int s_stop, s_bad;
    if (tid == 0) s_stop = s_bad = 0;  // published by the barrier after stage 1
    int n = 0;
    bool bad = false;
    for (int it = 0; it < a.niter; ++it) {
        const float2 *src = (it & 1) ? u1 : u0;
        float2 *dst = (it & 1) ? u0 : u1;
        // 1. the moving image by the iterate
        pixels([&](int, int i, int j, long o) {
            W[o] = warp_px(Iaux, src[o], Iaux[o], i, j, dx, dy, P);
        });
        __syncthreads();
        // 2. the correction (demons_corr_px, batch_demons_px.h)
        pixels([&](int, int i, int j, long o) {
            C[o] = demons_corr_px(W, Iref[o], o, i, j, dx, dy, P, a.sigma_isq, a.sigma_xsq, bad);
        });
        if (bad) s_bad = 1;
        __syncthreads();
        if (s_bad) break;  // block-uniform: the reference throws here
        if constexpr (EXP) {
            __shared__ int s_nsq;
            // 3. the smoothed correction into mid, and Motion::maxabs
            // (maxabs_fold, batch_demons_px.h)
            float mx = 0.0f;
            pixels([&](int, int i, int j, long o) {
                float2 c;
                if (!conv_direct<KW>(C, a.fluid, kw, i, j, dx, dy, P, c)) c = C[o];
                M[o] = c;
                mx = maxabs_fold(mx, c);
            });
            // 3a. the block's maximum (a thread without a pixel brings 0; the
            // barrier inside is stage 3's) and the squaring count
            // (exp_squarings, batch_demons_px.h)
            mx = block_max<WAVES>(mx, wave, lane);
            if (tid == 0) s_nsq = exp_squarings(mx);
            __syncthreads();
            const int nsq = s_nsq;  // block-uniform
            const float2 *E = M;    // the buffer that holds exp(c)
            if (nsq > 0) {          // Motion::exp returns early otherwise
                // 3b. Field<vector2d>::operator*=((float)std::pow(2, -nsq)),
                // exact; the thread's own pixels, in place
                const float sc = ldexpf(1.0f, -nsq);
                pixels([&](int, int, int, long o) {
                    float2 v = M[o];
                    v.x *= sc;
                    v.y *= sc;
                    M[o] = v;
                });
                __syncthreads();
                // 3c. u <- u o u (Motion.cpp:268-272: Mtmp = *this;
                // this->accumulate(*Mtmp)).  accumulate_px(f, f[o], f[o], ...)
                // is exp_square_kernel's expression: the same products and
                // sums in the same order with selects for its conditional
                // terms, c where floor(x + c) is outside the grid or the
                // weight is 0, and v / w skipped only where w is exactly 1.
                // A squaring gathers: from one buffer into the other (corr is
                // free once stage 3 has read it)
                float2 *from = M, *to = C;
                for (int q = 0; q < nsq; ++q) {
                    pixels([&](int, int i, int j, long o) {
                        const float2 c = from[o];
                        to[o] = accumulate_px(from, c, c, i, j, dx, dy, P);
                    });
                    __syncthreads();
                    float2 *t = from;
                    from = to;
                    to = t;
                }
                E = from;
            }
            // 4. motion->accumulate(*correspondence): E is read at the thread's
            // own pixel only and the gather is from src, so the write is in
            // place when E is mid
            pixels([&](int, int i, int j, long o) {
                M[o] = accumulate_px(src, E[o], src[o], i, j, dx, dy, P);
            });
        } else {
            // 3 + 4. the smoothed correction and the motion update
            pixels([&](int, int i, int j, long o) {
                float2 c;
                if (!conv_direct<KW>(C, a.fluid, kw, i, j, dx, dy, P, c)) c = C[o];
                const float2 own = src[o];
                float2 m = own;  // another enum value: no update
                if (a.mode == 0)
                    m = accumulate_px(src, c, own, i, j, dx, dy, P);
                else if (a.mode == 1)
                    m = make_float2(own.x + c.x, own.y + c.y);  // Field::operator+=
                M[o] = m;
            });
        }
        __syncthreads();
        // 5. the smoothed motion into the other buffer, and the Logger's terms
        double v[2] = {0.0, 0.0};
        pixels([&](int, int i, int j, long o) {
            float2 nw;
            if (!conv_direct<KW>(M, a.diff, kw, i, j, dx, dy, P, nw)) nw = M[o];
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
    loop_exit(a, pair, tid, lane, ps, n, bad);
}

}  // namespace

namespace {
template <int KW, bool EXP>
void launch_width(const DemonsLoopArgs &a, int B, bool conv, hipStream_t st) {
    if (conv)
        hipLaunchKernelGGL((demons_loop_kernel<kLoopWaves, true, KW, EXP>), dim3(B),
                           dim3(kLoopThreads), 0, st, a);
    else
        hipLaunchKernelGGL((demons_loop_kernel<kLoopWaves, false, KW, EXP>), dim3(B),
                           dim3(kLoopThreads), 0, st, a);
}
template <bool EXP>
void launch_exp(const DemonsLoopArgs &a, int B, bool conv, hipStream_t st) {
    switch (a.kw) {
        case 3: launch_width<3, EXP>(a, B, conv, st); break;
        case 5: launch_width<5, EXP>(a, B, conv, st); break;
        case 7: launch_width<7, EXP>(a, B, conv, st); break;
        default: launch_width<0, EXP>(a, B, conv, st); break;
    }
}
}  // namespace

// the usual widths are compiled in; every other one takes the runtime loops
void launch_demons_loop(const DemonsLoopArgs &a, int B, bool conv, hipStream_t st) {
    if (a.diffeomorphic)
        launch_exp<true>(a, B, conv, st);
    else
        launch_exp<false>(a, B, conv, st);
    OF2D_HIP(hipGetLastError());
}

}  // namespace batch
}  // namespace of2d
