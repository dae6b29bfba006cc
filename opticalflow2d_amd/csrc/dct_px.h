// dct_px.h — the per-line arithmetic of the fast REDFT10 / REDFT01 (the maths:
// dct_kernels.hip's header), shared by the one-pair line kernel
// (dct_lines_kernel) and the batch's Curvature loop
// (batch_curvature_kernels.hip), so that a line's result is the same bits
// whichever kernel holds it.  fp64, compiled with -ffp-contract=off: a line's
// result depends on that line, its length and the twiddle table only.
//
// A block holds whole lines in LDS as double2 points: line l at
// z + l * (N + PAD), first the x plane's N/2 complex points, then the y
// plane's.  PAD (points) is 0 where lanes of a wave walk along a line, and 1
// where they walk across lines (columns): a line stride of N points would put
// every lane on one bank.  Flat index g = l * N + r (r < N) of the one-pair
// kernel is point dct_zi(g).  tw[0, N) = exp(-2 pi i m / N), tw[N, 2N) =
// exp(-i pi k / (2N)) (dct_table).
#pragma once

#include <hip/hip_runtime.h>

namespace of2d {

// position of frequency k after the in-place passes (radices 4, 4, ..., [2])
__device__ inline int dct_pos(int k, int N) {
    int M = N, p = 0;
    while (M >= 4) {
        M >>= 2;
        p += (k & 3) * M;
        k >>= 2;
    }
    if (M == 2) p += k & 1;
    return p;
}

__device__ inline double2 cmul(double2 a, double2 w) {
    return make_double2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

// REDFT10 output k of one plane from its half-length spectrum zs (digit-
// reversed): Re(c_k 2 V_k) for k <= n/2, -Im(c_{n-k} 2 V_{n-k}) above
__device__ inline double dct_fwd_out(const double2 *zs, const double2 *tw, int k, int N) {
    const int Nh = N >> 1, kk = k <= Nh ? k : N - k;
    const double2 uk = zs[dct_pos(kk & (Nh - 1), Nh)], un = zs[dct_pos((Nh - kk) & (Nh - 1), Nh)];
    const double2 a = make_double2(uk.x + un.x, uk.y - un.y);   // U_k + conj U_{n/2-k}
    const double2 b = make_double2(uk.y + un.y, un.x - uk.x);   // -i (U_k - conj U_{n/2-k})
    const double2 wb = cmul(b, tw[kk]);
    const double2 t = cmul(make_double2(a.x + wb.x, a.y + wb.y), tw[N + kk]);
    return k <= Nh ? t.x : -t.y;
}

// V_k = conj(c_k) (C_k - i C_{n-k}) of one plane's coefficients C (C_n = 0), 0 <= k <= n/2
__device__ inline double2 dct_inv_v(const double *C, const double2 *tw, int k, int N) {
    const double2 c = tw[N + k];
    const double er = c.x, ei = -c.y, p = C[k], q = k == 0 ? 0.0 : C[N - k];
    return make_double2(er * p + ei * q, ei * p - er * q);
}

// REDFT01 sample n of the reordered line v from the FFT of the swapped
// spectrum (digit-reversed): v_2j = Im, v_{2j+1} = Re of element j
__device__ inline double dct_inv_out(const double2 *zs, int n, int Nh) {
    const double2 r = zs[dct_pos(n >> 1, Nh)];
    return (n & 1) ? r.x : r.y;
}

template <int PAD>
__device__ __forceinline__ int dct_zi(int g, int logN) {
    return g + (g >> logN) * PAD;
}

// Elements 2m, 2m + 1 of line l: a of the x plane, b of the y plane.  REDFT10
// (KIND 0) reorders on the way in: v_m = x_2m, v_{N-1-m} = x_{2m+1}, and
// u_j = (v_2j, v_{2j+1}) is v itself; REDFT01 keeps C in natural order
template <int KIND, int PAD>
__device__ __forceinline__ void dct_put(double2 *z, int l, int m, int N, double2 a, double2 b) {
    double2 *zl = z + l * (N + PAD);
    if (KIND == 0) {
        double *vx = reinterpret_cast<double *>(zl), *vy = vx + N;
        vx[m] = a.x;
        vx[N - 1 - m] = a.y;
        vy[m] = b.x;
        vy[N - 1 - m] = b.y;
    } else {
        zl[m] = a;
        zl[(N >> 1) + m] = b;
    }
}

// REDFT01, after the lines are in place (and a barrier): U_k of each plane
// from its C, stored with real and imaginary parts swapped; every lane reads
// its inputs before any lane overwrites them.  T = lines * N flat points,
// T <= KPER * nt; ends with a barrier
template <int PAD, int KPER>
__device__ __forceinline__ void dct_inv_pre(double2 *z, int T, int N, int logN, const double2 *tw,
                                            int tid, int nt) {
    const int half = N >> 1;
    const double *zd = reinterpret_cast<const double *>(z);
    double2 ur[KPER];
#pragma unroll
    for (int q = 0; q < KPER; q++) {
        const int g = tid + q * nt;
        if (g < T) {
            const int l = g >> logN, r = g & (N - 1), pl = r >> (logN - 1), k = r & (half - 1);
            const double *C = zd + 2 * (long)l * (N + PAD) + (long)pl * N;
            const double2 vk = dct_inv_v(C, tw, k, N), vh = dct_inv_v(C, tw, half - k, N);
            const double2 s = make_double2(vk.x + vh.x, vk.y - vh.y);  // V_k + conj V_{N/2-k}
            const double2 d = make_double2(vk.x - vh.x, vk.y + vh.y);  // V_k - conj V_{N/2-k}
            const double2 w = tw[k];
            const double px = d.x * w.x + d.y * w.y, py = d.y * w.x - d.x * w.y;  // d conj(w^k)
            ur[q] = make_double2(s.y + px, s.x - py);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KPER; q++) {
        const int g = tid + q * nt;
        if (g < T) z[dct_zi<PAD>(g, logN)] = ur[q];  // line l, plane pl, k: l * N + pl * N/2 + k = g
    }
    __syncthreads();
}

// forward FFT of every half-length line, in place: decimation in frequency,
// radix-4 passes and a last radix-2 pass when log2 (N/2) is odd, a barrier
// after each pass
template <int PAD>
__device__ __forceinline__ void dct_fft(double2 *z, int T, int N, int logN, const double2 *tw,
                                        int tid, int nt) {
    int M = N >> 1, logQ = logN - 3;
    for (; M >= 4; M >>= 2, logQ -= 2) {
        const int Q = M >> 2, step = N / M;
        for (int t = tid; t < (T >> 2); t += nt) {
            const int j = t & (Q - 1), base = dct_zi<PAD>(((t >> logQ) * M) + j, logN);
            const double2 x0 = z[base], x1 = z[base + Q], x2 = z[base + 2 * Q],
                          x3 = z[base + 3 * Q];
            const double2 t0 = make_double2(x0.x + x2.x, x0.y + x2.y);
            const double2 t1 = make_double2(x0.x - x2.x, x0.y - x2.y);
            const double2 t2 = make_double2(x1.x + x3.x, x1.y + x3.y);
            const double2 t3 = make_double2(x1.y - x3.y, x3.x - x1.x);  // -i (x1 - x3)
            z[base] = make_double2(t0.x + t2.x, t0.y + t2.y);
            z[base + Q] = cmul(make_double2(t1.x + t3.x, t1.y + t3.y), tw[j * step]);
            z[base + 2 * Q] = cmul(make_double2(t0.x - t2.x, t0.y - t2.y), tw[2 * j * step]);
            z[base + 3 * Q] = cmul(make_double2(t1.x - t3.x, t1.y - t3.y), tw[3 * j * step]);
        }
        __syncthreads();
    }
    if (M == 2) {
        for (int t = tid; t < (T >> 1); t += nt) {
            const int i = dct_zi<PAD>(2 * t, logN);
            const double2 a = z[i], b = z[i + 1];
            z[i] = make_double2(a.x + b.x, a.y + b.y);
            z[i + 1] = make_double2(a.x - b.x, a.y - b.y);
        }
        __syncthreads();
    }
}

// Results 2m, 2m + 1 of line l after dct_fft: ya of the x plane, yb of the y
// plane.  REDFT01 reads back through the reordering: x_2m = v_m, x_{2m+1} =
// v_{N-1-m}
template <int KIND, int PAD>
__device__ __forceinline__ void dct_get(const double2 *z, int l, int m, int N, const double2 *tw,
                                        double (&ya)[2], double (&yb)[2]) {
    const int half = N >> 1;
    const double2 *zx = z + l * (N + PAD), *zy = zx + half;
    if (KIND == 0) {
#pragma unroll
        for (int e = 0; e < 2; e++) {
            ya[e] = dct_fwd_out(zx, tw, 2 * m + e, N);
            yb[e] = dct_fwd_out(zy, tw, 2 * m + e, N);
        }
    } else {
        ya[0] = dct_inv_out(zx, m, half);
        ya[1] = dct_inv_out(zx, N - 1 - m, half);
        yb[0] = dct_inv_out(zy, m, half);
        yb[1] = dct_inv_out(zy, N - 1 - m, half);
    }
}

// the eigenvalue product at the forward axis-x store: both planes times E at
// elements 2m (ev.x) and 2m + 1 (ev.y)
__device__ __forceinline__ void dct_scale(double (&ya)[2], double (&yb)[2], double2 ev) {
    ya[0] *= ev.x;
    ya[1] *= ev.y;
    yb[0] *= ev.x;
    yb[1] *= ev.y;
}

}  // namespace of2d
