// dct_kernels.hip — the 1-D REDFT10 / REDFT01 of Curvature along one axis as
// a fast transform: O(n log n) per line instead of the O(n^2) of the cosine
// GEMMs (curvature_kernels.hip).  Same definitions and scaling as c10 / c01
// in build_curvature (solvers.cpp):
//   REDFT10: Y_k = 2 sum_j X_j cos(pi (j + 1/2) k / n)
//   REDFT01: Y_k = X_0 + 2 sum_{j>=1} X_j cos(pi j (k + 1/2) / n)
//
// Makhoul's reordering onto an FFT of the same length (J. Makhoul, "A fast
// cosine transform in one and two dimensions", IEEE Trans. ASSP 28(1), 1980).
// With v_m = x_2m, v_{n-1-m} = x_{2m+1} and V = FFT_n(v),
//   REDFT10(x)_k = 2 Re(c_k V_k),  c_k = exp(-i pi k / (2n)),
// and, since c_k V_k = C_k - i C_{n-k} for the half-sized result C = Y / 2,
//   REDFT01(C) = the unnormalised inverse FFT of V_k = conj(c_k) (C_k - i C_{n-k})
// (C_n = 0), read back through the same reordering.  v is real, so its FFT is
// taken as a complex FFT of half the length: u_j = v_2j + i v_{2j+1}, U =
// FFT_{n/2}(u), and with w = exp(-2 pi i / n), U_{n/2} = U_0,
//   2 V_k = (U_k + conj U_{n/2-k}) - i w^k (U_k - conj U_{n/2-k}),  0 <= k <= n/2,
//   U_k = (V_k + conj V_{n/2-k}) + i conj(w^k) (V_k - conj V_{n/2-k})  (inverse).
// The x plane and the y plane of a line are two such half-length FFTs side by
// side in LDS (the work of one complex FFT of length n, a 4096-point line pair
// in 64 KiB): no arithmetic mixes the planes, so a plane of zeros stays zero on
// the bits.  The inverse FFT is the forward one on data with real and imaginary
// parts swapped, so there is a single FFT: in-place decimation in frequency,
// radix-4 passes (a last radix-2 pass when log2 (n/2) is odd) with one barrier
// between passes; the result is left in digit-reversed order and the
// post-processing reads it through dct_pos().  The per-line arithmetic itself
// is dct_px.h's, which the batch's Curvature loop shares.
//
// fp64 throughout; the twiddles are a host-built fp64 table (dct_table).
// Lines are contiguous (element k of line l at l * P + k, the y plane `plane`
// doubles further): every global access is a 16-B-per-lane coalesced segment.
// The axis-y pass of the solver runs the same kernel on a transposed copy
// (transpose_pair_kernel), so no access is strided.
#include <algorithm>
#include <cmath>

#include "dct_px.h"
#include "of2d_device.h"

namespace of2d {

namespace {
constexpr int kDctPoints = 1024;  // complex points per block below that line length
constexpr int kDctThreads = 512;  // largest block
}  // namespace

// KIND 0: REDFT10 (times E[k + line * P] when E != nullptr), 1: REDFT01, in
// place on lines [0, nlines) of the plane pair X | X + plane.  A block holds
// lpb lines in LDS (lpb * N = T complex points: per line the x plane's N/2
// points, then the y plane's); tw[0, N) = exp(-2 pi i m / N), tw[N, 2N) =
// exp(-i pi k / (2N)).
template <int KIND>
__global__ __launch_bounds__(kDctThreads) void dct_lines_kernel(double *X, long plane, int P,
                                                                int nlines, int N, int logN,
                                                                int lpb, const double2 *tw,
                                                                const double *E) {
    extern __shared__ double2 z[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int T = lpb * N, half = N >> 1;
    const int line0 = blockIdx.x * lpb;

    // load two elements per plane per lane; REDFT10 reorders on the way in
    for (int g = tid; g < (T >> 1); g += nt) {
        const int l = g >> (logN - 1), m = g & (half - 1);
        double2 a = make_double2(0.0, 0.0), b = a;
        if (line0 + l < nlines) {
            const double *pa = X + (long)(line0 + l) * P + 2 * m;
            a = *reinterpret_cast<const double2 *>(pa);
            b = *reinterpret_cast<const double2 *>(pa + plane);
        }
        dct_put<KIND, 0>(z, l, m, N, a, b);
    }
    __syncthreads();
    constexpr int kPer = kDctMaxN / kDctThreads;  // T / nt at most
    if (KIND == 1) dct_inv_pre<0, kPer>(z, T, N, logN, tw, tid, nt);
    dct_fft<0>(z, T, N, logN, tw, tid, nt);

    // store two elements per plane per lane
    for (int g = tid; g < (T >> 1); g += nt) {
        const int l = g >> (logN - 1), m = g & (half - 1);
        if (line0 + l >= nlines) continue;
        const long off = (long)(line0 + l) * P + 2 * m;
        double ya[2], yb[2];
        dct_get<KIND, 0>(z, l, m, N, tw, ya, yb);
        if (KIND == 0 && E) dct_scale(ya, yb, *reinterpret_cast<const double2 *>(E + off));
        *reinterpret_cast<double2 *>(X + off) = make_double2(ya[0], ya[1]);
        *reinterpret_cast<double2 *>(X + off + plane) = make_double2(yb[0], yb[1]);
    }
}

bool dct_fast_length(int n) { return n >= kDctMinN && n <= kDctMaxN && (n & (n - 1)) == 0; }

std::vector<double> dct_table(int n) {
    std::vector<double> h(4 * (size_t)n);
    for (int m = 0; m < n; m++) {
        const double a = 2.0 * M_PI * (double)m / (double)n;
        h[2 * (size_t)m] = std::cos(a);
        h[2 * (size_t)m + 1] = -std::sin(a);
        const double b = M_PI * (double)m / (2.0 * (double)n);
        h[2 * (size_t)(n + m)] = std::cos(b);
        h[2 * (size_t)(n + m) + 1] = -std::sin(b);
    }
    return h;
}

void launch_dct_lines(double *X, long plane, int P, int nlines, int n, int kind, const double *tw,
                      const double *E, hipStream_t st) {
    if (!dct_fast_length(n)) throw std::invalid_argument("dct_lines: unsupported line length");
    int logN = 0;
    while ((1 << logN) < n) logN++;
    const int lpb = n >= kDctPoints ? 1 : kDctPoints / n;
    const int T = lpb * n;
    const int nt = std::min(kDctThreads, std::max(64, T / 4));
    const size_t lds = (size_t)T * sizeof(double2);
    const dim3 grid((nlines + lpb - 1) / lpb);
    auto kern = kind == 0 ? dct_lines_kernel<0> : dct_lines_kernel<1>;
    if (lds > 64 * 1024)  // beyond the default per-block limit
        OF2D_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(kDctMaxN * sizeof(double2))));
    hipLaunchKernelGGL(kern, grid, dim3(nt), lds, st, X, plane, P, nlines, n, logN, lpb,
                       reinterpret_cast<const double2 *>(tw), kind == 0 ? E : nullptr);
    OF2D_HIP(hipGetLastError());
}

// D(j, i) = S(i, j) for i < n0, j < n1: S element (i, j) at i + j * Ps, D
// element (j, i) at j + i * Pd; blockIdx.z is the plane.  64 x 64 tiles, both
// sides in 512-B row segments.
__global__ __launch_bounds__(256) void transpose_pair_kernel(const double *__restrict__ S, long Ps,
                                                             long planeS, double *__restrict__ D,
                                                             long Pd, long planeD, int n0,
                                                             int n1) {
    __shared__ double tile[64][65];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int i0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
    S += blockIdx.z * planeS;
    D += blockIdx.z * planeD;
    for (int r = ty; r < 64; r += 4) {
        const int i = i0 + tx, j = j0 + r;
        if (i < n0 && j < n1) tile[r][tx] = S[i + (long)j * Ps];
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int i = i0 + r, j = j0 + tx;
        if (i < n0 && j < n1) D[j + (long)i * Pd] = tile[tx][r];
    }
}

void launch_transpose_pair(const double *S, long Ps, long planeS, double *D, long Pd, long planeD,
                           int n0, int n1, hipStream_t st) {
    hipLaunchKernelGGL(transpose_pair_kernel, dim3((n0 + 63) / 64, (n1 + 63) / 64, 2),
                       dim3(64, 4), 0, st, S, Ps, planeS, D, Pd, planeD, n0, n1);
    OF2D_HIP(hipGetLastError());
}

}  // namespace of2d
