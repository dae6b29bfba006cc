// hs_variants_tail.hip — the end-of-band exchange of the quad kernel
// (hs::jacobi4_kernel XCH, csrc/hs_jacobi_impl.h) against the instantiation
// without it, and a timing-only probe (XSYNC = false: the drain's six stencil
// steps and their row loads left out, no exchange, no barrier; its results are
// wrong and the product never launches it).  Not part of the product.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 \
//         -I opticalflow2d_amd/csrc tools/hs_variants_tail.hip -o tools/abx/hs_variants_tail
//   hs_variants_tail [grid 4096] [rounds 6] [launches 5000] [warm-up launches 1250]
// The defaults are bench.py's --steps 20 --warmup 5 (250 quads per step).
// Rounds alternate product, probe, exchange; per round and variant the time per
// launch by HIP events.  Before the timing: the exchange's field after 12
// iterations is compared byte for byte with the product instantiation's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hs_jacobi_impl.h"

using namespace of2d;

#define CK(x)                                                                        \
    do {                                                                             \
        hipError_t e = (x);                                                          \
        if (e != hipSuccess) {                                                       \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e)); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

typedef void (*K4)(const float2 *, float2 *, const float2 *, const float *, int, int, int, int,
                   int, float, int, int, double *, double *, double *, double *, int, int, int,
                   int, const unsigned *, int, int);

struct Bufs {
    float2 *u[2], *dI;
    float *It;
    double *partial;
    unsigned *rflag;
    int P, n, rows, gx, gy;
};

static void launch(K4 k, const Bufs &b, int it) {
    double *p = b.partial;
    hipLaunchKernelGGL(k, dim3(8 * ((b.gx * b.gy + 7) / 8)), dim3(256), 0, 0, b.u[it & 1],
                       b.u[(it & 1) ^ 1], b.dI, b.It, b.P, b.n, b.n, 0, b.n, 0.01f, -2, b.n + 2, p,
                       p + 2 * 16384, p + 4 * 16384, p + 6 * 16384, 0, b.gx, b.gy, b.rows, b.rflag,
                       -1, -1);
}

static float time_us(K4 k, const Bufs &b, int nl) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    CK(hipEventRecord(e0, 0));
    for (int it = 0; it < nl; it++) launch(k, b, it);
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    CK(hipGetLastError());
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    return 1000.0f * ms / nl;
}

int main(int argc, char **argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 4096;
    const int rounds = argc > 2 ? atoi(argv[2]) : 6;
    const int nl = argc > 3 ? atoi(argv[3]) : 5000;
    const int warm = argc > 4 ? atoi(argv[4]) : 1250;
    Bufs b;
    b.n = n;
    b.P = (n + 255) / 256 * 256;
    b.rows = hs3_rows(n, n);
    b.gx = (n + kHs3Out - 1) / kHs3Out;
    b.gy = (n + 4 * b.rows - 1) / (4 * b.rows);
    if (b.gx * b.gy > 16384) {
        fprintf(stderr, "grid too large for the partial buffer\n");
        return 2;
    }
    const size_t rows = (size_t)n + 4, cnt = (size_t)b.P * rows;  // two ghost j-lines each side
    float2 *base[3];
    float *baset;
    for (auto &p : base) CK(hipMalloc(&p, sizeof(float2) * cnt));
    CK(hipMalloc(&baset, sizeof(float) * cnt));
    b.u[0] = base[0] + 2 * b.P;
    b.u[1] = base[1] + 2 * b.P;
    b.dI = base[2] + 2 * b.P;
    b.It = baset + 2 * b.P;
    CK(hipMalloc(&b.partial, sizeof(double) * 8 * 16384));
    unsigned *status;
    CK(hipMalloc(&status, 64));
    CK(hipMemset(status, 0, 64));
    b.rflag = status + 8;
    {  // gradients of a smooth texture pair, as bench-like inputs
        auto tex = [](double x, double y) {
            return 0.5 + 0.1 * (sin(0.11 * x + 0.07 * y) + sin(0.05 * x - 0.13 * y + 1.0) +
                                sin(0.23 * x + 0.19 * y + 2.0));
        };
        std::vector<float> g(cnt * 2, 0.0f), t(cnt, 0.0f);
        for (int j = 0; j < n; j++)
            for (int i = 0; i < n; i++) {
                const size_t o = (size_t)(j + 2) * b.P + i;
                g[2 * o] = (float)((tex(i - 0.5, j + 0.75) - tex(i - 2.5, j + 0.75)) / 2);
                g[2 * o + 1] = (float)((tex(i - 1.5, j + 1.75) - tex(i - 1.5, j - 0.25)) / 2);
                t[o] = (float)(tex(i - 1.5, j + 0.75) - tex(i, j));
            }
        CK(hipMemcpy(base[2], g.data(), sizeof(float2) * cnt, hipMemcpyHostToDevice));
        CK(hipMemcpy(baset, t.data(), sizeof(float) * cnt, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(hs::hs_precheck_kernel<>, dim3(1024), dim3(256), 0, 0, base[2], (long)cnt,
                       b.P, 2, n, n, 0.01f, b.rflag, status);
    unsigned hflag = 0;
    CK(hipMemcpy(&hflag, b.rflag, sizeof hflag, hipMemcpyDeviceToHost));
    printf("grid %d^2, %d j-lines per wave, %d blocks, range flag %u\n", n, b.rows, b.gx * b.gy,
           hflag);

    const K4 product = hs::jacobi4_kernel<4, true, 4, 1, true>;
    const K4 probe = hs::jacobi4_kernel<4, true, 4, 1, true, true, false>;
    const K4 xch = hs::jacobi4_kernel<4, true, 4, 1, true, true, true>;
    const K4 ks[3] = {product, probe, xch};
    const char *kn[3] = {"product (no exchange)", "probe (drain skipped, wrong)", "exchange"};

    // bits: three launches of the product and of the exchange from zero
    std::vector<float2> A(cnt), B(cnt);
    std::vector<double> PA(8 * 16384), PB(8 * 16384);
    for (int v = 0; v < 2; v++) {
        CK(hipMemset(base[0], 0, sizeof(float2) * cnt));
        CK(hipMemset(base[1], 0, sizeof(float2) * cnt));
        CK(hipMemset(b.partial, 0, sizeof(double) * 8 * 16384));
        for (int it = 0; it < 3; it++) launch(v ? xch : product, b, it);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(v ? B.data() : A.data(), base[1], sizeof(float2) * cnt, hipMemcpyDeviceToHost));
        CK(hipMemcpy(v ? PB.data() : PA.data(), b.partial, sizeof(double) * 8 * 16384,
                     hipMemcpyDeviceToHost));
    }
    const bool same = memcmp(A.data(), B.data(), sizeof(float2) * cnt) == 0 &&
                      memcmp(PA.data(), PB.data(), sizeof(double) * 8 * 16384) == 0;
    printf("exchange after 12 iterations: %s\n",
           same ? "field and Logger partials bit-identical to the product" : "MISMATCH");
    if (!same) return 1;

    for (int v = 0; v < 3; v++) time_us(ks[v], b, warm);
    std::vector<float> t[3];
    for (int r = 0; r < rounds; r++) {
        for (int v = 0; v < 3; v++) t[v].push_back(time_us(ks[v], b, nl));
        printf("round %d: product %.3f  probe %.3f  exchange %.3f us/launch\n", r, t[0][r], t[1][r],
               t[2][r]);
        fflush(stdout);
    }
    double mean[3], spread[3];
    for (int v = 0; v < 3; v++) {
        double s = 0;
        for (float x : t[v]) s += x;
        mean[v] = s / rounds;
        spread[v] = (*std::max_element(t[v].begin(), t[v].end()) -
                     *std::min_element(t[v].begin(), t[v].end())) / mean[v];
        printf("%-30s mean %.3f us/launch, round-to-round spread %.3f %%\n", kn[v], mean[v],
               100 * spread[v]);
    }
    printf("probe gain %.3f %%  (gate: 3 x larger spread of product and probe = %.3f %%)\n",
           100 * (1 - mean[1] / mean[0]), 300 * std::max(spread[0], spread[1]));
    printf("exchange gain %.3f %%  (3 x larger spread of product and exchange = %.3f %%)\n",
           100 * (1 - mean[2] / mean[0]), 300 * std::max(spread[0], spread[2]));
    return 0;
}
