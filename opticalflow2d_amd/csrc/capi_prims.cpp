// capi_prims.cpp — the test and diagnostic entries of libof2d.so
// (of2d_prims.h): one launch of the function the solvers call, on host arrays:
// dense float images (idx = i + j*dimx) and interleaved float2 motion fields.
#include "of2d_prims.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "of2d_batch.h"
#include "of2d_solvers.h"

using namespace of2d::capi;

namespace {
// the status word of a context (kStatus* bits), zeroed
struct StatusWord {
    of2d::DevArray<unsigned> w;
    StatusWord() { w.alloc(64); }
    unsigned read() {
        unsigned v = 0;
        fetch(&v, w.p, 1);
        return v;
    }
    // the Fluid loop's control words: c = {status, stop, regrid, mcur}
    void put_control(const unsigned *c) {
        unsigned h[64] = {};
        h[0] = c[0];
        h[of2d::kStopWord] = c[1];
        h[of2d::kFluidRegridWord] = c[2];
        h[of2d::kFluidMcurWord] = c[3];
        OF2D_HIP(hipMemcpy(w.p, h, sizeof h, hipMemcpyHostToDevice));
    }
    void get_control(unsigned *c) {
        unsigned h[64];
        fetch(h, w.p, 64);
        c[0] = h[0];
        c[1] = h[of2d::kStopWord];
        c[2] = h[of2d::kFluidRegridWord];
        c[3] = h[of2d::kFluidMcurWord];
    }
};
// a Gaussian of the product on the device, as Registration::loop_demons holds
// kfluid_ / kdiff_: float and double weights, the full weight sum
struct DeviceGaussian {
    of2d::DevArray<float> kf;
    of2d::DevArray<double> kd;
    of2d::DevArray<float> gs;  // gaussian_marginals
    double wfull = 0;
    // the launches' gs argument for `method`
    const float *factors(int method) const { return method ? gs.p : nullptr; }
    DeviceGaussian(int kw, float sigma) {
        const std::vector<double> k = of2d::gaussian_kernel(kw, sigma);
        std::vector<float> f(k.size());
        for (size_t t = 0; t < k.size(); t++) f[t] = (float)k[t];
        kf.alloc(k.size());
        kd.alloc(k.size());
        OF2D_HIP(hipMemcpy(kf.p, f.data(), sizeof(float) * f.size(), hipMemcpyHostToDevice));
        OF2D_HIP(hipMemcpy(kd.p, k.data(), sizeof(double) * k.size(), hipMemcpyHostToDevice));
        wfull = of2d::full_weight(k, kw);
        const std::vector<float> g = of2d::gaussian_marginals(k, kw);
        gs.alloc(g.size());
        OF2D_HIP(hipMemcpy(gs.p, g.data(), sizeof(float) * g.size(), hipMemcpyHostToDevice));
    }
};
// a level of the solver with nothing but Curvature's buffers, tables and
// eigenvalues
void curvature_level(of2d::Level &L, int dimx, int dimy, float alpha, float tau, int method) {
    L.dx = dimx;
    L.dy = dimy;
    L.P = of2d::pitch_for(dimx);
    of2d::solvers::alloc_level(L, OF2D_REG_CURVATURE);
    of2d::solvers::build_curvature(L, alpha, tau, method, nullptr);
}
}  // namespace

extern "C" {

// ------------------------------------------------------------------ transforms, Logger norms
int of2d_dct2d(double *a, int dimx, int dimy, int kind, int method, int *paths) {
    return prim(a && paths && dimx > 0 && dimy > 0 && (kind == 10 || kind == 1) &&
                    (method == 0 || method == 1),
                [&] {
                    of2d::Level L;
                    curvature_level(L, dimx, dimy, 0.0f, 0.0f, method);
                    paths[0] = L.cpath & 1;
                    paths[1] = (L.cpath >> 1) & 1;
                    upload(L.cbuf[0].p, L.P, a, dimx, dimy);
                    const double *res = of2d::solvers::curvature_dct2d(
                        L, kind == 1, L.cbuf[0].p, L.cbuf[1].p, nullptr, nullptr);
                    download(a, res, L.P, dimx, dimy);
                });
}

int of2d_dct_time_passes(int dimx, int dimy, int nlaunch, double *us) {
    return prim(us && nlaunch > 0 && of2d::dct_fast_length(dimx) && of2d::dct_fast_length(dimy), [&] {
        of2d::Level L;
        curvature_level(L, dimx, dimy, 0.0f, 0.0f, 1);
        const int P = L.P, Pt = of2d::pitch_for(dimy);
        const long plane = (long)P * dimy, planeT = (long)Pt * dimx;
        double *X = L.cbuf[0].p, *T = L.cbuf[1].p;
        hipEvent_t e0, e1;
        OF2D_HIP(hipEventCreate(&e0));
        OF2D_HIP(hipEventCreate(&e1));
        // the buffers hold zeros: the transforms' cost does not depend on the data
        for (int which = 0; which < 4; which++) {
            for (int k = -1; k < nlaunch; k++) {  // k = -1: one untimed launch
                if (k == 0) OF2D_HIP(hipEventRecord(e0, nullptr));
                if (which == 0)
                    of2d::launch_dct_lines(X, plane, P, dimy, dimx, 0, L.ctwx.p, L.cE.p, nullptr);
                else if (which == 1)
                    of2d::launch_dct_lines(X, plane, P, dimy, dimx, 1, L.ctwx.p, nullptr, nullptr);
                else if (which == 2)
                    of2d::launch_transpose_pair(X, P, plane, T, Pt, planeT, dimx, dimy, nullptr);
                else
                    of2d::launch_dct_lines(T, planeT, Pt, dimx, dimy, 0, L.ctwy.p, nullptr,
                                           nullptr);
            }
            OF2D_HIP(hipEventRecord(e1, nullptr));
            OF2D_HIP(hipEventSynchronize(e1));
            float ms = 0.0f;
            OF2D_HIP(hipEventElapsedTime(&ms, e0, e1));
            us[which] = 1000.0 * (double)ms / nlaunch;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    });
}

int of2d_motion_norms(const float *cur, const float *prev, int dimx, int dimy, int npairs,
                      float *sums, int *stats) {
    return prim(cur && prev && sums && dimx > 0 && dimy > 0 && npairs > 0, [&] {
        of2d::Field<float2> c, p;
        c.alloc(dimx, dimy);
        p.alloc(dimx, dimy);
        const size_t n = (size_t)dimx * dimy * 2;
        of2d::DevArray<unsigned char> ws;
        ws.alloc(of2d::seqnorm_workspace_bytes(dimx, dimy));
        of2d::DevArray<float> out;
        out.alloc(2 * (size_t)npairs);
        // the walk's counters: the 8 of the ABI, then 2 more (tools)
        constexpr int kSnDbg = 10;
        of2d::DevArray<int> dbg;
        dbg.alloc(kSnDbg * (size_t)npairs);
        for (int k = 0; k < npairs; k++) {
            // one workspace: each pair's walk predicts the next (its profile)
            upload(c.p, c.P, cur + k * n, dimx, dimy);
            upload(p.p, p.P, prev + k * n, dimx, dimy);
            of2d::launch_seqnorm(c.p, p.p, dimx, dimy, c.P, ws.p, k > 0, out.p + 2 * k,
                                 dbg.p + kSnDbg * k, nullptr);
        }
        OF2D_HIP(hipMemcpy(sums, out.p, 2 * sizeof(float) * npairs, hipMemcpyDeviceToHost));
        if (stats)
            OF2D_HIP(hipMemcpy2D(stats, 8 * sizeof(int), dbg.p, kSnDbg * sizeof(int),
                                 8 * sizeof(int), npairs, hipMemcpyDeviceToHost));
    });
}

int of2d_motion_norms_chain(const float *u, int dimx, int dimy, int niter, int batch,
                            float *sums, int *stats) {
    return prim(u && sums && dimx > 0 && dimy > 0 && niter > 0 && batch >= 1 && batch <= 3, [&] {
        const size_t n = (size_t)dimx * dimy * 2;
        std::vector<of2d::Field<float2>> f((size_t)niter + 1);
        for (size_t k = 0; k <= (size_t)niter; k++) upload(f[k], u + k * n, dimx, dimy);
        // four sets of three workspaces rotated per batch, as the registration
        // loops (Registration::kSeqSets): batch g's profile is batch g - 4's
        constexpr int kSets = 4;
        of2d::DevArray<unsigned char> ws[3 * kSets];
        bool used[3 * kSets] = {};
        for (auto &w : ws) w.alloc(of2d::seqnorm_workspace_bytes(dimx, dimy));
        of2d::DevArray<float> out;
        out.alloc(2 * (size_t)niter);
        constexpr int kSnDbg = 10;
        of2d::DevArray<int> dbg;
        dbg.alloc(kSnDbg * (size_t)niter);
        for (int t = 0, g = 0; t < niter; g++) {
            of2d::SeqnormBatch B;
            B.K = std::min(batch, niter - t);
            for (int i = 0; i <= B.K; i++) B.u[i] = f[(size_t)t + i].p;
            for (int i = 0; i < B.K; i++) {
                const int w = 3 * (g % kSets) + i;
                B.ws[i] = ws[w].p;
                B.use_profile[i] = used[w];
                used[w] = true;
                B.out[i] = out.p + 2 * (size_t)(t + i);
                B.dbg[i] = dbg.p + kSnDbg * (size_t)(t + i);
            }
            of2d::launch_seqnorm_pass(B, dimx, dimy, f[0].P, nullptr);
            of2d::launch_seqnorm_refine(B, dimx, dimy, f[0].P, nullptr);
            of2d::launch_seqnorm_walk(B, dimx, dimy, f[0].P, nullptr);
            t += B.K;
        }
        OF2D_HIP(hipMemcpy(sums, out.p, 2 * sizeof(float) * niter, hipMemcpyDeviceToHost));
        if (stats)
            OF2D_HIP(hipMemcpy2D(stats, 8 * sizeof(int), dbg.p, kSnDbg * sizeof(int),
                                 8 * sizeof(int), niter, hipMemcpyDeviceToHost));
    });
}

// ------------------------------------------------------------------ field / Demons primitives
int of2d_prim_warp(const float *src, const float *u, int dimx, int dimy, float *out) {
    return prim(src && u && out && dimx > 0 && dimy > 0, [&] {
        of2d::Field<float> s, d;
        of2d::Field<float2> m;
        upload(s, src, dimx, dimy);
        upload(m, u, dimx, dimy);
        upload(d, nullptr, dimx, dimy);
        of2d::launch_warp(s.p, m.p, d.p, dimx, dimy, s.P, nullptr);
        download(out, d.p, d.P, dimx, dimy);
    });
}

int of2d_prim_accumulate(const float *m_old, const float *v, int dimx, int dimy, float *out) {
    return prim(m_old && v && out && dimx > 0 && dimy > 0, [&] {
        of2d::Field<float2> mo, c, mn;
        upload(mo, m_old, dimx, dimy);
        upload(c, v, dimx, dimy);
        upload(mn, nullptr, dimx, dimy);
        of2d::launch_accumulate(mo.p, c.p, mn.p, dimx, dimy, mo.P, nullptr);
        download(out, mn.p, mn.P, dimx, dimy);
    });
}

int of2d_prim_regrid(const float *m_old, const float *est, const float *Imov, int dimx, int dimy,
                     float *m_new, float *est0, float *Iaux) {
    return prim(m_old && est && Imov && m_new && est0 && Iaux && dimx > 0 && dimy > 0, [&] {
        of2d::Field<float2> mo, e, e0, mn;
        of2d::Field<float> im, ia;
        upload(mo, m_old, dimx, dimy);
        upload(e, est, dimx, dimy);
        upload(e0, est, dimx, dimy);  // not zero: the launch has to clear it
        upload(mn, nullptr, dimx, dimy);
        upload(im, Imov, dimx, dimy);
        upload(ia, nullptr, dimx, dimy);
        of2d::launch_regrid(mo.p, e.p, e0.p, mn.p, im.p, ia.p, dimx, dimy, mo.P, nullptr);
        download(m_new, mn.p, mn.P, dimx, dimy);
        download(est0, e0.p, e0.P, dimx, dimy);
        download(Iaux, ia.p, ia.P, dimx, dimy);
    });
}

int of2d_prim_compose_zero(const float *v, int dimx, int nrows, int row0, int dimy, float *out) {
    return prim(v && out && dimx > 0 && nrows > 0 && row0 >= 0 && row0 + nrows <= dimy, [&] {
        of2d::Field<float2> c, o;
        upload(c, v, dimx, nrows);
        upload(o, nullptr, dimx, nrows);
        of2d::launch_compose_zero(c.p, o.p, dimx, nrows, c.P, row0, dimy, nullptr);
        download(out, o.p, o.P, dimx, nrows);
    });
}

int of2d_prim_add_motion(const float *a, const float *b, int dimx, int dimy, float *out) {
    return prim(a && b && out && dimx > 0 && dimy > 0, [&] {
        of2d::Field<float2> x, y, o;
        upload(x, a, dimx, dimy);
        upload(y, b, dimx, dimy);
        upload(o, nullptr, dimx, dimy);
        of2d::launch_add_motion(x.p, y.p, o.p, dimx, dimy, x.P, nullptr);
        download(out, o.p, o.P, dimx, dimy);
    });
}

int of2d_prim_resample(int what, const float *in, int dxi, int dyi, float *out, int dxo, int dyo) {
    return prim(in && out && dxi > 0 && dyi > 0 && what >= 0 && what <= 2, [&] {
        // the launches refuse the sizes the reference refuses, before any field
        if (what == 0) {
            of2d::Field<float> a, o;
            if (dxo > 0 && dyo > 0) {
                upload(a, in, dxi, dyi);
                upload(o, out, dxo, dyo);
            }
            of2d::launch_downsample_image(a.p, dxi, dyi, a.P, o.p, dxo, dyo, o.P, nullptr);
            download(out, o.p, o.P, dxo, dyo);
            return;
        }
        of2d::Field<float2> a, o;
        if (dxo > 0 && dyo > 0) {
            upload(a, in, dxi, dyi);
            upload(o, out, dxo, dyo);
        }
        if (what == 1)
            of2d::launch_downsample_motion(a.p, dxi, dyi, a.P, o.p, dxo, dyo, o.P, nullptr);
        else
            of2d::launch_upsample_motion(a.p, dxi, dyi, a.P, o.p, dxo, dyo, o.P, nullptr);
        download(out, o.p, o.P, dxo, dyo);
    });
}

int of2d_prim_gradients(const float *Iref, const float *Iaux, int dimx, int dimy, int row0,
                        int nrows, float *dI, float *It) {
    return prim(Iref && Iaux && dI && It && dimx > 0 && nrows > 0 && row0 >= 0 &&
                    row0 + nrows <= dimy,
                [&] {
                    // the slab's rows, and in its ghost j-lines the neighbours' image rows
                    of2d::Field<float> r, a, t;
                    of2d::Field<float2> g;
                    upload(r, Iref + (size_t)row0 * dimx, dimx, nrows);
                    upload(a, nullptr, dimx, nrows);
                    upload(g, nullptr, dimx, nrows);
                    upload(t, nullptr, dimx, nrows);
                    const int lo = row0 > 0 ? row0 - 1 : row0;
                    const int hi = row0 + nrows < dimy ? row0 + nrows + 1 : row0 + nrows;
                    upload(a.p + (long)(lo - row0) * a.P, a.P, Iaux + (size_t)lo * dimx, dimx,
                           hi - lo);
                    of2d::launch_gradients_rows(r.p, a.p, g.p, t.p, dimx, nrows, r.P, row0, dimy,
                                                nullptr);
                    download(dI, g.p, g.P, dimx, nrows);
                    download(It, t.p, t.P, dimx, nrows);
                });
}

int of2d_prim_demons_force(const float *Iref, const float *Imov, const float *u, int dimx,
                           int dimy, float sigma_i, float sigma_x, float *corr,
                           unsigned *status) {
    return prim(Iref && Imov && u && corr && status && dimx > 0 && dimy > 0, [&] {
        of2d::Field<float> r, m;
        of2d::Field<float2> f, c;
        upload(r, Iref, dimx, dimy);
        upload(m, Imov, dimx, dimy);
        upload(f, u, dimx, dimy);
        upload(c, nullptr, dimx, dimy);
        StatusWord st;
        // Demons.cpp:48-49
        of2d::launch_demons_force(r.p, m.p, f.p, c.p, dimx, dimy, r.P, sigma_i * sigma_i,
                                  sigma_x * sigma_x, st.w.p, nullptr);
        download(corr, c.p, c.P, dimx, dimy);
        *status = st.read();
    });
}

int of2d_prim_smooth_compose(const float *corr, const float *u, int dimx, int dimy, int kw,
                             float sigma, int mode, float *out, double *wfull, int method,
                             int *path) {
    return prim(corr && u && out && dimx > 0 && dimy > 0 && kw >= 1 && mode >= 0 && mode <= 3 &&
                    path && (method == 0 || method == 1),
                [&] {
                    of2d::Field<float2> c, f, o;
                    upload(c, corr, dimx, dimy);
                    upload(f, u, dimx, dimy);
                    upload(o, nullptr, dimx, dimy);
                    DeviceGaussian g(kw, sigma);
                    if (wfull) *wfull = g.wfull;
                    *path = of2d::launch_smooth_compose(c.p, f.p, o.p, dimx, dimy, c.P, g.kf.p,
                                                        g.kd.p, kw, g.wfull, mode, nullptr,
                                                        g.factors(method));
                    download(out, o.p, o.P, dimx, dimy);
                });
}

int of2d_prim_smooth_norm(const float *umid, const float *prev, int dimx, int dimy, int kw,
                          float sigma, float *out, double *sums, int method, int *path) {
    return prim(umid && prev && out && dimx > 0 && dimy > 0 && kw >= 1 && path &&
                    (method == 0 || method == 1), [&] {
        of2d::Field<float2> m, p, o;
        upload(m, umid, dimx, dimy);
        upload(p, prev, dimx, dimy);
        upload(o, nullptr, dimx, dimy);
        DeviceGaussian g(kw, sigma);
        const int nb = of2d::conv_nblocks(dimx, dimy);
        of2d::DevArray<double> part, red;
        part.alloc(2 * (size_t)nb);
        red.alloc(2);
        // sums: the Logger partials reduced as the fp64 Logger mode reduces
        // them; none: the launch of the default mode, without partials
        *path = of2d::launch_smooth_norm(m.p, p.p, o.p, dimx, dimy, m.P, g.kf.p, g.kd.p, kw,
                                         g.wfull, sums ? part.p : nullptr, nullptr,
                                         g.factors(method));
        if (sums) {
            of2d::launch_reduce_partials(part.p, nb, 1, red.p, nullptr);
            fetch(sums, red.p, 2);
        }
        download(out, o.p, o.P, dimx, dimy);
    });
}

int of2d_prim_demons_update(const float *Iref, const float *Imov, const float *u, int dimx,
                            int dimy, float sigma_i, float sigma_x, int kw, float sigma_fluid,
                            int mode, float *out, unsigned *status, int method, int *path) {
    return prim(Iref && Imov && u && out && status && dimx > 0 && dimy > 0 && kw >= 1 &&
                    mode >= 0 && mode <= 3 && path && (method == 0 || method == 1),
                [&] {
                    of2d::Field<float> r, m;
                    of2d::Field<float2> f, c, o;
                    upload(r, Iref, dimx, dimy);
                    upload(m, Imov, dimx, dimy);
                    upload(f, u, dimx, dimy);
                    upload(c, nullptr, dimx, dimy);
                    upload(o, nullptr, dimx, dimy);
                    DeviceGaussian g(kw, sigma_fluid);
                    StatusWord st;
                    *path = of2d::launch_demons_update(
                        r.p, m.p, f.p, c.p, o.p, dimx, dimy, r.P, sigma_i * sigma_i,
                        sigma_x * sigma_x, g.kf.p, g.kd.p, kw, g.wfull, mode, st.w.p, nullptr,
                        g.factors(method));
                    download(out, o.p, o.P, dimx, dimy);
                    *status = st.read();
                });
}

int of2d_prim_motion_exp(float *f, int dimx, int dimy, float sigma_i, float sigma_x, int *nsq,
                         unsigned *status) {
    return prim(f && nsq && status && dimx > 0 && dimy > 0, [&] {
        of2d::Field<float2> a, b;
        upload(a, f, dimx, dimy);
        upload(b, nullptr, dimx, dimy);
        constexpr int nparts = 256;  // Registration::loop_demons
        of2d::DevArray<float> part, maxabs;
        of2d::DevArray<int> n;
        part.alloc(nparts);
        maxabs.alloc(1);
        n.alloc(1);
        StatusWord st;
        float2 *res = nullptr;
        of2d::launch_motion_exp(a.p, b.p, dimx, dimy, a.P,
                                of2d::exp_squarings_bound(sigma_i * sigma_i, sigma_x * sigma_x),
                                part.p, nparts, n.p, maxabs.p, st.w.p, &res, nullptr);
        download(f, res, a.P, dimx, dimy);
        OF2D_HIP(hipMemcpy(nsq, n.p, sizeof(int), hipMemcpyDeviceToHost));
        *status = st.read();
    });
}

int of2d_prim_d2f(const double *in, int dimx, int dimy, float *out) {
    return prim(in && out && dimx > 0 && dimy > 0, [&] {
        of2d::DevArray<double> d;
        d.alloc((size_t)dimx * dimy);
        OF2D_HIP(hipMemcpy(d.p, in, sizeof(double) * d.n, hipMemcpyHostToDevice));
        of2d::Field<float> o;
        upload(o, nullptr, dimx, dimy);
        of2d::launch_d2f(d.p, dimx, dimy, o.p, o.P, 0, nullptr);
        download(out, o.p, o.P, dimx, dimy);
    });
}

int of2d_prim_f2d(const float *in, int dimx, int dimy, double *out) {
    return prim(in && out && dimx > 0 && dimy > 0, [&] {
        of2d::Field<float> a;
        upload(a, in, dimx, dimy);
        of2d::DevArray<double> d;
        d.alloc((size_t)dimx * dimy);
        of2d::launch_f2d(a.p, a.P, dimx, dimy, d.p, nullptr);
        fetch(out, d.p, d.n);
    });
}

int of2d_prim_motion_to_planar(const float *m, int dimx, int dimy, double *out) {
    return prim(m && out && dimx > 0 && dimy > 0, [&] {
        of2d::Field<float2> a;
        upload(a, m, dimx, dimy);
        of2d::DevArray<double> d;
        d.alloc(2 * (size_t)dimx * dimy);
        of2d::launch_motion_to_planar(a.p, a.P, dimx, dimy, d.p, nullptr);
        fetch(out, d.p, d.n);
    });
}

// ------------------------------------------------------------------ Curvature primitives
int of2d_prim_curv_rhs(const float *u, const float *dI, const float *It, float tau, int dimx,
                       int dimy, double *out_x, double *out_y) {
    return prim(u && dI && It && out_x && out_y && dimx > 0 && dimy > 0, [&] {
        of2d::Field<float2> m, g;
        of2d::Field<float> t;
        upload(m, u, dimx, dimy);
        upload(g, dI, dimx, dimy);
        upload(t, It, dimx, dimy);
        const long plane = (long)m.P * dimy;
        of2d::DevArray<double> X;
        X.alloc(2 * (size_t)plane);
        of2d::launch_curv_rhs(m.p, g.p, t.p, tau, dimx, dimy, m.P, X.p, plane, nullptr);
        download(out_x, X.p, m.P, dimx, dimy);
        download(out_y, X.p + plane, m.P, dimx, dimy);
    });
}

int of2d_prim_curv_eigen(int dimx, int dimy, float alpha, float tau, int method, double *out) {
    return prim(out && dimx > 0 && dimy > 0 && (method == 0 || method == 1), [&] {
        of2d::Level L;
        curvature_level(L, dimx, dimy, alpha, tau, method);
        download(out, L.cE.p, L.P, dimx, dimy);
    });
}

int of2d_prim_curv_dct2d(double *ax, double *ay, int dimx, int dimy, int kind, int method,
                         int with_eig, float alpha, float tau, int *paths) {
    return prim(ax && ay && paths && dimx > 0 && dimy > 0 && (kind == 10 || kind == 1) &&
                    (method == 0 || method == 1) && (with_eig == 0 || (with_eig == 1 && kind == 10)),
                [&] {
                    of2d::Level L;
                    curvature_level(L, dimx, dimy, alpha, tau, method);
                    paths[0] = L.cpath & 1;
                    paths[1] = (L.cpath >> 1) & 1;
                    const long plane = (long)L.P * dimy;
                    upload(L.cbuf[0].p, L.P, ax, dimx, dimy);
                    upload(L.cbuf[0].p + plane, L.P, ay, dimx, dimy);
                    const double *res = of2d::solvers::curvature_dct2d(
                        L, kind == 1, L.cbuf[0].p, L.cbuf[1].p, with_eig ? L.cE.p : nullptr,
                        nullptr);
                    download(ax, res, L.P, dimx, dimy);
                    download(ay, res + plane, L.P, dimx, dimy);
                });
}

int of2d_prim_curv_construct(const double *zx, const double *zy, const float *u, float div,
                             int dimx, int dimy, float *out, double *sums) {
    return prim(zx && zy && u && out && sums && dimx > 0 && dimy > 0, [&] {
        of2d::Field<float2> m, o;
        upload(m, u, dimx, dimy);
        upload(o, nullptr, dimx, dimy);
        const long plane = (long)m.P * dimy;
        of2d::DevArray<double> Z, part;
        Z.alloc(2 * (size_t)plane);
        upload(Z.p, m.P, zx, dimx, dimy);
        upload(Z.p + plane, m.P, zy, dimx, dimy);
        const int nb = of2d::curv_nblocks(dimx, dimy);
        part.alloc(2 * (size_t)nb);
        of2d::launch_curv_construct(Z.p, plane, m.p, o.p, div, dimx, dimy, m.P, part.p, nullptr);
        download(out, o.p, o.P, dimx, dimy);
        std::vector<double> h(2 * (size_t)nb);
        OF2D_HIP(hipMemcpy(h.data(), part.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
        sums[0] = sums[1] = 0.0;
        for (int b = 0; b < nb; b++) {
            sums[0] += h[2 * (size_t)b];
            sums[1] += h[2 * (size_t)b + 1];
        }
    });
}

// ------------------------------------------------------------------ analysis timing
int of2d_analysis_time_kernels(int dimx, int dimy, int nlaunch, double *us) {
    if (!us || nlaunch <= 0) return refuse(nullptr, "of2d_analysis_time_kernels: us, nlaunch");
    if (dimx < 2 || dimy < 2)
        return refuse(nullptr, "analysis timing: the field needs dimx >= 2 and dimy >= 2");
    return prim(true, [&] {
        // the inverse's test field (tests/test_gpu_analysis.py), amplitude 3
        std::vector<float> hu((size_t)dimx * dimy * 2);
        const double tp = 6.283185307179586;
        for (int j = 0; j < dimy; j++)
            for (int i = 0; i < dimx; i++) {
                float *p = &hu[((size_t)j * dimx + i) * 2];
                p[0] = (float)(3.0 * sin(tp * i / dimx + 0.3) * cos(tp * j / dimy));
                p[1] = (float)(2.1 * cos(2 * tp * i / dimx) * sin(tp * j / dimy + 0.5));
            }
        of2d::Field<float2> f, v0, v1;
        of2d::Field<float> jm;
        upload(f, hu.data(), dimx, dimy);
        upload(v0, nullptr, dimx, dimy);
        upload(v1, nullptr, dimx, dimy);
        upload(jm, nullptr, dimx, dimy);
        of2d::DevArray<of2d::JacPartial> part;
        part.alloc((size_t)of2d::jacobian_nblocks(dimx, dimy));
        of2d::DevArray<double> ds;
        ds.alloc(5);
        of2d::DevArray<unsigned> ctl;
        ctl.alloc(of2d::invert_ctl_words(4));
        // an iterate near the fixed point: the gather pattern of a real update
        const of2d::InvertResult r =
            of2d::invert_field(f.p, v0.p, v1.p, dimx, dimy, f.P, 4, 1e-3f, ctl.p, nullptr, nullptr);
        float2 *vin = r.v, *vout = r.v == v0.p ? v1.p : v0.p;
        hipEvent_t e0, e1;
        OF2D_HIP(hipEventCreate(&e0));
        OF2D_HIP(hipEventCreate(&e1));
        for (int which = 0; which < 2; which++) {
            for (int k = -1; k < nlaunch; k++) {  // k = -1: one untimed launch
                if (k == 0) OF2D_HIP(hipEventRecord(e0, nullptr));
                if (which == 0)
                    of2d::launch_jacobian(f.p, dimx, dimy, f.P, jm.p, part.p, ds.p, nullptr);
                else  // update 0 reads no control word: every launch does the work
                    of2d::launch_invert_step(f.p, vin, vout, dimx, dimy, f.P, 0, 1e-3f, ctl.p, 4,
                                             nullptr);
            }
            OF2D_HIP(hipEventRecord(e1, nullptr));
            OF2D_HIP(hipEventSynchronize(e1));
            float ms = 0.0f;
            OF2D_HIP(hipEventElapsedTime(&ms, e0, e1));
            us[which] = 1000.0 * (double)ms / nlaunch;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    });
}

}  // extern "C"

// ------------------------------------------------------------------ SOR / Fluid / Elastic primitives
namespace {
constexpr unsigned kNoStop = 0x7f7f7f7fu;  // the stop word before any break (loop_fluid)

// A level with nothing but the buffers solvers::alloc_level gives Elastic
// (reg 2) or Fluid (reg 5), the 64-word status / control buffer of a context,
// and the host side of the skewed working array and the hand-off granules.
struct SorLevel {
    of2d::Level L;
    StatusWord st;
    std::vector<float2> hvb;   // the whole vb allocation (from L.vb.base)
    std::vector<unsigned> hH;  // every granule region
    SorLevel(int dimx, int dimy, int reg) {
        L.dx = dimx;
        L.dy = dimy;
        L.P = of2d::pitch_for(dimx);
        of2d::solvers::alloc_level(L, reg);
        hvb.assign(2 * L.vb.count, make_float2(0.0f, 0.0f));
        hH.assign(2 * L.sorH.n, 0u);
    }
    float2 &cell(long k) { return hvb[(size_t)(2L * L.P + k)]; }  // k: sor_v / sor_b
    unsigned *granule0(int j) { return &hH[4 * (size_t)(of2d::kSorPadRows + j)]; }
    // every word of both allocations (the padding cells, the never-published
    // granule rows), before put() writes the image's cells
    void fill(unsigned word) {
        float f;
        memcpy(&f, &word, sizeof f);
        std::fill(hvb.begin(), hvb.end(), make_float2(f, f));
        std::fill(hH.begin(), hH.end(), word);
    }
    // v and b of the image pixels (a null plane keeps the fill) and the
    // region-0 granules: column 0 of v tagged with `epoch` (gran non-null: those
    // dimy x 4 words instead)
    void put(const float *v, const float *b, unsigned epoch, const unsigned *gran = nullptr) {
        const float2 *v2 = reinterpret_cast<const float2 *>(v);
        const float2 *b2 = reinterpret_cast<const float2 *>(b);
        for (int j = 0; j < L.dy; j++) {
            for (int i = 0; i < L.dx; i++) {
                if (v) cell(of2d::sor_v(i, j, L.P)) = v2[(size_t)j * L.dx + i];
                if (b) cell(of2d::sor_b(i, j, L.P)) = b2[(size_t)j * L.dx + i];
            }
            unsigned *g = granule0(j);
            if (gran) {
                memcpy(g, gran + 4 * (size_t)j, 16);
            } else {
                memcpy(g, &cell(of2d::sor_v(0, j, L.P)), 8);
                g[2] = g[3] = epoch;
            }
        }
        OF2D_HIP(hipMemcpy(L.vb.base, hvb.data(), L.vb.bytes(), hipMemcpyHostToDevice));
        OF2D_HIP(hipMemcpy(L.sorH.p, hH.data(), hH.size() * sizeof(unsigned),
                           hipMemcpyHostToDevice));
    }
    // the region-0 granules' tags for the next sweep (their values, column 0
    // of v, are never relaxed)
    void retag(unsigned epoch) {
        for (int j = 0; j < L.dy; j++) granule0(j)[2] = granule0(j)[3] = epoch;
        OF2D_HIP(hipMemcpy(reinterpret_cast<unsigned *>(L.sorH.p) + 4 * (size_t)of2d::kSorPadRows,
                           granule0(0), 16 * (size_t)L.dy, hipMemcpyHostToDevice));
    }
    void control(unsigned status, unsigned stop, unsigned regrid, unsigned mcur) {
        const unsigned c[4] = {status, stop, regrid, mcur};
        st.put_control(c);
    }
    // the unskewed planes and the region-0 granules (dimy x 4 words)
    void get(float *v, float *b, unsigned *gran) {
        OF2D_HIP(hipStreamSynchronize(nullptr));
        OF2D_HIP(hipMemcpy(hvb.data(), L.vb.base, L.vb.bytes(), hipMemcpyDeviceToHost));
        OF2D_HIP(hipMemcpy(hH.data(), L.sorH.p, hH.size() * sizeof(unsigned),
                           hipMemcpyDeviceToHost));
        float2 *v2 = reinterpret_cast<float2 *>(v), *b2 = reinterpret_cast<float2 *>(b);
        for (int j = 0; j < L.dy; j++) {
            for (int i = 0; i < L.dx; i++) {
                if (v) v2[(size_t)j * L.dx + i] = cell(of2d::sor_v(i, j, L.P));
                if (b) b2[(size_t)j * L.dx + i] = cell(of2d::sor_b(i, j, L.P));
            }
            if (gran) memcpy(gran + 4 * (size_t)j, granule0(j), 16);
        }
    }
};
// a FluidReport where the Fluid loop keeps its ring: host memory the device
// writes; every byte 0xAB until a kernel writes it
struct HostReport {
    of2d::FluidReport *p = nullptr;
    HostReport() {
        OF2D_HIP(hipHostMalloc(&p, sizeof(of2d::FluidReport),
                               hipHostMallocCoherent | hipHostMallocMapped));
        memset(p, 0xAB, sizeof(of2d::FluidReport));
    }
    ~HostReport() {
        if (p) (void)hipHostFree(p);
    }
    HostReport(const HostReport &) = delete;
    HostReport &operator=(const HostReport &) = delete;
};
}  // namespace

extern "C" {

int of2d_prim_sor_pack(const float *u, const float *dI, const float *It, const float *v0,
                       int elastic, int dimx, int dimy, unsigned epoch, float *v, float *b,
                       unsigned *gran) {
    if (!u || !dI || !It || !v || !b || !gran)
        return refuse(nullptr, "of2d_prim_sor_pack: u, dI, It, v, b or gran is NULL");
    if (elastic != 0 && elastic != 1) return refuse(nullptr, "of2d_prim_sor_pack: elastic is 0 or 1");
    if (!elastic && !v0)
        return refuse(nullptr, "of2d_prim_sor_pack: the force-only mode takes the prior v plane");
    if (dimx < 1 || dimy < 1) return refuse(nullptr, "of2d_prim_sor_pack: dimx, dimy < 1");
    return prim(true, [&] {
        SorLevel S(dimx, dimy, elastic ? 2 : 5);
        of2d::Field<float2> m, g;
        of2d::Field<float> t;
        upload(m, u, dimx, dimy);
        upload(g, dI, dimx, dimy);
        upload(t, It, dimx, dimy);
        S.put(elastic ? nullptr : v0, nullptr, 0u);  // stale granules: tag 0
        of2d::launch_sor_pack(S.L.vb.p, m.p, g.p, t.p, elastic ? m.p : nullptr, dimx, dimy,
                              S.L.P, S.L.sorH.p, epoch, nullptr);
        S.get(v, b, gran);
    });
}

int of2d_prim_regrid_pack(const float *Iref, const float *Iaux, const float *v0, int regridded,
                          int dimx, int dimy, unsigned epoch, float *dI, float *It, float *b,
                          unsigned *gran) {
    if (!Iref || !Iaux || !v0 || !dI || !It || !b || !gran)
        return refuse(nullptr, "of2d_prim_regrid_pack: Iref, Iaux, v0, dI, It, b or gran is NULL");
    if (regridded != 0 && regridded != 1)
        return refuse(nullptr, "of2d_prim_regrid_pack: regridded is 0 or 1");
    if (dimx < 2 || dimy < 2)
        return refuse(nullptr, "of2d_prim_regrid_pack: the gradients need dimx >= 2 and dimy >= 2");
    return prim(true, [&] {
        SorLevel S(dimx, dimy, 5);
        of2d::Field<float> ir, ia, t;
        of2d::Field<float2> g;
        upload(ir, Iref, dimx, dimy);
        upload(ia, Iaux, dimx, dimy);
        upload(g, dI, dimx, dimy);
        upload(t, It, dimx, dimy);
        S.put(v0, b, 0u, gran);
        S.control(0u, kNoStop, (unsigned)regridded, 0u);
        of2d::launch_regrid_pack(ir.p, ia.p, g.p, t.p, S.L.vb.p, dimx, dimy, S.L.P, S.L.sorH.p,
                                 epoch, nullptr, of2d::FluidCtl{S.st.w.p, 1});
        download(dI, g.p, g.P, dimx, dimy);
        download(It, t.p, t.P, dimx, dimy);
        S.get(nullptr, b, gran);
    });
}

int of2d_prim_sor_sweep(const float *v, const float *b, const float *u, int dimx, int dimy,
                        float mu, float lambda, float omega, int method, int nsweeps,
                        int zero_est, int skip_at, int poison, unsigned poison_word,
                        float *v_out, float *R, float *scal, float *part, int *path,
                        unsigned long long *words, unsigned *status) {
    if (!v || !b || !v_out || !words || !status || !path)
        return refuse(nullptr, "of2d_prim_sor_sweep: v, b, v_out, path, words or status is NULL");
    if (method != 0 && method != 1)
        return refuse(nullptr, "of2d_prim_sor_sweep: method is 0 (launch_sor) or 1 "
                               "(launch_sor_increment)");
    if (method == 1 && (!u || !R || !scal || !part))
        return refuse(nullptr, "of2d_prim_sor_sweep: method 1 takes u and returns R, scal, part");
    if (dimx < 1 || dimy < 1) return refuse(nullptr, "of2d_prim_sor_sweep: dimx, dimy < 1");
    if (nsweeps < 1) return refuse(nullptr, "of2d_prim_sor_sweep: nsweeps < 1");
    if (skip_at < -1 || skip_at >= nsweeps)
        return refuse(nullptr, "of2d_prim_sor_sweep: skip_at is -1 or a sweep of the call");
    return prim(true, [&] {
        SorLevel S(dimx, dimy, method ? 5 : 2);
        of2d::Level &L = S.L;
        of2d::Field<float2> m;
        of2d::DevArray<float> sc;
        sc.alloc(4);
        upload(m, method ? u : nullptr, dimx, dimy);
        if (poison) S.fill(poison_word);
        const unsigned ep0 = 1u;
        S.put(v, b, ep0);
        // the stop word of a loop that broke at iteration 0: sweep skip_at runs
        // as iteration 1, every other sweep as iteration 0
        S.control(0u, skip_at >= 0 ? 0u : kNoStop, zero_est ? 1u : 0u, 0u);
        *path = method ? (of2d::sor_increment_plan(dimx, dimy) > 0 ? 1 : 0) : 0;
        for (int s = 0; s < nsweeps; s++) {
            const of2d::FluidCtl c{S.st.w.p, s == skip_at ? 1 : 0};
            if (s) S.retag(ep0 + (unsigned)s);
            if (method)
                of2d::launch_sor_increment(L.vb.p, dimx, dimy, L.P, mu, lambda, omega, L.sorH.p,
                                           ep0 + (unsigned)s, L.sorTicket.p, L.sorCtr.p, m.p,
                                           L.increment.p, L.part.p, sc.p, S.st.w.p, nullptr, c);
            else
                of2d::launch_sor(L.vb.p, dimx, dimy, L.P, mu, lambda, omega, L.sorH.p,
                                 ep0 + (unsigned)s, L.sorTicket.p, S.st.w.p, nullptr, c);
        }
        S.get(v_out, nullptr, nullptr);
        unsigned w[4];
        S.st.get_control(w);
        *status = w[0];
        unsigned t = 0;
        fetch(&t, L.sorTicket.p, 1);
        words[0] = t;
        words[1] = words[2] = 0;
        if (method) {
            fetch(words + 1, L.sorCtr.p, 2);
            download(R, L.increment.p, L.increment.P, dimx, dimy);
            fetch(scal, sc.p, 2);
            fetch(part, L.part.p, (size_t)of2d::increment_nblocks(dimx, dimy));
        }
    });
}

int of2d_prim_fluid_increment(const float *u, const float *v, int dimx, int dimy, int zero_est,
                              float *R, float *scal, float *part) {
    if (!u || !v || !R || !scal || !part)
        return refuse(nullptr, "of2d_prim_fluid_increment: u, v, R, scal or part is NULL");
    if (dimx < 1 || dimy < 1) return refuse(nullptr, "of2d_prim_fluid_increment: dimx, dimy < 1");
    return prim(true, [&] {
        SorLevel S(dimx, dimy, 5);
        of2d::Level &L = S.L;
        of2d::Field<float2> m;
        of2d::DevArray<float> sc;
        sc.alloc(4);
        upload(m, u, dimx, dimy);
        S.put(v, nullptr, 0u);
        S.control(0u, kNoStop, zero_est ? 1u : 0u, 0u);
        of2d::launch_increment(m.p, L.vb.p, L.increment.p, dimx, dimy, L.P, L.part.p, sc.p,
                               nullptr, of2d::FluidCtl{S.st.w.p, 0});
        download(R, L.increment.p, L.increment.P, dimx, dimy);
        fetch(scal, sc.p, 2);
        fetch(part, L.part.p, (size_t)of2d::increment_nblocks(dimx, dimy));
    });
}

int of2d_prim_fluid_step(const float *u, const float *R, const float *prev, const float *dI,
                         const float *It, const float *v0, float dt, int zero_est, int dimx,
                         int dimy, unsigned epoch, float *uo, double *sums, float *jmin, float *b,
                         unsigned *gran) {
    if (!u || !R || !dI || !It || !v0 || !uo || !sums || !jmin || !b || !gran)
        return refuse(nullptr, "of2d_prim_fluid_step: an array other than prev is NULL");
    if (dimx < 1 || dimy < 1) return refuse(nullptr, "of2d_prim_fluid_step: dimx, dimy < 1");
    return prim(true, [&] {
        SorLevel S(dimx, dimy, 5);
        of2d::Level &L = S.L;
        of2d::Field<float2> m, r, o, pv, g;
        of2d::Field<float> t;
        upload(m, u, dimx, dimy);
        upload(r, R, dimx, dimy);
        upload(o, nullptr, dimx, dimy);
        if (prev) upload(pv, prev, dimx, dimy);
        upload(g, dI, dimx, dimy);
        upload(t, It, dimx, dimy);
        const int nb = of2d::increment_nblocks(dimx, dimy);
        of2d::DevArray<double> lpart;
        of2d::DevArray<float> sc;
        lpart.alloc(2 * (size_t)nb);
        sc.alloc(4);
        const float s[2] = {0.0f, dt};
        OF2D_HIP(hipMemcpy(sc.p, s, sizeof s, hipMemcpyHostToDevice));
        S.put(v0, nullptr, 0u);
        S.control(0u, kNoStop, zero_est ? 1u : 0u, 0u);
        HostReport rep;
        // the next sweep's epoch, as loop_fluid passes it
        of2d::launch_fluid_step(m.p, r.p, o.p, prev ? pv.p : nullptr, sc.p, g.p, t.p, L.vb.p,
                                dimx, dimy, L.P, L.sorH.p, epoch + 1, lpart.p, L.part.p, nullptr,
                                of2d::FluidCtl{S.st.w.p, 0});
        of2d::launch_fluid_report(lpart.p, nb, L.part.p, sc.p, S.st.w.p, rep.p, nullptr);
        download(uo, o.p, o.P, dimx, dimy);
        S.get(nullptr, b, gran);
        sums[0] = rep.p->sums[0];
        sums[1] = rep.p->sums[1];
        *jmin = rep.p->jmin;
    });
}

int of2d_prim_fluid_decide(const double *lpart, const float *jpart, int nb, const float *seq,
                           double npx, int fixed, int it, const float *scal, unsigned *words,
                           double *sums, float *repf, unsigned *repu) {
    if (!lpart || !jpart || !scal || !words || !sums || !repf || !repu)
        return refuse(nullptr, "of2d_prim_fluid_decide: an array other than seq is NULL");
    if (nb < 1) return refuse(nullptr, "of2d_prim_fluid_decide: nb < 1");
    if (!(npx >= 1.0)) return refuse(nullptr, "of2d_prim_fluid_decide: npx < 1");
    if (it < 0) return refuse(nullptr, "of2d_prim_fluid_decide: it < 0");
    return prim(true, [&] {
        StatusWord st;
        of2d::DevArray<double> lp;
        of2d::DevArray<float> jp, sq, sc;
        lp.alloc(2 * (size_t)nb);
        jp.alloc((size_t)nb);
        sq.alloc(2);
        sc.alloc(4);
        OF2D_HIP(hipMemcpy(lp.p, lpart, 2 * (size_t)nb * sizeof(double), hipMemcpyHostToDevice));
        OF2D_HIP(hipMemcpy(jp.p, jpart, (size_t)nb * sizeof(float), hipMemcpyHostToDevice));
        if (seq) OF2D_HIP(hipMemcpy(sq.p, seq, 2 * sizeof(float), hipMemcpyHostToDevice));
        const float s[3] = {scal[0], scal[1], repf[6]};  // scal[2]: the caller's marker
        OF2D_HIP(hipMemcpy(sc.p, s, sizeof s, hipMemcpyHostToDevice));
        st.put_control(words);
        HostReport rep;
        of2d::launch_fluid_report_decide(lp.p, nb, jp.p, sc.p, seq ? sq.p : nullptr, npx,
                                         fixed != 0, rep.p, nullptr, of2d::FluidCtl{st.w.p, it});
        st.get_control(words);
        const of2d::FluidReport &r = *rep.p;
        sums[0] = r.sums[0];
        sums[1] = r.sums[1];
        const float f[6] = {r.maxabs, r.dt, r.jmin, r.seq[0], r.seq[1], r.err};
        memcpy(repf, f, sizeof f);
        fetch(repf + 6, sc.p + 2, 1);
        repu[0] = r.status;
        repu[1] = r.flags;
    });
}

int of2d_prim_elastic_logger(const float *v, const float *prev, int dimx, int dimy, float *u,
                             float *prev_out, double *sums) {
    if (!v || !prev || !u || !prev_out || !sums)
        return refuse(nullptr, "of2d_prim_elastic_logger: v, prev, u, prev_out or sums is NULL");
    if (dimx < 1 || dimy < 1) return refuse(nullptr, "of2d_prim_elastic_logger: dimx, dimy < 1");
    return prim(true, [&] {
        SorLevel S(dimx, dimy, 2);
        of2d::Level &L = S.L;
        of2d::Field<float2> est, pv;
        upload(est, nullptr, dimx, dimy);
        upload(pv, prev, dimx, dimy);
        const int nb = of2d::increment_nblocks(dimx, dimy);
        of2d::DevArray<double> part, ds;
        part.alloc(2 * (size_t)nb);
        ds.alloc(2);
        S.put(v, nullptr, 0u);
        of2d::launch_logger(L.vb.p, est.p, pv.p, dimx, dimy, L.P, part.p, nullptr);
        of2d::launch_reduce_partials(part.p, nb, 1, ds.p, nullptr);
        download(u, est.p, est.P, dimx, dimy);
        download(prev_out, pv.p, pv.P, dimx, dimy);
        fetch(sums, ds.p, 2);
    });
}

}  // extern "C"

// ------------------------------------------------------------------ device-resident I/O kernels
namespace {
// dense host fields -> npairs pitched fields
template <class T>
void upload_pairs(of2d::batch::BField<T> &f, const float *host, int npairs, int dimx, int dimy) {
    f.alloc(dimx, dimy, npairs);
    const long stride = of2d::batch::pair_stride(dimx, dimy);
    const size_t per = (size_t)dimx * dimy * (sizeof(T) / sizeof(float));
    for (int k = 0; host && k < npairs; k++)
        upload(f.p + k * stride, of2d::pitch_for(dimx), host + k * per, dimx, dimy);
}
// the pack entries' target: npairs pitched fields with kPackSentinel in every
// byte, not the allocator's zeros, so that a stray store of 0 shows in `raw`
constexpr int kPackSentinel = 0xC5;  // as a float -6328.72: finite, unlikely
template <class T>
void sentinel_pairs(of2d::batch::BField<T> &f, int npairs, int dimx, int dimy) {
    f.alloc(dimx, dimy, npairs);
    OF2D_HIP(hipMemset(f.base, kPackSentinel, f.bytes()));
}
// the pixels of every pair, dense, into out_host; into raw_host (optional) the
// whole allocation from its base: ghost j-lines and slack too
template <class T>
void download_pairs(const of2d::batch::BField<T> &f, int npairs, int dimx, int dimy,
                    float *out_host, float *raw_host) {
    const long stride = of2d::batch::pair_stride(dimx, dimy);
    const size_t per = (size_t)dimx * dimy * (sizeof(T) / sizeof(float));
    for (int k = 0; k < npairs; k++)
        download(out_host + k * per, f.p + k * stride, of2d::pitch_for(dimx), dimx, dimy);
    if (raw_host) OF2D_HIP(hipMemcpy(raw_host, f.base, f.bytes(), hipMemcpyDeviceToHost));
}
bool pack_sizes_ok(int npairs, int dimx, int dimy) {
    return npairs > 0 && npairs <= of2d::batch::kMaxPairs && dimx > 0 && dimy > 0;
}
}  // namespace

extern "C" {

int of2d_prim_pack_layout(int dimx, int dimy, long long *stride, int *pitch) {
    if (!stride || !pitch || dimx < 1 || dimy < 1)
        return refuse(nullptr, "of2d_prim_pack_layout: stride or pitch is NULL, or a size < 1");
    *stride = of2d::batch::pair_stride(dimx, dimy);
    *pitch = of2d::pitch_for(dimx);
    return OF2D_OK;
}

int of2d_prim_pack_image(const of2d_darray *in, int npairs, int dimx, int dimy, float *out_host,
                         float *raw_host) {
    const Extents e = {{npairs, dimx, dimy, 0}};
    const bool ok = out_host && pack_sizes_ok(npairs, dimx, dimy);
    const std::string why =
        ok ? first_refusal("of2d_prim_pack_image", {{in, "in", false, e}})
           : std::string("of2d_prim_pack_image: out_host is NULL or a size is out of range");
    if (!why.empty()) return refuse(nullptr, why.c_str());
    return prim(true, [&] {
        of2d::batch::BField<float> f;
        sentinel_pairs(f, npairs, dimx, dimy);
        of2d::launch_pack_image(view_of(in, e), npairs, dimx, dimy, f.p,
                                of2d::batch::pair_stride(dimx, dimy), of2d::pitch_for(dimx),
                                nullptr);
        download_pairs(f, npairs, dimx, dimy, out_host, raw_host);
    });
}

int of2d_prim_unpack_image(const float *in_host, int npairs, int dimx, int dimy,
                           const of2d_darray *out) {
    const Extents e = {{npairs, dimx, dimy, 0}};
    const bool ok = in_host && npairs > 0 && npairs <= of2d::batch::kMaxPairs && dimx > 0 &&
                    dimy > 0;
    const std::string why =
        ok ? first_refusal("of2d_prim_unpack_image", {{out, "out", true, e}})
           : std::string("of2d_prim_unpack_image: in_host is NULL or a size is out of range");
    if (!why.empty()) return refuse(nullptr, why.c_str());
    return prim(true, [&] {
        of2d::batch::BField<float> f;
        upload_pairs(f, in_host, npairs, dimx, dimy);
        of2d::launch_unpack_image(f.p, of2d::batch::pair_stride(dimx, dimy),
                                  of2d::pitch_for(dimx), npairs, dimx, dimy, view_of(out, e),
                                  nullptr);
        OF2D_HIP(hipStreamSynchronize(nullptr));
    });
}

int of2d_prim_unpack_motion(const float *m_host, int npairs, int dimx, int dimy,
                            const of2d_darray *out) {
    const Extents e = {{npairs, dimx, dimy, 2}};
    const bool ok = m_host && npairs > 0 && npairs <= of2d::batch::kMaxPairs && dimx > 0 &&
                    dimy > 0;
    const std::string why =
        ok ? first_refusal("of2d_prim_unpack_motion", {{out, "out", true, e}})
           : std::string("of2d_prim_unpack_motion: m_host is NULL or a size is out of range");
    if (!why.empty()) return refuse(nullptr, why.c_str());
    return prim(true, [&] {
        of2d::batch::BField<float2> f;
        upload_pairs(f, m_host, npairs, dimx, dimy);
        of2d::launch_unpack_motion(f.p, of2d::batch::pair_stride(dimx, dimy),
                                   of2d::pitch_for(dimx), npairs, dimx, dimy, view_of(out, e),
                                   nullptr);
        OF2D_HIP(hipStreamSynchronize(nullptr));
    });
}

int of2d_prim_pack_motion(const of2d_darray *in, int npairs, int dimx, int dimy, float *out_host,
                          float *raw_host) {
    const Extents e = {{npairs, dimx, dimy, 2}};
    const bool ok = out_host && pack_sizes_ok(npairs, dimx, dimy);
    const std::string why =
        ok ? first_refusal("of2d_prim_pack_motion", {{in, "in", false, e}})
           : std::string("of2d_prim_pack_motion: out_host is NULL or a size is out of range");
    if (!why.empty()) return refuse(nullptr, why.c_str());
    return prim(true, [&] {
        int dev = 0;
        (void)hipGetDevice(&dev);  // without a device the pointer check below refuses
        of2d::check_device_pointer(in->ptr, dev, "of2d_prim_pack_motion: in");
        of2d::batch::BField<float2> f;
        sentinel_pairs(f, npairs, dimx, dimy);
        of2d::launch_pack_motion(view_of(in, e), npairs, dimx, dimy, f.p,
                                 of2d::batch::pair_stride(dimx, dimy), of2d::pitch_for(dimx),
                                 nullptr);
        download_pairs(f, npairs, dimx, dimy, out_host, raw_host);
    });
}

int of2d_prim_planar_to_motion(const double *planar_host, int npairs, int dimx, int dimy,
                               float *out_host, float *raw_host) {
    if (!planar_host || !out_host || !pack_sizes_ok(npairs, dimx, dimy))
        return refuse(nullptr, "of2d_prim_planar_to_motion: planar_host or out_host is NULL or a "
                               "size is out of range");
    return prim(true, [&] {
        const size_t n = 2 * (size_t)npairs * dimx * dimy;
        of2d::DevArray<double> in;
        in.alloc(n);
        OF2D_HIP(hipMemcpy(in.p, planar_host, n * sizeof(double), hipMemcpyHostToDevice));
        of2d::batch::BField<float2> f;
        sentinel_pairs(f, npairs, dimx, dimy);
        of2d::launch_planar_to_motion(in.p, npairs, dimx, dimy, f.p,
                                      of2d::batch::pair_stride(dimx, dimy),
                                      of2d::pitch_for(dimx), nullptr);
        download_pairs(f, npairs, dimx, dimy, out_host, raw_host);
    });
}

// ------------------------------------------------------------------ batched analysis kernels
int of2d_prim_batch_jacobian(const float *u, int B, int dimx, int dimy, float *jac,
                             double *stats) {
    if (!u || !stats) return refuse(nullptr, "of2d_prim_batch_jacobian: u or stats is NULL");
    if (B < 1 || B > of2d::batch::kMaxPairs)
        return refuse(nullptr, "of2d_prim_batch_jacobian: B outside [1, 65535]");
    if (const char *why = of2d::batch::jacobian_refusal(dimx, dimy)) return refuse(nullptr, why);
    return prim(true, [&] {
        of2d::batch::BField<float2> f;
        of2d::batch::BField<float> j;
        upload_pairs(f, u, B, dimx, dimy);
        if (jac) upload_pairs(j, nullptr, B, dimx, dimy);
        of2d::DevArray<double> ds;
        ds.alloc(5 * (size_t)B);
        const long stride = of2d::batch::pair_stride(dimx, dimy);
        const int P = of2d::pitch_for(dimx);
        of2d::batch::launch_batch_jacobian({f.p, stride, dimx, dimy, P, j.p, ds.p}, B, nullptr);
        for (int k = 0; jac && k < B; k++)
            download(jac + (size_t)k * dimx * dimy, j.p + k * stride, P, dimx, dimy);
        fetch(stats, ds.p, 5 * (size_t)B);
    });
}

int of2d_prim_batch_invert(const float *u, int B, int dimx, int dimy, int max_iter, double tol,
                           float *v, double *info, float *residuals) {
    if (!u || !v || !info) return refuse(nullptr, "of2d_prim_batch_invert: u, v or info is NULL");
    if (B < 1 || B > of2d::batch::kMaxPairs)
        return refuse(nullptr, "of2d_prim_batch_invert: B outside [1, 65535]");
    if (const char *why = of2d::batch::invert_refusal(dimx, dimy, max_iter, tol))
        return refuse(nullptr, why);
    return prim(true, [&] {
        of2d::batch::BField<float2> f, w;
        upload_pairs(f, u, B, dimx, dimy);
        upload_pairs(w, nullptr, B, dimx, dimy);
        of2d::DevArray<double> di;
        di.alloc(4 * (size_t)B);
        of2d::DevArray<float> dr;
        if (residuals) dr.alloc((size_t)B * max_iter);
        const long stride = of2d::batch::pair_stride(dimx, dimy);
        const int P = of2d::pitch_for(dimx);
        of2d::batch::launch_batch_invert(
            {f.p, w.p, stride, dimx, dimy, P, max_iter, (float)tol, di.p, dr.p}, B, nullptr);
        for (int k = 0; k < B; k++)
            download(v + (size_t)k * dimx * dimy * 2, w.p + k * stride, P, dimx, dimy);
        fetch(info, di.p, 4 * (size_t)B);
        if (residuals) fetch(residuals, dr.p, (size_t)B * max_iter);
    });
}

int of2d_prim_batch_similarity(const float *a, int shared_a, const float *b, int B, int dimx,
                               int dimy, double *out) {
    if (!a || !b || !out) return refuse(nullptr, "of2d_prim_batch_similarity: a, b or out is NULL");
    if (B < 1 || B > of2d::batch::kMaxPairs)
        return refuse(nullptr, "of2d_prim_batch_similarity: B outside [1, 65535]");
    if (dimx < 1 || dimy < 1) return refuse(nullptr, "similarity: empty image");
    return prim(true, [&] {
        of2d::batch::BField<float> x, y;
        upload_pairs(x, a, shared_a ? 1 : B, dimx, dimy);
        upload_pairs(y, b, B, dimx, dimy);
        of2d::DevArray<double> ds;
        ds.alloc(2 * (size_t)B);
        const long stride = of2d::batch::pair_stride(dimx, dimy);
        of2d::batch::launch_batch_similarity(
            {x.p, shared_a ? 0 : stride, y.p, stride, dimx, dimy, of2d::pitch_for(dimx), ds.p, 2},
            B, nullptr);
        fetch(out, ds.p, 2 * (size_t)B);
    });
}

}  // extern "C"
