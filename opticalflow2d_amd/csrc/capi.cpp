// capi.cpp — the extern "C" boundary of libof2d.so (include/of2d.h).
//
// Every entry point catches the C++ exceptions of the driver and turns them
// into a status code plus the reference's message, so nothing throws across
// the ABI.  The gateway reproduces mexFunction's five modes over the same
// process-global singleton (WrapperOpticalFlow2d.cpp:13-155).  The test and
// diagnostic entries (of2d_prims.h) are in capi_prims.cpp.
#include "../../include/of2d.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <string>

#include "capi_internal.h"
#include "of2d_batch.h"

using namespace of2d::capi;

struct of2d_ctx {
    std::unique_ptr<of2d::Registration> reg;
    std::string err;
};

namespace {
of2d_print_fn g_print = nullptr;
void *g_print_user = nullptr;
std::mutex g_print_mu;
thread_local std::string g_gateway_err;
}  // namespace

namespace of2d {
namespace capi {
void set_gateway_error(const std::string &msg) { g_gateway_err = msg; }
int refuse(of2d_ctx *ctx, const char *why) {
    g_gateway_err = why;
    if (ctx) ctx->err = why;
    return OF2D_ERR_INVALID_ARGUMENT;
}
}  // namespace capi


void print(const char *fmt, ...) {
    char buf[2048];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lk(g_print_mu);
    if (g_print)
        g_print(buf, g_print_user);
    else {
        fputs(buf, stdout);
        fflush(stdout);
    }
}
}  // namespace of2d

extern "C" {

void of2d_set_print_hook(of2d_print_fn fn, void *user) {
    std::lock_guard<std::mutex> lk(g_print_mu);
    g_print = fn;
    g_print_user = user;
}

const char *of2d_version(void) { return "opticalflow2d_amd 0.1 (gfx950)"; }

int of2d_device_count(int *count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (count) *count = (e == hipSuccess) ? n : 0;
    return e == hipSuccess ? OF2D_OK : OF2D_ERR_DEVICE;
}

int of2d_create(of2d_ctx **out, int dimx, int dimy, const int *niter, int nscales, int reg,
                const float *regparams, unsigned nparams, int nrefine, int verbose) {
    if (!out) return OF2D_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    auto *c = new of2d_ctx();
    std::string err;
    int rc = guarded(err, [&] {
        if (!niter) throw std::invalid_argument("niter is NULL");
        if (nparams > 0 && !regparams) throw std::invalid_argument("regparams is NULL");
        static const float zero = 0.0f;
        c->reg.reset(new of2d::Registration(dimx, dimy, nscales, niter, nrefine, reg,
                                            nparams ? regparams : &zero, nparams, verbose));
    });
    if (rc != OF2D_OK) {
        g_gateway_err = err;
        delete c;
        return rc;
    }
    *out = c;
    return OF2D_OK;
}

int of2d_set_images(of2d_ctx *ctx, const double *Iref, const double *Imov) {
    if (!ctx || !Iref || !Imov) return OF2D_ERR_INVALID_ARGUMENT;
    return guarded(ctx->err, [&] { ctx->reg->set_images(Iref, Imov); });
}

int of2d_estimate(of2d_ctx *ctx) {
    if (!ctx) return OF2D_ERR_INVALID_ARGUMENT;
    return guarded(ctx->err, [&] { ctx->reg->estimate(); });
}

int of2d_get_motion(of2d_ctx *ctx, double *out) {
    if (!ctx || !out) return OF2D_ERR_INVALID_ARGUMENT;
    return guarded(ctx->err, [&] { ctx->reg->get_motion(out); });
}

int of2d_set_motion(of2d_ctx *ctx, const double *motion) {
    if (!ctx) return refuse(nullptr, "of2d_set_motion: ctx is NULL");
    if (!motion) return refuse(ctx, "of2d_set_motion: motion is NULL");
    return guarded(ctx->err, [&] { ctx->reg->set_motion(motion); });
}

int of2d_reset_motion(of2d_ctx *ctx) {
    if (!ctx) return refuse(nullptr, "of2d_reset_motion: ctx is NULL");
    return guarded(ctx->err, [&] { ctx->reg->reset_motion(); });
}

int of2d_warp(of2d_ctx *ctx, const double *Imov, double *out) {
    if (!ctx || !Imov || !out) return OF2D_ERR_INVALID_ARGUMENT;
    return guarded(ctx->err, [&] { ctx->reg->warp(Imov, out); });
}

int of2d_destroy(of2d_ctx *ctx) {
    if (!ctx) return OF2D_ERR_INVALID_ARGUMENT;
    std::string err;
    int rc = guarded(err, [&] { ctx->reg.reset(); });
    delete ctx;
    return rc;
}

const char *of2d_last_error(const of2d_ctx *ctx) {
    return ctx ? ctx->err.c_str() : g_gateway_err.c_str();
}

int of2d_iterations_executed(const of2d_ctx *ctx, int *out, int cap) {
    if (!ctx) return -1;
    const auto &v = ctx->reg->iterations();
    for (int i = 0; i < (int)v.size() && i < cap; i++) out[i] = v[i];
    return (int)v.size();
}

int of2d_last_errors(const of2d_ctx *ctx, float *out, int cap) {
    if (!ctx) return -1;
    const auto &v = ctx->reg->last_errors();
    for (int i = 0; i < (int)v.size() && i < cap; i++) out[i] = v[i];
    return (int)v.size();
}

int of2d_set_option(of2d_ctx *ctx, const char *key, double value) {
    if (!ctx || !key) return OF2D_ERR_INVALID_ARGUMENT;
    return guarded(ctx->err, [&] { ctx->reg->set_option(key, value); });
}

int of2d_curvature_paths(const of2d_ctx *ctx, int *out, int cap) {
    if (!ctx) return -1;
    const auto &v = ctx->reg->curvature_paths();
    for (int i = 0; i < (int)v.size() && i < cap; i++) out[i] = v[i];
    return (int)v.size() / 4;
}

int of2d_demons_paths(const of2d_ctx *ctx, int *out, int cap) {
    if (!ctx) return -1;
    const auto &v = ctx->reg->demons_paths();
    for (int i = 0; i < (int)v.size() && i < cap; i++) out[i] = v[i];
    return (int)v.size() / 4;
}

static_assert(OF2D_SEP_KW_MAX == of2d::kSepKwMax,
              "include/of2d.h documents the separable smoothing's widths");
static_assert(OF2D_DCT_NMIN == of2d::kDctMinN && OF2D_DCT_NMAX == of2d::kDctMaxN,
              "include/of2d.h documents the fast transform's lengths");

// ------------------------------------------------------------------ analysis
}  // extern "C"

namespace {
// the analysis of a context's motion: its own error string, mirrored for
// of2d_gateway_last_error
template <class F>
int analysis(of2d_ctx *ctx, F &&f) {
    const int rc = guarded(ctx->err, f);
    if (rc != OF2D_OK) g_gateway_err = ctx->err;
    return rc;
}
const char *invert_args(int dimx, int dimy, int max_iter, double tol) {
    return of2d::batch::invert_refusal(dimx, dimy, max_iter, tol);  // batch_plan.h
}
}  // namespace

extern "C" {

static_assert(OF2D_INVERT_CHUNK == of2d::kInvertChunk,
              "include/of2d.h documents the inverse's chunk");

int of2d_field_jacobian(const float *u, int dimx, int dimy, float *jac, double *stats) {
    if (!u || !stats) return refuse(nullptr, "of2d_field_jacobian: u or stats is NULL");
    if (dimx < 2 || dimy < 2)
        return refuse(nullptr, "jacobian: the field needs dimx >= 2 and dimy >= 2");
    return prim(true, [&] {
        of2d::Field<float2> f;
        of2d::Field<float> j;
        upload(f, u, dimx, dimy);
        if (jac) upload(j, nullptr, dimx, dimy);
        of2d::DevArray<of2d::JacPartial> part;
        part.alloc((size_t)of2d::jacobian_nblocks(dimx, dimy));
        of2d::DevArray<double> ds;
        ds.alloc(5);
        of2d::launch_jacobian(f.p, dimx, dimy, f.P, j.p, part.p, ds.p, nullptr);
        if (jac) download(jac, j.p, j.P, dimx, dimy);
        fetch(stats, ds.p, 5);
    });
}

int of2d_jacobian(of2d_ctx *ctx, double *jac, double *stats) {
    if (!ctx || !stats) return refuse(ctx, "of2d_jacobian: ctx or stats is NULL");
    if (ctx->reg->dimx() < 2 || ctx->reg->dimy() < 2)
        return refuse(ctx, "jacobian: the field needs dimx >= 2 and dimy >= 2");
    return analysis(ctx, [&] { ctx->reg->jacobian(jac, stats); });
}

int of2d_field_invert(const float *u, int dimx, int dimy, int max_iter, double tol, float *v,
                      double *info, float *residuals) {
    if (!u || !v || !info) return refuse(nullptr, "of2d_field_invert: u, v or info is NULL");
    if (const char *why = invert_args(dimx, dimy, max_iter, tol)) return refuse(nullptr, why);
    return prim(true, [&] {
        of2d::Field<float2> f, v0, v1;
        upload(f, u, dimx, dimy);
        upload(v0, nullptr, dimx, dimy);
        upload(v1, nullptr, dimx, dimy);
        of2d::DevArray<unsigned> ctl;
        ctl.alloc(of2d::invert_ctl_words(max_iter));
        const of2d::InvertResult r = of2d::invert_field(f.p, v0.p, v1.p, dimx, dimy, f.P,
                                                        max_iter, (float)tol, ctl.p, residuals,
                                                        nullptr);
        download(v, r.v, f.P, dimx, dimy);
        info[0] = r.iterations;
        info[1] = (double)r.residual;
        info[2] = (double)r.oob;
        info[3] = r.converged ? 1.0 : 0.0;
    });
}

int of2d_invert_motion(of2d_ctx *ctx, int max_iter, double tol, double *out, double *info) {
    if (!ctx || !out || !info) return refuse(ctx, "of2d_invert_motion: ctx, out or info is NULL");
    if (const char *why = invert_args(ctx->reg->dimx(), ctx->reg->dimy(), max_iter, tol))
        return refuse(ctx, why);
    return analysis(ctx, [&] { ctx->reg->invert_motion(max_iter, tol, out, info); });
}

int of2d_image_similarity(const float *a, const float *b, int dimx, int dimy, double *out) {
    if (!a || !b || !out) return refuse(nullptr, "of2d_image_similarity: a, b or out is NULL");
    if (dimx < 1 || dimy < 1) return refuse(nullptr, "similarity: empty image");
    return prim(true, [&] {
        of2d::Field<float> x, y;
        upload(x, a, dimx, dimy);
        upload(y, b, dimx, dimy);
        of2d::DevArray<of2d::SimPartial> part;
        part.alloc((size_t)of2d::similarity_nblocks(dimx, dimy));
        of2d::DevArray<double> ds;
        ds.alloc(2);
        of2d::launch_similarity(x.p, y.p, dimx, dimy, x.P, part.p, ds.p, nullptr);
        fetch(out, ds.p, 2);
    });
}

int of2d_quality(of2d_ctx *ctx, const double *Iref, const double *Imov, double *out) {
    if (!ctx || !Iref || !Imov || !out)
        return refuse(ctx, "of2d_quality: ctx, Iref, Imov or out is NULL");
    return analysis(ctx, [&] { ctx->reg->quality(Iref, Imov, out); });
}

// ------------------------------------------------------------------ gateway
// static ImageRegistration *myImageRegistration (WrapperOpticalFlow2d.cpp:13)
static of2d_ctx *g_single = nullptr;
static int g_dimx = 0, g_dimy = 0;

size_t of2d_gateway_output_numel(int nlhs, int nrhs) {
    if (!g_single || nlhs != 1) return 0;
    if (nrhs == 0) return (size_t)g_dimx * g_dimy * 2;
    if (nrhs == 1) return (size_t)g_dimx * g_dimy;
    return 0;
}

int of2d_gateway_output_dims(int nlhs, int nrhs, size_t *dims, int *ndims) {
    if (!g_single || nlhs != 1 || (nrhs != 0 && nrhs != 1)) {
        if (ndims) *ndims = 0;
        return OF2D_ERR_STATE;
    }
    dims[0] = (size_t)g_dimx;  // dim_motion_mw / dim_image_mw (:74-78)
    dims[1] = (size_t)g_dimy;
    if (nrhs == 0) {
        dims[2] = 2;
        *ndims = 3;
    } else {
        *ndims = 2;
    }
    return OF2D_OK;
}

const char *of2d_gateway_last_error(void) { return g_gateway_err.c_str(); }

int of2d_gateway(int nlhs, double **plhs, int nrhs, const double *const *prhs) {
    // init (:23-83); a ninth input (this library's, not the reference's) is
    // the number of devices HS runs on (of2d_set_option "ngpus")
    if (nlhs == 0 && (nrhs == 8 || nrhs == 9) && g_single == nullptr) {
        const int dimx = (int)prhs[0][0], dimy = (int)prhs[0][1];
        const int nscales = (int)prhs[2][0];
        if (nscales < 0) {
            g_gateway_err = "Error: invalid number of scales\n";
            return OF2D_ERR_INVALID_ARGUMENT;
        }
        std::vector<int> niter(nscales + 1);
        for (int s = 0; s < nscales + 1; s++) niter[s] = (int)prhs[1][s];
        const int reg = (int)prhs[3][0];
        const unsigned nparams = (unsigned)prhs[5][0];
        std::vector<float> rp(nparams ? nparams : 1, 0.0f);
        for (unsigned p = 0; p < nparams; p++) rp[p] = (float)prhs[4][p];
        const int nrefine = (int)prhs[6][0];
        const int verbose = (int)prhs[7][0];
        of2d_ctx *c = nullptr;
        int rc = of2d_create(&c, dimx, dimy, niter.data(), nscales, reg, rp.data(), nparams,
                             nrefine, verbose);
        if (rc != OF2D_OK) return rc;  // message already in g_gateway_err
        if (nrhs == 9) {
            rc = of2d_set_option(c, "ngpus", prhs[8][0]);
            if (rc != OF2D_OK) {
                g_gateway_err = c->err;
                of2d_destroy(c);
                return rc;
            }
        }
        g_single = c;
        g_dimx = dimx;
        g_dimy = dimy;
        g_gateway_err.clear();
        return OF2D_OK;
    }
    // register (:86-102)
    if (nlhs == 0 && nrhs == 2 && g_single != nullptr) {
        int rc = of2d_set_images(g_single, prhs[0], prhs[1]);
        if (rc == OF2D_OK) rc = of2d_estimate(g_single);
        g_gateway_err = g_single->err;
        return rc;
    }
    // get motion (:105-117)
    if (nlhs == 1 && nrhs == 0 && g_single != nullptr) {
        int rc = of2d_get_motion(g_single, plhs[0]);
        g_gateway_err = g_single->err;
        return rc;
    }
    // warp (:120-137)
    if (nlhs == 1 && nrhs == 1 && g_single != nullptr) {
        int rc = of2d_warp(g_single, prhs[0], plhs[0]);
        g_gateway_err = g_single->err;
        return rc;
    }
    // close (:140-147)
    if (nlhs == 0 && nrhs == 0 && g_single != nullptr) {
        int rc = of2d_destroy(g_single);
        g_single = nullptr;
        g_dimx = g_dimy = 0;
        return rc;
    }
    g_gateway_err = "Error: invalid number of input and output variables gives.\n";
    return OF2D_ERR_STATE;
}

}  // extern "C"

// ------------------------------------------------------------------ batched Horn-Schunck
struct of2d_batch {
    std::unique_ptr<of2d::batch::Batch> b;
    std::string err;
};

static_assert(OF2D_BATCH_MAXPX == of2d::batch::kMaxPx, "include/of2d.h documents the batch's size");

extern "C" {

int of2d_batch_create(of2d_batch **out, int nbatch, int dimx, int dimy, const int *niter,
                      int nscales, int reg, const float *regparams, unsigned nparams,
                      int nrefine) {
    if (!out) return refuse(nullptr, "of2d_batch_create: out is NULL");
    *out = nullptr;
    auto *c = new of2d_batch();
    std::string err;
    const int rc = guarded(err, [&] {
        c->b.reset(new of2d::batch::Batch(nbatch, dimx, dimy, niter, nscales, reg, regparams,
                                          nparams, nrefine));
    });
    if (rc != OF2D_OK) {
        g_gateway_err = err;
        delete c;
        return rc;
    }
    *out = c;
    return OF2D_OK;
}

int of2d_batch_set_option(of2d_batch *b, const char *key, double value) {
    if (!b || !key) return refuse(nullptr, "of2d_batch_set_option: b or key is NULL");
    return guarded(b->err, [&] { b->b->set_option(key, value); });
}

int of2d_batch_set_images(of2d_batch *b, const double *Iref, int shared_ref, const double *Imov) {
    if (!b) return refuse(nullptr, "of2d_batch_set_images: b is NULL");
    if (!Iref || !Imov) {
        b->err = "of2d_batch_set_images: Iref or Imov is NULL";
        return OF2D_ERR_INVALID_ARGUMENT;
    }
    return guarded(b->err, [&] { b->b->set_images(Iref, shared_ref != 0, Imov); });
}

int of2d_batch_estimate(of2d_batch *b) {
    if (!b) return refuse(nullptr, "of2d_batch_estimate: b is NULL");
    return guarded(b->err, [&] { b->b->estimate(); });
}

int of2d_batch_get_motion(of2d_batch *b, double *out) {
    if (!b) return refuse(nullptr, "of2d_batch_get_motion: b is NULL");
    if (!out) {
        b->err = "of2d_batch_get_motion: out is NULL";
        return OF2D_ERR_INVALID_ARGUMENT;
    }
    return guarded(b->err, [&] { b->b->get_motion(out); });
}

int of2d_batch_set_motion(of2d_batch *b, const double *motion) {
    if (!b) return refuse(nullptr, "of2d_batch_set_motion: b is NULL");
    if (!motion) {
        b->err = "of2d_batch_set_motion: motion is NULL";
        return OF2D_ERR_INVALID_ARGUMENT;
    }
    return guarded(b->err, [&] { b->b->set_motion(motion); });
}

int of2d_batch_reset_motion(of2d_batch *b) {
    if (!b) return refuse(nullptr, "of2d_batch_reset_motion: b is NULL");
    return guarded(b->err, [&] { b->b->reset_motion(); });
}

int of2d_batch_warp(of2d_batch *b, const double *Imov, double *out) {
    if (!b) return refuse(nullptr, "of2d_batch_warp: b is NULL");
    if (!Imov || !out) {
        b->err = "of2d_batch_warp: Imov or out is NULL";
        return OF2D_ERR_INVALID_ARGUMENT;
    }
    return guarded(b->err, [&] { b->b->warp(Imov, out); });
}

int of2d_batch_status(const of2d_batch *b, int *out) {
    if (!b || !out) return OF2D_ERR_INVALID_ARGUMENT;
    const auto &s = b->b->status();
    for (size_t k = 0; k < s.size(); k++)
        out[k] = (s[k] & of2d::kStatusDivZero) ? OF2D_ERR_RUNTIME : OF2D_OK;
    return OF2D_OK;
}

int of2d_batch_iterations(const of2d_batch *b, int *out, int cap) {
    if (!b) return -1;
    const auto &v = b->b->iterations();
    for (int i = 0; i < (int)v.size() && i < cap; i++) out[i] = v[i];
    return (int)v.size();
}

int of2d_batch_last_errors(const of2d_batch *b, int pair, float *out, int cap) {
    if (!b || pair < 0 || pair >= b->b->nbatch()) return -1;
    const std::vector<float> v = b->b->last_errors(pair);
    for (int i = 0; i < (int)v.size() && i < cap; i++) out[i] = v[i];
    return (int)v.size();
}

int of2d_batch_fluid_log(const of2d_batch *b, int pair, int loop, float *out, int cap) {
    if (!b || pair < 0 || pair >= b->b->nbatch() || loop < 0 || loop >= b->b->nloops()) return -1;
    const std::vector<float> v = b->b->fluid_log(pair, loop);
    constexpr int R = of2d::batch::kFluidLogFloats;
    const int n = (int)v.size() / R;
    for (int i = 0; i < n && i < cap; i++)
        for (int q = 0; q < R; q++) out[R * i + q] = v[R * i + q];
    return n;
}

int of2d_batch_info(const of2d_batch *b, int *info, int n) {
    if (!b) return -1;
    const std::vector<int> v = b->b->info();
    for (int i = 0; i < (int)v.size() && i < n; i++) info[i] = v[i];
    return (int)v.size();
}

int of2d_batch_destroy(of2d_batch *b) {
    if (!b) return OF2D_ERR_INVALID_ARGUMENT;
    std::string err;
    const int rc = guarded(err, [&] {
        of2d::DeviceScope scope;
        b->b.reset();
    });
    delete b;
    return rc;
}

const char *of2d_batch_last_error(const of2d_batch *b) {
    if (!b) return g_gateway_err.c_str();
    return b->err.empty() ? b->b->pair_error().c_str() : b->err.c_str();
}

}  // extern "C"

// ------------------------------------------------------------------ device-resident I/O
namespace {
// "" or why the array is refused; no device work.  Unused axes' strides are
// not looked at.
std::string darray_refusal(const of2d_darray *a, const char *name, bool output, const Extents &e) {
    const std::string n(name);
    if (!a) return n + " is NULL";
    if (!a->ptr) return n + ".ptr is NULL";
    if (a->dtype != OF2D_F32 && a->dtype != OF2D_F64)
        return n + ".dtype is neither OF2D_F32 nor OF2D_F64";
    for (int k = 0; k < 4; k++) {
        if (e.n[k] <= 0) continue;
        if (a->stride[k] < 0) return n + " has a negative stride";
        if (output && a->stride[k] == 0 && e.n[k] > 1)
            return n + " has a zero stride on an axis of extent > 1";
    }
    return "";
}
}  // namespace

of2d::DArrayView of2d::capi::view_of(const of2d_darray *a, const Extents &e) {
    of2d::DArrayView v;
    v.ptr = a->ptr;
    v.f64 = a->dtype == OF2D_F64;
    v.sp = e.n[0] > 0 ? a->stride[0] : 0;
    v.sx = a->stride[1];
    v.sy = a->stride[2];
    v.sc = e.n[3] > 0 ? a->stride[3] : 0;
    return v;
}
std::string of2d::capi::first_refusal(const char *fn, std::initializer_list<DArrayArg> args) {
    for (const DArrayArg &g : args) {
        const std::string why = darray_refusal(g.a, g.name, g.output, g.e);
        if (!why.empty()) return std::string(fn) + ": " + why;
    }
    return "";
}

namespace {
template <class F>
int device_io(of2d_ctx *ctx, const char *fn, std::initializer_list<DArrayArg> args, F &&f) {
    if (!ctx) return refuse(nullptr, (std::string(fn) + ": ctx is NULL").c_str());
    const std::string why = first_refusal(fn, args);
    if (!why.empty()) return refuse(ctx, why.c_str());
    return guarded(ctx->err, f);
}
template <class F>
int device_io(of2d_batch *b, const char *fn, std::initializer_list<DArrayArg> args, F &&f) {
    if (!b) return refuse(nullptr, (std::string(fn) + ": b is NULL").c_str());
    const std::string why = first_refusal(fn, args);
    if (!why.empty()) {
        b->err = why;
        return OF2D_ERR_INVALID_ARGUMENT;
    }
    return guarded(b->err, f);
}
}  // namespace

extern "C" {

int of2d_set_images_device(of2d_ctx *ctx, const of2d_darray *Iref, const of2d_darray *Imov,
                           void *stream) {
    const Extents e = {{0, ctx ? ctx->reg->dimx() : 0, ctx ? ctx->reg->dimy() : 0, 0}};
    return device_io(ctx, "of2d_set_images_device", {{Iref, "Iref", false, e}, {Imov, "Imov", false, e}},
                     [&] {
                         ctx->reg->set_images_device(view_of(Iref, e), view_of(Imov, e),
                                                     static_cast<hipStream_t>(stream));
                     });
}

int of2d_get_motion_device(of2d_ctx *ctx, const of2d_darray *out, void *stream) {
    const Extents e = {{0, ctx ? ctx->reg->dimx() : 0, ctx ? ctx->reg->dimy() : 0, 2}};
    return device_io(ctx, "of2d_get_motion_device", {{out, "out", true, e}}, [&] {
        ctx->reg->get_motion_device(view_of(out, e), static_cast<hipStream_t>(stream));
    });
}

int of2d_set_motion_device(of2d_ctx *ctx, const of2d_darray *motion, void *stream) {
    const Extents e = {{0, ctx ? ctx->reg->dimx() : 0, ctx ? ctx->reg->dimy() : 0, 2}};
    return device_io(ctx, "of2d_set_motion_device", {{motion, "motion", false, e}}, [&] {
        ctx->reg->set_motion_device(view_of(motion, e), static_cast<hipStream_t>(stream));
    });
}

int of2d_batch_set_motion_device(of2d_batch *b, const of2d_darray *motion, void *stream) {
    const Extents e = {{b ? b->b->nbatch() : 0, b ? b->b->dimx() : 0, b ? b->b->dimy() : 0, 2}};
    return device_io(b, "of2d_batch_set_motion_device", {{motion, "motion", false, e}}, [&] {
        b->b->set_motion_device(view_of(motion, e), static_cast<hipStream_t>(stream));
    });
}

int of2d_warp_device(of2d_ctx *ctx, const of2d_darray *Imov, const of2d_darray *out,
                     void *stream) {
    const Extents e = {{0, ctx ? ctx->reg->dimx() : 0, ctx ? ctx->reg->dimy() : 0, 0}};
    return device_io(ctx, "of2d_warp_device", {{Imov, "Imov", false, e}, {out, "out", true, e}},
                     [&] {
                         ctx->reg->warp_device(view_of(Imov, e), view_of(out, e),
                                               static_cast<hipStream_t>(stream));
                     });
}

int of2d_batch_set_images_device(of2d_batch *b, const of2d_darray *Iref, int shared_ref,
                                 const of2d_darray *Imov, void *stream) {
    const int dx = b ? b->b->dimx() : 0, dy = b ? b->b->dimy() : 0, nb = b ? b->b->nbatch() : 0;
    const Extents er = {{shared_ref ? 0 : nb, dx, dy, 0}}, em = {{nb, dx, dy, 0}};
    return device_io(b, "of2d_batch_set_images_device",
                     {{Iref, "Iref", false, er}, {Imov, "Imov", false, em}}, [&] {
                         b->b->set_images_device(view_of(Iref, er), shared_ref != 0,
                                                 view_of(Imov, em),
                                                 static_cast<hipStream_t>(stream));
                     });
}

int of2d_batch_get_motion_device(of2d_batch *b, const of2d_darray *out, void *stream) {
    const Extents e = {{b ? b->b->nbatch() : 0, b ? b->b->dimx() : 0, b ? b->b->dimy() : 0, 2}};
    return device_io(b, "of2d_batch_get_motion_device", {{out, "out", true, e}}, [&] {
        b->b->get_motion_device(view_of(out, e), static_cast<hipStream_t>(stream));
    });
}

int of2d_batch_warp_device(of2d_batch *b, const of2d_darray *Imov, const of2d_darray *out,
                           void *stream) {
    const Extents e = {{b ? b->b->nbatch() : 0, b ? b->b->dimx() : 0, b ? b->b->dimy() : 0, 0}};
    return device_io(b, "of2d_batch_warp_device",
                     {{Imov, "Imov", false, e}, {out, "out", true, e}}, [&] {
                         b->b->warp_device(view_of(Imov, e), view_of(out, e),
                                           static_cast<hipStream_t>(stream));
                     });
}

}  // extern "C"

// ------------------------------------------------------------------ batched analysis
namespace {
// a refusal of a batch entry before any device work
int refuse_batch(of2d_batch *b, const std::string &why) {
    b->err = why;
    return OF2D_ERR_INVALID_ARGUMENT;
}
}  // namespace

extern "C" {

int of2d_batch_jacobian(of2d_batch *b, double *jac, double *stats) {
    if (!b) return refuse(nullptr, "of2d_batch_jacobian: b is NULL");
    if (!stats) return refuse_batch(b, "of2d_batch_jacobian: stats is NULL");
    return guarded(b->err, [&] { b->b->jacobian(jac, stats); });
}

int of2d_batch_invert_motion(of2d_batch *b, int max_iter, double tol, double *out, double *info) {
    if (!b) return refuse(nullptr, "of2d_batch_invert_motion: b is NULL");
    if (!info) return refuse_batch(b, "of2d_batch_invert_motion: info is NULL");
    return guarded(b->err, [&] { b->b->invert_motion(max_iter, tol, out, info); });
}

int of2d_batch_quality(of2d_batch *b, const double *Iref, int shared_ref, const double *Imov,
                       double *out) {
    if (!b) return refuse(nullptr, "of2d_batch_quality: b is NULL");
    if (!Iref || !Imov || !out)
        return refuse_batch(b, "of2d_batch_quality: Iref, Imov or out is NULL");
    return guarded(b->err, [&] { b->b->quality(Iref, shared_ref != 0, Imov, out); });
}

int of2d_batch_jacobian_device(of2d_batch *b, const of2d_darray *jac, double *stats,
                               void *stream) {
    if (!b) return refuse(nullptr, "of2d_batch_jacobian_device: b is NULL");
    if (!stats) return refuse_batch(b, "of2d_batch_jacobian_device: stats is NULL");
    const Extents e = {{b->b->nbatch(), b->b->dimx(), b->b->dimy(), 0}};
    auto run = [&] {
        of2d::DArrayView v;
        if (jac) v = view_of(jac, e);
        b->b->jacobian_device(jac ? &v : nullptr, stats, static_cast<hipStream_t>(stream));
    };
    if (!jac) return guarded(b->err, run);
    return device_io(b, "of2d_batch_jacobian_device", {{jac, "jac", true, e}}, run);
}

int of2d_batch_invert_motion_device(of2d_batch *b, int max_iter, double tol,
                                    const of2d_darray *out, double *info, void *stream) {
    if (!b) return refuse(nullptr, "of2d_batch_invert_motion_device: b is NULL");
    if (!info) return refuse_batch(b, "of2d_batch_invert_motion_device: info is NULL");
    const Extents e = {{b->b->nbatch(), b->b->dimx(), b->b->dimy(), 2}};
    return device_io(b, "of2d_batch_invert_motion_device", {{out, "out", true, e}}, [&] {
        b->b->invert_motion_device(max_iter, tol, view_of(out, e), info,
                                   static_cast<hipStream_t>(stream));
    });
}

int of2d_batch_quality_device(of2d_batch *b, const of2d_darray *Iref, int shared_ref,
                              const of2d_darray *Imov, double *out, void *stream) {
    if (!b) return refuse(nullptr, "of2d_batch_quality_device: b is NULL");
    if (!out) return refuse_batch(b, "of2d_batch_quality_device: out is NULL");
    const int dx = b->b->dimx(), dy = b->b->dimy(), nb = b->b->nbatch();
    const Extents er = {{shared_ref ? 0 : nb, dx, dy, 0}}, em = {{nb, dx, dy, 0}};
    return device_io(b, "of2d_batch_quality_device",
                     {{Iref, "Iref", false, er}, {Imov, "Imov", false, em}}, [&] {
                         b->b->quality_device(view_of(Iref, er), shared_ref != 0,
                                              view_of(Imov, em), out,
                                              static_cast<hipStream_t>(stream));
                     });
}

}  // extern "C"
