// batch.cpp — host driver of the batched Horn-Schunck, Curvature, Elastic, Fluid and
// Thirion's Demons registrations (of2d_batch.h).  The pyramid and refine sequence is that
// of Registration::estimate / estimate_level for Diffusion, Curvature, Elastic and
// Thirion's Demons (registration.cpp; Demons takes no gradients pass: its loop warps and
// differentiates the moving image itself),
// applied to all pairs at once: the host enqueues every level's launches and
// reads nothing back until the estimate ends; every decision (a pair's break,
// its divide-by-zero) is taken in the kernels.  The number of launches does
// not depend on the number of pairs.
#include "of2d_batch.h"

#include <algorithm>
#include <cmath>

#include "of2d_host.h"

namespace of2d {
namespace batch {

Batch::Batch(int nbatch, int dimx, int dimy, const int *niter, int nscales, int reg,
             const float *params, unsigned nparams, int nrefine)
    : B_(nbatch), dimx_(dimx), dimy_(dimy), nscales_(nscales), nrefine_(nrefine), reg_(reg) {
    if (nbatch < 1) throw std::invalid_argument("Error: batch needs nbatch >= 1\n");
    if (nbatch > kMaxPairs)
        throw std::invalid_argument("Error: batch takes at most 65535 pairs per call\n");
    // one sentence for every refusal by method; a Curvature batch whose levels
    // do not all qualify gets it too (below), and Elastic without its omega:
    // the reference's two-parameter form (omega = 0.66f) is the caller's to
    // spell out (include/of2d.h)
    static const char *const kMethods =
        "Error: the batched registration supports Diffusion regularisation only, Thirion's "
        "Demons, Curvature where every level's sides are powers of two from 8 to 512, or "
        "Elastic with its three parameters [mu, lambda, omega] (Fluid is the option \"fluid\" of "
        "such an Elastic batch)\n";
    if (reg != 0 && reg != 1 && reg != 2 && reg != 3) throw std::invalid_argument(kMethods);
    if (reg == 2 && nparams != 3) throw std::invalid_argument(kMethods);
    if (!valid_regularisation_parameters(reg, nparams))
        throw std::invalid_argument(
            "Invalid number of regularisation parameters for given regularisation method.\n");
    if (!niter) throw std::invalid_argument("niter is NULL");
    if (!params) throw std::invalid_argument("regparams is NULL");
    if (dimx <= 0 || dimy <= 0 || nscales < 0)
        throw std::invalid_argument("Error: invalid image dimensions\n");
    if (nscales > 30) throw std::invalid_argument("Error: pyramid level with zero size\n");
    if ((long)dimx * dimy > kMaxPx)
        throw std::invalid_argument(
            "Error: batch images may have at most 512 * 512 pixels (OF2D_BATCH_MAXPX)\n");
    niter_.assign(niter, niter + nscales + 1);
    params_.assign(params, params + nparams);
    if (reg == 3) {  // Demons.cpp:19-23, as Registration::Registration
        const int kw = (int)(unsigned)params[4];
        if (kw < 1) throw std::invalid_argument("Error: Demons kernel width must be >= 1\n");
        kdiff_ = gaussian_kernel(kw, params[2]);
        kfluid_ = gaussian_kernel(kw, params[3]);
    } else if (reg == 2) {
        sor_ = sor_coef(params[0], params[1], params[2]);
    } else {
        alpha_ = params[0];
        if (reg == 1 && nparams == 2) tau_ = params[1];  // else OpticalFlowCurvature.h:8
    }
    // ImageRegistration.cpp:56-61: dim(dimin.x/scale, dimin.y/scale) with float scale
    ldx_.resize(nscales + 1);
    ldy_.resize(nscales + 1);
    for (int s = nscales; s >= 0; s--) {
        const float scale = (float)std::pow(2, s);
        ldx_[s] = (int)(unsigned)((float)(unsigned)dimx / scale);
        ldy_[s] = (int)(unsigned)((float)(unsigned)dimy / scale);
        if (ldx_[s] <= 0 || ldy_[s] <= 0)
            throw std::invalid_argument("Error: pyramid level with zero size\n");
        // Curvature runs the fast line transforms on both axes of every level
        if (reg == 1 && !curv_level_ok(ldx_[s], ldy_[s])) throw std::invalid_argument(kMethods);
    }
    nloops_ = (nscales + 1) * std::max(nrefine, 0);
    for (int n : niter_) maxn_ = std::max(maxn_, n);
    h_status_.assign(B_, 0u);
    h_iters_.assign((size_t)B_ * nloops_, 0);
}

Batch::~Batch() { release_device(); }

// every owner lets go (the levels' fields with lv_), then the events and the stream
void Batch::release_device() {
    lv_.clear();
    qref_.release();
    d_stage_.release();
    d_words_.release();
    d_status_.release();
    d_iters_.release();
    d_errs_.release();
    d_flog_.release();
    d_kf_.release();
    d_kd_.release();
    for (hipEvent_t e : ev_)
        if (e) (void)hipEventDestroy(e);
    ev_.clear();
    for (hipEvent_t &e : ev_io_) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    if (st_) (void)hipStreamDestroy(st_);
    st_ = nullptr;
    ref_pairs_ = qref_pairs_ = 0;
    on_cu_ok_ = -1;
    ready_ = false;
}

// the value of a 0/1 option
static bool flag_value(const std::string &key, double v) {
    if (!(v == 0 || v == 1))  // a NaN too
        throw std::invalid_argument(key + ": the value must be 0 or 1");
    return v == 1;
}

// The 0/1 options are taken by the next estimate; a refusal changes nothing
void Batch::set_option(const std::string &key, double v) {
    if (key == "fixed_iters")
        fixed_ = v != 0;
    else if (key == "device") {
        if (ready_) throw std::invalid_argument("option 'device' must be set before first use");
        device_ = (int)v;
    } else if (key == "diffeomorphic") {
        // DemonsDiffeomorphic::get_update is DemonsThirions' with Composition
        // plus exp(): an option of such a batch
        if (kind() != LoopKind::Demons)
            throw std::invalid_argument("diffeomorphic: the batch is not a Thirion's Demons batch");
        if ((int)params_[5] != 0)
            throw std::invalid_argument("diffeomorphic: accumulation must be Composition (0)");
        diffeo_ = flag_value(key, v);
    } else if (key == "warm_start") {
        warm_ = flag_value(key, v);
    } else if (key == "fluid") {
        // OpticalFlowFluid takes Elastic's parameters and relaxes its velocity
        // with Elastic's sweep: an option of such a batch
        if (!loop_sweeps(kind()))
            throw std::invalid_argument("fluid: the batch is not an Elastic batch");
        const bool on = flag_value(key, v);
        // the Jacobian's one-sided differences need a neighbour
        for (int s = 0; on && s <= nscales_; s++)
            if (ldx_[s] < 2 || ldy_[s] < 2)
                throw std::invalid_argument("fluid: every level needs sides of at least 2");
        // a change of the value: the next estimate with it starts from a zero
        // velocity
        if (on != fluid_ && ready_ && have_velocity()) {
            DeviceScope scope;
            OF2D_HIP(hipSetDevice(home_));
            zero_velocity();
            OF2D_HIP(hipStreamSynchronize(st_));
        }
        if (on != fluid_) h_flog_.clear();  // the log is the option's
        fluid_ = on;
    } else if (key == "resident" || key == "conv_lds") {
        // the Horn-Schunck loop with the iterate on the CU, the Demons loop
        // with the convolved field in LDS, at the levels that fit (on_cu_fits)
        const char *own = on_cu_option(kind());
        if (!own || key != own)
            throw std::invalid_argument(key == "resident"
                                            ? "resident: the batch is not a Diffusion batch"
                                            : "conv_lds: the batch is not a Thirion's Demons batch");
        on_cu_ = flag_value(key, v);
    } else
        throw std::invalid_argument("unknown option: " + key);
}

void Batch::ensure_device() {
    if (ready_) {
        OF2D_HIP(hipSetDevice(home_));  // the entry point's DeviceScope restores the caller's
        return;
    }
    // a failure partway leaves nothing behind: the next call starts afresh
    try {
        allocate_device();
    } catch (...) {
        release_device();
        throw;
    }
    ready_ = true;
}

// a table on the device
template <class T>
static void upload(DevArray<T> &d, const std::vector<T> &h) {
    d.alloc(h.size());
    OF2D_HIP(hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
}

void Batch::allocate_device() {
    if (device_ >= 0) OF2D_HIP(hipSetDevice(device_));
    OF2D_HIP(hipGetDevice(&home_));
    OF2D_HIP(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
    lv_.resize(nscales_ + 1);
    for (int s = 0; s <= nscales_; s++) {
        BLevel &L = lv_[s];
        L.dx = ldx_[s];
        L.dy = ldy_[s];
        L.P = pitch_for(L.dx);
        L.stride = pair_stride(L.dx, L.dy);
        // Iref: set_images allocates it, one image or B (ensure_reference)
        L.Imov.alloc(L.dx, L.dy, B_);
        L.Iaux.alloc(L.dx, L.dy, B_);
        L.It.alloc(L.dx, L.dy, B_);
        L.motion[0].alloc(L.dx, L.dy, B_);
        L.motion[1].alloc(L.dx, L.dy, B_);
        L.dI.alloc(L.dx, L.dy, B_);
        L.est[0].alloc(L.dx, L.dy, B_);
        L.est[1].alloc(L.dx, L.dy, B_);
        // the kind's own scratch (option "fluid" can change an Elastic batch's
        // kind later: both take the force)
        switch (kind()) {
            case LoopKind::HornSchunck: break;
            case LoopKind::Demons: L.mid.alloc(L.dx, L.dy, B_); break;
            case LoopKind::Elastic:
            case LoopKind::Fluid: L.force.alloc(L.dx, L.dy, B_); break;
            case LoopKind::Curvature:
                // the level's tables by the one-pair path's own builders
                // (solvers::build_curvature), E dense
                L.cX.alloc(curv_scratch_doubles(L.dx, L.dy) * B_);
                upload(L.cE, curvature_eigenvalues(L.dx, L.dy, L.dx, alpha_, tau_));
                upload(L.ctwx, dct_table(L.dx));
                upload(L.ctwy, dct_table(L.dy));
                break;
        }
    }
    if (kind() == LoopKind::Demons) {
        // both tables once per Batch, sigma_fluid's first (Registration::loop_demons)
        std::vector<double> kd(kfluid_);
        kd.insert(kd.end(), kdiff_.begin(), kdiff_.end());
        upload(d_kd_, kd);
        upload(d_kf_, std::vector<float>(kd.begin(), kd.end()));
    }
    stage_pairs_ = stage_chunk_pairs(B_, dimx_, dimy_);  // 64 MiB of doubles at most
    d_stage_.alloc(stage_pairs_ * 2 * (size_t)dimx_ * dimy_);
    d_status_.alloc(B_);
    d_iters_.alloc((size_t)B_ * nloops_);
    ev_.assign(2 * (size_t)nloops_, nullptr);
    for (hipEvent_t &e : ev_) OF2D_HIP(hipEventCreate(&e));
    for (hipEvent_t &e : ev_io_) OF2D_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    // the null-stream memsets are unordered with the non-blocking stream
    OF2D_HIP(hipDeviceSynchronize());
}

// Iref of every level holds npairs images: one for a shared reference, else B.
// The stream is idle here (set_images and estimate end in a synchronise).
void Batch::ensure_reference(int npairs) {
    if (ref_pairs_ >= npairs) return;
    ref_pairs_ = 0;  // a failure partway: the next call allocates every level again
    have_images_ = false;
    for (BLevel &L : lv_) L.Iref.alloc(L.dx, L.dy, npairs);
    OF2D_HIP(hipDeviceSynchronize());  // null-stream memsets, as above
    ref_pairs_ = npairs;
}

// ImageRegistration::set_reference_image / set_moving_image per pair
void Batch::set_images(const double *ref, bool shared_ref, const double *mov) {
    DeviceScope scope;  // the caller's device again on return
    ensure_device();
    ensure_reference(shared_ref ? 1 : B_);
    BLevel &L0 = lv_[0];
    for (int which = 0; which < 2; which++) {
        const double *src = which ? mov : ref;
        float *dst = which ? L0.Imov.p : L0.Iref.p;
        const int npairs = (!which && shared_ref) ? 1 : B_;
        for_rounds(npairs, [&](const StageRound &r) { images_in(r, src, dst); });
        downsample_levels(which, npairs);
    }
    images_in_place(shared_ref);
}

// ---- one staging round's launches (of2d_batch.h, for_rounds)
void Batch::images_in(const StageRound &r, const double *host, float *field) {
    const BLevel &L0 = lv_[0];
    OF2D_HIP(hipMemcpyAsync(d_stage_.p, host + r.image,
                            sizeof(double) * r.nk * (size_t)dimx_ * dimy_, hipMemcpyHostToDevice,
                            st_));
    launch_d2f(d_stage_.p, r.nk, dimx_, dimy_, field + r.field, L0.stride, L0.P, st_);
}
void Batch::images_out(const StageRound &r, const float *field, double *host) {
    const BLevel &L0 = lv_[0];
    launch_f2d(field + r.field, L0.stride, L0.P, dimx_, dimy_, d_stage_.p, r.nk, st_);
    OF2D_HIP(hipMemcpyAsync(host + r.image, d_stage_.p,
                            sizeof(double) * r.nk * (size_t)dimx_ * dimy_, hipMemcpyDeviceToHost,
                            st_));
}
void Batch::motion_in(const StageRound &r, const double *host, float2 *field) {
    const BLevel &L0 = lv_[0];
    OF2D_HIP(hipMemcpyAsync(d_stage_.p, host + r.motion,
                            sizeof(double) * 2 * r.nk * (size_t)dimx_ * dimy_,
                            hipMemcpyHostToDevice, st_));
    launch_planar_to_motion(d_stage_.p, r.nk, dimx_, dimy_, field + r.field, L0.stride, L0.P, st_);
}
void Batch::motion_out(const StageRound &r, const float2 *field, double *host) {
    const BLevel &L0 = lv_[0];
    launch_motion_to_planar(field + r.field, L0.stride, L0.P, dimx_, dimy_, d_stage_.p, r.nk, st_);
    OF2D_HIP(hipMemcpyAsync(host + r.motion, d_stage_.p,
                            sizeof(double) * 2 * r.nk * (size_t)dimx_ * dimy_,
                            hipMemcpyDeviceToHost, st_));
}

// the same from the caller's device arrays (include/of2d.h, the stream
// contract): one pack launch per stack, no staging
void Batch::set_images_device(const DArrayView &ref, bool shared_ref, const DArrayView &mov,
                              hipStream_t user) {
    DeviceScope scope;
    ensure_device();
    check_device_pointer(ref.ptr, home_, "of2d_batch_set_images_device: Iref");
    check_device_pointer(mov.ptr, home_, "of2d_batch_set_images_device: Imov");
    const int nref = shared_ref ? 1 : B_;
    ensure_reference(nref);
    BLevel &L0 = lv_[0];
    stream_after(st_, user, ev_io_[0]);
    launch_pack_image(ref, nref, dimx_, dimy_, L0.Iref.p, L0.stride, L0.P, st_);
    launch_pack_image(mov, B_, dimx_, dimy_, L0.Imov.p, L0.stride, L0.P, st_);
    stream_after(user, st_, ev_io_[1]);  // the caller's arrays are free again
    downsample_levels(0, nref);
    downsample_levels(1, B_);
    images_in_place(shared_ref);
}

// the pyramid of the reference (0) or moving (1) images below level 0
void Batch::downsample_levels(int which, int npairs) {
    BLevel &L0 = lv_[0];
    for (int s = nscales_; s >= 1; s--) {
        BLevel &L = lv_[s];
        launch_downsample_image((which ? L0.Imov : L0.Iref).p, L0.stride, L0.dx, L0.dy, L0.P,
                                (which ? L.Imov : L.Iref).p, L.stride, L.dx, L.dy, L.P, npairs,
                                st_);
    }
}

// what set_images does once both pyramids are enqueued
void Batch::images_in_place(bool shared_ref) {
    OF2D_HIP(hipStreamSynchronize(st_));
    shared_ = shared_ref;
    have_images_ = true;
}

// ImageRegistration::estimate_motion (:133-156) for every pair, each from a
// zero motion field (as a new ImageRegistration's first estimate); with
// warm_start from the motion every level holds, as a reused ImageRegistration
// (estimate_motion resets nothing): level nscales continues from its own
// motion, the levels between are downsampled from level 0, and level 0 is
// overwritten by the upsample when nscales >= 1
void Batch::estimate() {
    DeviceScope scope;
    ensure_device();
    if (!have_images_) throw std::invalid_argument("of2d_batch_estimate: no images set");
    const LoopKind kind = this->kind();
    const bool conv = !fixed_;
    const bool fluid = kind == LoopKind::Fluid;
    if (conv && !d_errs_.p && maxn_ > 0 && nloops_ > 0)
        d_errs_.alloc((size_t)B_ * nloops_ * maxn_);
    if (fluid) prepare_fluid();
    launches_ = 0;
    pair_err_.clear();
    OF2D_HIP(hipMemsetAsync(d_status_.p, 0, sizeof(unsigned) * B_, st_));
    // option "resident" or "conv_lds": asked of the runtime once per handle; a
    // refusal there is "no level fits", not an error.  (on_cu_ is set for the
    // two kinds of on_cu_option only; a third needs its prepare named here)
    if (on_cu_ && on_cu_ok_ < 0)
        on_cu_ok_ = (kind == LoopKind::Demons ? conv_lds_prepare() : resident_prepare()) ? 1 : 0;
    placement_.assign(nscales_ + 1, 0);
    if (on_cu_ && on_cu_ok_ == 1)
        for (int s = 0; s <= nscales_; s++)
            placement_[s] = on_cu_fits(kind, ldx_[s], ldy_[s]) ? 1 : 0;
    const bool warm = warm_;
    if (!warm)
        for (BLevel &L : lv_) {
            L.mcur = 0;
            OF2D_HIP(hipMemsetAsync(L.motion[0].base, 0, L.motion[0].bytes(), st_));
        }
    BLevel &L0 = lv_[0];
    int loop = 0;
    for (int s = nscales_; s >= 0; s--) {
        BLevel &L = lv_[s];
        if (s > 0 && s < nscales_) {
            launch_downsample_motion(L0.motion[L0.mcur].p, L0.stride, L0.dx, L0.dy, L0.P,
                                     L.motion[L.mcur].p, L.stride, L.dx, L.dy, L.P, B_, d_status_.p,
                                     st_);
            launches_++;
        }
        // estimate_motion_at_current_resolution
        for (int refine = 0; refine < nrefine_; refine++, loop++) {
            // *Iaux = *Imov; Iaux->warp2d(*motion)
            launch_warp(L.Imov.p, L.motion[L.mcur].p, L.Iaux.p, L.stride, L.dx, L.dy, L.P, B_,
                        d_status_.p, st_);
            if (loop_takes_gradients(kind))
                launch_gradients(L.Iref.p, shared_ ? 0 : L.stride, L.Iaux.p, L.dI.p, L.It.p,
                                 L.stride, L.dx, L.dy, L.P, B_, d_status_.p, st_);
            // motion_est starts at zero
            OF2D_HIP(hipMemsetAsync(L.est[0].base, 0, L.est[0].bytes(), st_));
            launch_loop(s, loop, conv);
            // motion->accumulate(*motion_est)
            launch_accumulate(L.motion[L.mcur].p, L.est[0].p, L.est[1].p, L.motion[1 - L.mcur].p,
                              L.stride, L.dx, L.dy, L.P, B_, d_iters_.p, nloops_, loop, d_status_.p,
                              st_);
            L.mcur ^= 1;
            launches_ += loop_launches(kind);
        }
        if (s > 0) {
            launch_upsample_motion(L.motion[L.mcur].p, L.stride, L.dx, L.dy, L.P,
                                   L0.motion[L0.mcur].p, L0.stride, L0.dx, L0.dy, L0.P, B_,
                                   d_status_.p, st_);
            launches_++;
        }
    }
    // a divide-by-zero pair's motion is left zero; with warm_start at every
    // level, so that the pair's next estimate starts as a fresh handle's
    for (int s = 0; s <= (warm ? nscales_ : 0); s++) {
        BLevel &L = lv_[s];
        launch_zero_failed(L.motion[L.mcur].base, L.stride, B_, d_status_.p, st_);
        launches_++;
    }
    OF2D_HIP(hipMemcpyAsync(h_status_.data(), d_status_.p, sizeof(unsigned) * B_,
                            hipMemcpyDeviceToHost, st_));
    if (nloops_ > 0)
        OF2D_HIP(hipMemcpyAsync(h_iters_.data(), d_iters_.p, sizeof(int) * h_iters_.size(),
                                hipMemcpyDeviceToHost, st_));
    // a lazy buffer's content where this estimate wrote it, else nothing
    auto fetch = [&](std::vector<float> &h, const DevArray<float> &d, bool on) {
        h.resize(on ? d.n : 0);
        if (!h.empty())
            OF2D_HIP(hipMemcpyAsync(h.data(), d.p, sizeof(float) * d.n, hipMemcpyDeviceToHost, st_));
    };
    fetch(h_errs_, d_errs_, conv);
    fetch(h_flog_, d_flog_, fluid);
    OF2D_HIP(hipStreamSynchronize(st_));
    loop_us_ = 0.0;
    for (int l = 0; l < nloops_; l++) {
        float ms = 0.0f;
        OF2D_HIP(hipEventElapsedTime(&ms, ev_[2 * l], ev_[2 * l + 1]));
        loop_us_ += 1000.0 * (double)ms;
    }
    for (int k = 0; k < B_; k++)
        if (h_status_[k] & kStatusDivZero) {
            pair_err_ = "Divide by zero exception (pair " + std::to_string(k) + ")";
            break;
        }
}

// option "fluid", before an estimate: the velocity, a field per pair and level
// that outlives the estimate (OpticalFlowFluid::velocity), and the log
void Batch::prepare_fluid() {
    if (!have_velocity()) {
        for (BLevel &L : lv_) L.vel.alloc(L.dx, L.dy, B_);
        OF2D_HIP(hipDeviceSynchronize());  // null-stream memsets, as allocate_device's
    }
    if (!d_flog_.p && maxn_ > 0 && nloops_ > 0)
        d_flog_.alloc((size_t)kFluidLogFloats * B_ * nloops_ * maxn_);
    // a fresh handle's velocity; with warm_start it carries over, as a
    // reused one-pair object's
    if (!warm_) zero_velocity();
}

// loop `loop` of level s, the iterate in est[]: the common arguments, the
// kind's own, the kernel by placement_[s], between the loop's events
void Batch::launch_loop(int s, int loop, bool conv) {
    BLevel &L = lv_[s];
    LoopCommon c;
    c.u0 = L.est[0].p;
    c.u1 = L.est[1].p;
    c.stride = L.stride;
    c.dx = L.dx;
    c.dy = L.dy;
    c.P = L.P;
    c.niter = niter_[s];
    c.status = d_status_.p;
    c.iters = d_iters_.p;
    c.nloops = nloops_;
    c.loop = loop;
    c.errs = d_errs_.p;
    c.maxn = maxn_;
    const bool on_cu = placement_[s] != 0;
    OF2D_HIP(hipEventRecord(ev_[2 * loop], st_));
    switch (kind()) {
        case LoopKind::HornSchunck:
            (on_cu ? launch_hs_resident : launch_hs_loop)(hs_args(c, L), B_, conv, st_);
            break;
        case LoopKind::Curvature: launch_curv_loop(curv_args(c, L), B_, conv, st_); break;
        case LoopKind::Elastic: launch_elastic_loop(elastic_args(c, L), B_, conv, st_); break;
        case LoopKind::Fluid: launch_fluid_loop(fluid_args(c, L), B_, conv, st_); break;
        case LoopKind::Demons:
            (on_cu ? launch_demons_lds : launch_demons_loop)(demons_args(c, L), B_, conv, st_);
            break;
    }
    OF2D_HIP(hipEventRecord(ev_[2 * loop + 1], st_));
}

// ---- c and a kind's own arguments at level L
LoopArgs Batch::hs_args(const LoopCommon &c, BLevel &L) const {
    LoopArgs a{c};
    a.dI = L.dI.p;
    a.It = L.It.p;
    a.alphasq = alpha_ * alpha_;  // OpticalFlowDiffusion.cpp:70
    return a;
}

CurvLoopArgs Batch::curv_args(const LoopCommon &c, BLevel &L) const {
    CurvLoopArgs a{c};
    a.dI = L.dI.p;
    a.It = L.It.p;
    a.X = L.cX.p;
    a.sx = (long)curv_scratch_doubles(L.dx, L.dy);
    a.E = L.cE.p;
    a.twx = reinterpret_cast<const double2 *>(L.ctwx.p);
    a.twy = reinterpret_cast<const double2 *>(L.ctwy.p);
    a.tau = tau_;
    a.div = 4.0f * (float)((unsigned)L.dx * (unsigned)L.dy);  // 4.0f*sizein
    a.logx = a.logy = 0;
    while ((1 << a.logx) < L.dx) a.logx++;
    while ((1 << a.logy) < L.dy) a.logy++;
    a.lx = curv_chunk_lines(L.dx, L.dy);
    a.ly = curv_chunk_lines(L.dy, L.dx);
    return a;
}

// what the Elastic and the Fluid loop share: the derivatives, the force plane
// and the sweep's constants
template <class Args>
static Args sweep_args(const LoopCommon &c, BLevel &L, const SorCoef &k) {
    Args a{c};
    a.dI = L.dI.p;
    a.It = L.It.p;
    a.f = L.force.p;
    a.k = k;
    return a;
}

ElasticLoopArgs Batch::elastic_args(const LoopCommon &c, BLevel &L) const {
    return sweep_args<ElasticLoopArgs>(c, L, sor_);
}

FluidLoopArgs Batch::fluid_args(const LoopCommon &c, BLevel &L) const {
    FluidLoopArgs a = sweep_args<FluidLoopArgs>(c, L, sor_);
    a.vel = L.vel.p;
    a.m_cur = L.motion[L.mcur].p;
    a.m_other = L.motion[1 - L.mcur].p;
    a.Iref = L.Iref.p;
    a.sref = shared_ ? 0 : L.stride;
    a.Imov = L.Imov.p;
    a.Iaux = L.Iaux.p;
    a.log = d_flog_.p;
    return a;
}

// c and Thirion's Demons' own arguments at level L: It as the warped image, dI
// as the correction
DemonsLoopArgs Batch::demons_args(const LoopCommon &c, BLevel &L) const {
    const size_t n = kfluid_.size();
    const int kw = (int)(unsigned)params_[4];
    DemonsLoopArgs a{c};
    a.Iref = L.Iref.p;
    a.sref = shared_ ? 0 : L.stride;
    a.Iaux = L.Iaux.p;
    a.W = L.It.p;
    a.corr = L.dI.p;
    a.mid = L.mid.p;
    // Demons.cpp:48-49
    a.sigma_isq = params_[0] * params_[0];
    a.sigma_xsq = params_[1] * params_[1];
    a.fluid = DemonsTable{d_kf_.p, d_kd_.p, full_weight(kfluid_, kw)};
    a.diff = DemonsTable{d_kf_.p + n, d_kd_.p + n, full_weight(kdiff_, kw)};
    a.kw = kw;
    // static_cast<MotionAccumulation>((int) regparams[5]), as loop_demons
    const int accum = (int)params_[5];
    a.mode = accum == 0 ? 0 : (accum == 1 ? 1 : 2);
    a.diffeomorphic = diffeo_ ? 1 : 0;  // set_option admits it with mode 0 only
    return a;
}

void Batch::get_motion(double *out) {
    DeviceScope scope;
    ensure_device();
    const float2 *m = lv_[0].motion[lv_[0].mcur].p;
    for_rounds(B_, [&](const StageRound &r) { motion_out(r, m, out); });
}

// get_motion's reverse into level 0's current buffer, through the same
// staging rounds; then the coarsest level (motion_in_place)
void Batch::set_motion(const double *in) {
    DeviceScope scope;
    ensure_device();
    float2 *m = lv_[0].motion[lv_[0].mcur].p;
    for_rounds(B_, [&](const StageRound &r) { motion_in(r, in, m); });
    motion_in_place();
}

void Batch::set_motion_device(const DArrayView &in, hipStream_t user) {
    DeviceScope scope;
    ensure_device();
    check_device_pointer(in.ptr, home_, "of2d_batch_set_motion_device: motion");
    BLevel &L0 = lv_[0];
    stream_after(st_, user, ev_io_[0]);
    launch_pack_motion(in, B_, dimx_, dimy_, L0.motion[L0.mcur].p, L0.stride, L0.P, st_);
    stream_after(user, st_, ev_io_[1]);  // the caller's array is free again
    motion_in_place();
}

// Level nscales is the one level a warm estimate neither downsamples into nor
// overwrites before reading: it takes Motion::downSample of the supplied
// field, so that the estimate starts from it at every level
void Batch::motion_in_place() {
    if (nscales_ >= 1) {
        BLevel &L0 = lv_[0], &L = lv_[nscales_];
        launch_downsample_motion(L0.motion[L0.mcur].p, L0.stride, L0.dx, L0.dy, L0.P,
                                 L.motion[L.mcur].p, L.stride, L.dx, L.dy, L.P, B_, nullptr, st_);
    }
    OF2D_HIP(hipStreamSynchronize(st_));
}

// option "fluid": every level's velocity <- 0 (enqueued)
void Batch::zero_velocity() {
    for (BLevel &L : lv_)
        if (L.vel.base) OF2D_HIP(hipMemsetAsync(L.vel.base, 0, L.vel.bytes(), st_));
}

// every level as allocate_device left it; the velocity of option "fluid" too,
// as Registration::reset_motion's
void Batch::reset_motion() {
    DeviceScope scope;
    ensure_device();
    for (BLevel &L : lv_) {
        L.mcur = 0;
        for (BField<float2> &m : L.motion) OF2D_HIP(hipMemsetAsync(m.base, 0, m.bytes(), st_));
    }
    zero_velocity();
    OF2D_HIP(hipStreamSynchronize(st_));
}

// pair k's image by pair k's motion (WrapperOpticalFlow2d.cpp:120-137 per pair);
// level 0's Iaux and It are free between estimates and hold the images here
void Batch::warp(const double *in, double *out) {
    DeviceScope scope;
    ensure_device();
    BLevel &L0 = lv_[0];
    // upload, warp and download of a round's pairs before the next round
    for_rounds(B_, [&](const StageRound &r) {
        images_in(r, in, L0.Iaux.p);
        launch_warp(L0.Iaux.p + r.field, L0.motion[L0.mcur].p + r.field, L0.It.p + r.field,
                    L0.stride, dimx_, dimy_, L0.P, r.nk, nullptr, st_);
        images_out(r, L0.It.p, out);
    });
}

void Batch::get_motion_device(const DArrayView &out, hipStream_t user) {
    DeviceScope scope;
    ensure_device();
    check_device_pointer(out.ptr, home_, "of2d_batch_get_motion_device: out");
    BLevel &L0 = lv_[0];
    stream_after(st_, user, ev_io_[0]);
    launch_unpack_motion(L0.motion[L0.mcur].p, L0.stride, L0.P, B_, dimx_, dimy_, out, st_);
    stream_after(user, st_, ev_io_[1]);
}

// as warp: level 0's Iaux and It hold the images
void Batch::warp_device(const DArrayView &in, const DArrayView &out, hipStream_t user) {
    DeviceScope scope;
    ensure_device();
    check_device_pointer(in.ptr, home_, "of2d_batch_warp_device: Imov");
    check_device_pointer(out.ptr, home_, "of2d_batch_warp_device: out");
    BLevel &L0 = lv_[0];
    stream_after(st_, user, ev_io_[0]);
    launch_pack_image(in, B_, dimx_, dimy_, L0.Iaux.p, L0.stride, L0.P, st_);
    launch_warp(L0.Iaux.p, L0.motion[L0.mcur].p, L0.It.p, L0.stride, dimx_, dimy_, L0.P, B_,
                nullptr, st_);
    launch_unpack_image(L0.It.p, L0.stride, L0.P, B_, dimx_, dimy_, out, st_);
    stream_after(user, st_, ev_io_[1]);
}

// ------------------------------------------------------------ analysis
// (of2d_batch.h; the kernels: batch_analysis_kernels.hip.)  Scratch at level 0,
// free between estimates as warp's: It holds the Jacobian maps or the warped
// images, Iaux the moving images, est[0] the inverse (estimate() zeroes est[0]
// before every loop and writes est[1] before reading it, and nothing reads
// either after an estimate).  The stored images and the motion are only read.
double *Batch::analysis_words() {
    if (!d_words_.p) d_words_.alloc(5 * (size_t)B_);
    return d_words_.p;
}

void Batch::fetch_words(double *host, int per_pair) {
    OF2D_HIP(hipMemcpyAsync(host, d_words_.p, sizeof(double) * per_pair * (size_t)B_,
                            hipMemcpyDeviceToHost, st_));
    OF2D_HIP(hipStreamSynchronize(st_));
}

void Batch::ensure_quality_reference(int npairs) {
    if (qref_pairs_ >= npairs) return;
    qref_pairs_ = 0;
    qref_.alloc(dimx_, dimy_, npairs);
    OF2D_HIP(hipDeviceSynchronize());  // null-stream memset, as ensure_reference
    qref_pairs_ = npairs;
}

void Batch::run_jacobian(bool map) {
    BLevel &L0 = lv_[0];
    JacobianArgs a;
    a.u = L0.motion[L0.mcur].p;
    a.stride = L0.stride;
    a.dx = dimx_;
    a.dy = dimy_;
    a.P = L0.P;
    a.jac = map ? L0.It.p : nullptr;
    a.stats = analysis_words();
    launch_batch_jacobian(a, B_, st_);
}

void Batch::jacobian(double *jac, double *stats) {
    if (const char *why = jacobian_refusal(dimx_, dimy_)) throw std::invalid_argument(why);
    DeviceScope scope;
    ensure_device();
    run_jacobian(jac != nullptr);
    if (jac) for_rounds(B_, [&](const StageRound &r) { images_out(r, lv_[0].It.p, jac); });
    fetch_words(stats, 5);
}

void Batch::jacobian_device(const DArrayView *jac, double *stats, hipStream_t user) {
    if (const char *why = jacobian_refusal(dimx_, dimy_)) throw std::invalid_argument(why);
    DeviceScope scope;
    ensure_device();
    if (jac) check_device_pointer(jac->ptr, home_, "of2d_batch_jacobian_device: jac");
    BLevel &L0 = lv_[0];
    if (jac) stream_after(st_, user, ev_io_[0]);
    run_jacobian(jac != nullptr);
    if (jac) {
        launch_unpack_image(L0.It.p, L0.stride, L0.P, B_, dimx_, dimy_, *jac, st_);
        stream_after(user, st_, ev_io_[1]);
    }
    fetch_words(stats, 5);
}

void Batch::run_invert(int max_iter, double tol) {
    BLevel &L0 = lv_[0];
    InvertArgs a;
    a.u = L0.motion[L0.mcur].p;
    a.v = L0.est[0].p;
    a.stride = L0.stride;
    a.dx = dimx_;
    a.dy = dimy_;
    a.P = L0.P;
    a.max_iter = max_iter;
    a.tol = (float)tol;
    a.info = analysis_words();
    a.residuals = nullptr;
    launch_batch_invert(a, B_, st_);
}

void Batch::invert_motion(int max_iter, double tol, double *out, double *info) {
    if (const char *why = invert_refusal(dimx_, dimy_, max_iter, tol))
        throw std::invalid_argument(why);
    DeviceScope scope;
    ensure_device();
    run_invert(max_iter, tol);
    if (out) for_rounds(B_, [&](const StageRound &r) { motion_out(r, lv_[0].est[0].p, out); });
    fetch_words(info, 4);
}

void Batch::invert_motion_device(int max_iter, double tol, const DArrayView &out, double *info,
                                 hipStream_t user) {
    if (const char *why = invert_refusal(dimx_, dimy_, max_iter, tol))
        throw std::invalid_argument(why);
    DeviceScope scope;
    ensure_device();
    check_device_pointer(out.ptr, home_, "of2d_batch_invert_motion_device: out");
    BLevel &L0 = lv_[0];
    stream_after(st_, user, ev_io_[0]);
    run_invert(max_iter, tol);
    launch_unpack_motion(L0.est[0].p, L0.stride, L0.P, B_, dimx_, dimy_, out, st_);
    stream_after(user, st_, ev_io_[1]);
    fetch_words(info, 4);
}

// Iref in qref_ (one image or B), Imov in Iaux: the warp, then {mse, ncc} of
// (Iref, Imov) and of (Iref, warped) into a pair's four words
void Batch::run_quality(bool shared_ref) {
    BLevel &L0 = lv_[0];
    launch_warp(L0.Iaux.p, L0.motion[L0.mcur].p, L0.It.p, L0.stride, dimx_, dimy_, L0.P, B_,
                nullptr, st_);
    SimilarityArgs a;
    a.a = qref_.p;
    a.sa = shared_ref ? 0 : L0.stride;
    a.b = L0.Iaux.p;
    a.sb = L0.stride;
    a.dx = dimx_;
    a.dy = dimy_;
    a.P = L0.P;
    a.out = analysis_words();
    a.so = 4;
    launch_batch_similarity(a, B_, st_);
    a.b = L0.It.p;
    a.out += 2;
    launch_batch_similarity(a, B_, st_);
}

void Batch::quality(const double *ref, bool shared_ref, const double *mov, double *out) {
    DeviceScope scope;
    ensure_device();
    ensure_quality_reference(shared_ref ? 1 : B_);
    BLevel &L0 = lv_[0];
    for (int which = 0; which < 2; which++) {
        const double *src = which ? mov : ref;
        float *dst = which ? L0.Iaux.p : qref_.p;
        const int npairs = (!which && shared_ref) ? 1 : B_;
        for_rounds(npairs, [&](const StageRound &r) { images_in(r, src, dst); });
    }
    run_quality(shared_ref);
    fetch_words(out, 4);
}

void Batch::quality_device(const DArrayView &ref, bool shared_ref, const DArrayView &mov,
                           double *out, hipStream_t user) {
    DeviceScope scope;
    ensure_device();
    check_device_pointer(ref.ptr, home_, "of2d_batch_quality_device: Iref");
    check_device_pointer(mov.ptr, home_, "of2d_batch_quality_device: Imov");
    const int nref = shared_ref ? 1 : B_;
    ensure_quality_reference(nref);
    BLevel &L0 = lv_[0];
    stream_after(st_, user, ev_io_[0]);
    launch_pack_image(ref, nref, dimx_, dimy_, qref_.p, L0.stride, L0.P, st_);
    launch_pack_image(mov, B_, dimx_, dimy_, L0.Iaux.p, L0.stride, L0.P, st_);
    stream_after(user, st_, ev_io_[1]);  // the caller's arrays are free again
    run_quality(shared_ref);
    fetch_words(out, 4);
}

std::vector<float> Batch::last_errors(int pair) const {
    std::vector<float> v;
    if (pair < 0 || pair >= B_ || h_errs_.empty() || nloops_ == 0) return v;
    const size_t loop = (size_t)pair * nloops_ + (nloops_ - 1);
    const int n = std::min(h_iters_[loop], maxn_);
    v.assign(h_errs_.begin() + loop * maxn_, h_errs_.begin() + loop * maxn_ + n);
    return v;
}

std::vector<float> Batch::fluid_log(int pair, int loop) const {
    std::vector<float> v;
    if (pair < 0 || pair >= B_ || loop < 0 || loop >= nloops_ || h_flog_.empty()) return v;
    const size_t l = (size_t)pair * nloops_ + loop;
    const int n = std::min(h_iters_[l], maxn_);
    const float *p = h_flog_.data() + l * maxn_ * kFluidLogFloats;
    v.assign(p, p + (size_t)n * kFluidLogFloats);
    return v;
}

std::vector<int> Batch::info() const {
    std::vector<int> v = {launches_, nloops_, nscales_ + 1, (int)std::lround(loop_us_)};
    for (int s = 0; s <= nscales_; s++) {
        // 0: every field of the loop in global memory; 1: the iterate
        // (resident) or the convolved field (conv_lds) stays on the CU
        v.push_back(s < (int)placement_.size() ? placement_[s] : 0);
        v.push_back(loop_threads(kind(), ldx_[s]));
    }
    return v;
}

}  // namespace batch
}  // namespace of2d
