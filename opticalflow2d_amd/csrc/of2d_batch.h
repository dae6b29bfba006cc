// of2d_batch.h — B independent Horn-Schunck, Curvature, Elastic, Fluid or Thirion's
// Demons registrations of one size in one call, and the deformation analysis of
// their motions (batch.cpp, batch_kernels.hip, batch_resident_kernels.hip,
// batch_curvature_kernels.hip, batch_elastic_kernels.hip, batch_fluid_kernels.hip,
// batch_demons_kernels.hip, batch_demons_lds_kernels.hip,
// batch_analysis_kernels.hip; the loop kernels' frame: batch_loop.h; the sweep
// of the Elastic and Fluid loops: batch_sweep.h; the host arithmetic and what
// each kind of loop needs: batch_plan.h).
//
// Layout: the B fields of a pyramid level live in one allocation, pair k at
// k * stride elements, each laid out exactly as a Field<T> (of2d_host.h): the
// pitch of pitch_for(dimx), one zeroed ghost j-line above row 0 and one below
// the last row, kPitchAlign elements of slack; stride = (dimy + 2) * P +
// kPitchAlign for every element type.  The per-pixel code (field_px.h,
// accumulate_px, hs::update_px) therefore sees what it sees in the one-pair
// path.  Pointers passed to the launches address row 0 of pair 0.
//
// One workgroup runs the whole iteration loop of one pair; no workgroup waits
// for another.  The passes around the loop take the pair as grid dimension z.
// Every kernel of an estimate returns at once for a pair whose status word has
// kStatusDivZero set, so that pair's fields stop changing and the others run on.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "batch_loop.h"
#include "batch_plan.h"
#include "of2d_device.h"
#include "of2d_host.h"
#include "sor_px.h"

namespace of2d {
namespace batch {

constexpr int kMaxPx = 512 * 512;   // OF2D_BATCH_MAXPX
constexpr int kMaxPairs = 65535;    // the pair is grid dimension z of the passes

inline long pair_stride(int dimx, int dimy) {
    return (long)(dimy + 2) * pitch_for(dimx) + kPitchAlign;
}
static_assert(sizeof(float2) == kLdsElementBytes, "batch_plan.h counts LDS in float2 elements");

// the common arguments (batch_loop.h) and the Horn-Schunck loop's own
struct LoopArgs : LoopCommon {
    const float2 *dI;
    const float *It;
    float alphasq;
};
// conv: Logger sums, errors and the reference's break (fp64 sums in a fixed
// order: the logger_fp64 semantics); otherwise exactly niter iterations
void launch_hs_loop(const LoopArgs &a, int B, bool conv, hipStream_t st);

// Curvature (batch_curvature_kernels.hip): the pair's whole
// loop of OpticalFlowCurvature::get_update with the fast line transforms, the
// fp64 plane pair in the pair's slice of X.  curv_level_ok(dx, dy) must hold
struct CurvLoopArgs : LoopCommon {
    const float2 *dI;
    const float *It;
    double *X;           // scratch: [B][curv_scratch_doubles(dx, dy)]
    long sx;             // X's pair stride in doubles
    const double *E;     // the level's eigenvalues, element (p, q) at p + q * dx
    const double2 *twx;  // dct_table(dx), dct_table(dy)
    const double2 *twy;
    float tau;
    float div;           // 4.0f * sizein
    int logx, logy;      // log2 of dx, dy
    int lx, ly;          // lines per chunk of a pass along x, along y (curv_chunk_lines)
};
// conv as launch_hs_loop's
void launch_curv_loop(const CurvLoopArgs &a, int B, bool conv, hipStream_t st);

// Elastic (batch_elastic_kernels.hip): the pair's whole loop
// of OpticalFlowElastic::get_update, the force in the pair's slice of f and the
// SOR sweep in place on the iterate's output buffer, step after step of the
// reference's order (batch_plan.h, elastic_last_step).  The workgroup has
// elastic_threads(dx) threads
struct ElasticLoopArgs : LoopCommon {
    const float2 *dI;
    const float *It;
    float2 *f;  // scratch: the force, a field per pair
    SorCoef k;  // sor_coef(mu, lambda, omega)
};
// conv as launch_hs_loop's
void launch_elastic_loop(const ElasticLoopArgs &a, int B, bool conv, hipStream_t st);

// Fluid, option "fluid" of an Elastic batch (batch_fluid_kernels.hip, DESIGN.md
// §4.6.9): the pair's whole loop of ImageRegistrationFluid::
// estimate_motion_at_current_resolution with OpticalFlowFluid::get_update, the
// regrid inside.  The sweep is the Elastic loop's on the pair's velocity; the
// workgroup has elastic_threads(dx) threads; dx, dy >= 2.
// A record of the log: {maxabs, dt, jmin, regridded (0 or 1)}
constexpr int kFluidLogFloats = 4;
struct FluidLoopArgs : LoopCommon {
    float2 *dI;  // a regrid rewrites both
    float *It;
    float2 *f;    // scratch: the force, then the increment, a field per pair
    float2 *vel;  // the level's velocity, a field per pair; outlives the launch
    // the level's motion: the current buffer of every pair before and after
    // the launch, and the other one, which a regrid accumulates into
    float2 *m_cur, *m_other;
    const float *Iref;
    long sref;  // Iref's pair stride, 0 for a shared reference
    const float *Imov;
    float *Iaux;
    float *log;  // [B][nloops][maxn] records
    SorCoef k;   // sor_coef(mu, lambda, omega)
};
// conv as launch_hs_loop's; without it the break is off and the regrid stays on
void launch_fluid_loop(const FluidLoopArgs &a, int B, bool conv, hipStream_t st);

// ---- option "resident" (batch_resident_kernels.hip): the
// same loop with the pair's iterate in LDS and dI, It in registers across the
// iterations, at the levels that resident_fits (batch_plan.h).
// Once per device before the first launch: admits the dynamic LDS above the
// default limit for every instantiation; false when the runtime refuses (the
// caller then runs launch_hs_loop at every level)
bool resident_prepare();
// a, conv: launch_hs_loop's; resident_fits(a.dx, a.dy) must hold.  Dynamic LDS
// is the level's resident_lds_bytes, so a small level does not reserve a CU
void launch_hs_resident(const LoopArgs &a, int B, bool conv, hipStream_t st);

// One Gaussian table of the Demons loop on the device (Batch::allocate_device):
// (float) weights for the sums, double weights for the boundary weight sums,
// idx = (ii + c) + (jj + c) * kw, and the interior weight sum in the
// reference's order (full_weight, solvers.cpp)
struct DemonsTable {
    const float *kf = nullptr;
    const double *kd = nullptr;
    double wfull = 0.0;
};
// Thirion's Demons (batch_demons_kernels.hip): the pair's whole loop of
// DemonsThirions::get_update, staged through the pair's slices of W, corr and
// mid with a barrier after each stage; with `diffeomorphic` the loop of
// DemonsDiffeomorphic::get_update
struct DemonsLoopArgs : LoopCommon {
    const float *Iref;
    long sref;            // Iref's pair stride, 0 for a shared reference
    const float *Iaux;    // Imov warped by the level's motion
    float *W;             // scratch: Iaux warped by the iterate
    float2 *corr, *mid;   // scratch: the correction; the motion before the last smoothing
    float sigma_isq, sigma_xsq;  // Demons.cpp:48-49
    DemonsTable fluid, diff;
    int kw;
    int mode;             // 0 Composition, 1 Addition, 2 neither (launch_demons_update's)
    // option "diffeomorphic": Motion::exp of the smoothed correction before the
    // update (DemonsDiffeomorphic::get_update); mode is 0
    int diffeomorphic;
};
// conv as launch_hs_loop's
void launch_demons_loop(const DemonsLoopArgs &a, int B, bool conv, hipStream_t st);

// ---- option "conv_lds" (batch_demons_lds_kernels.hip): the
// same loop with the field its two convolutions read (the correction, then the
// motion before the last smoothing; with `diffeomorphic` every squaring of
// exp() too) in one dense float2 plane in LDS instead of the corr and mid
// slices, at the levels that conv_lds_fits (batch_plan.h).
// As resident_prepare: false when the runtime refuses the dynamic LDS (the
// caller then runs launch_demons_loop at every level)
bool conv_lds_prepare();
// a, conv: launch_demons_loop's (corr and mid are not used);
// conv_lds_fits(a.dx, a.dy) must hold.  Dynamic LDS is the level's
// conv_lds_bytes
void launch_demons_lds(const DemonsLoopArgs &a, int B, bool conv, hipStream_t st);

void launch_d2f(const double *in, int npairs, int dimx, int dimy, float *out, long so, int P,
                hipStream_t st);
void launch_f2d(const float *in, long si, int P, int dimx, int dimy, double *out, int npairs,
                hipStream_t st);
void launch_motion_to_planar(const float2 *m, long sm, int P, int dimx, int dimy, double *out,
                             int npairs, hipStream_t st);
void launch_downsample_image(const float *in, long si, int dxi, int dyi, int Pi, float *out,
                             long so, int dxo, int dyo, int Po, int B, hipStream_t st);
// status (the launches below): per-pair words, nullptr outside an estimate
void launch_downsample_motion(const float2 *in, long si, int dxi, int dyi, int Pi, float2 *out,
                              long so, int dxo, int dyo, int Po, int B, const unsigned *status,
                              hipStream_t st);
void launch_upsample_motion(const float2 *in, long si, int dxi, int dyi, int Pi, float2 *out,
                            long so, int dxo, int dyo, int Po, int B, const unsigned *status,
                            hipStream_t st);
void launch_warp(const float *src, const float2 *u, float *dst, long stride, int dimx, int dimy,
                 int P, int B, const unsigned *status, hipStream_t st);
// sref: Iref's pair stride, 0 for one reference shared by every pair
void launch_gradients(const float *Iref, long sref, const float *Iaux, float2 *dI, float *It,
                      long stride, int dimx, int dimy, int P, int B, const unsigned *status,
                      hipStream_t st);
// m_new <- accumulate(m_old, est) with est = v[iters[pair][loop] & 1]: the
// buffer holding the pair's last iterate
void launch_accumulate(const float2 *m_old, const float2 *v0, const float2 *v1, float2 *m_new,
                       long stride, int dimx, int dimy, int P, int B, const int *iters,
                       int nloops, int loop, const unsigned *status, hipStream_t st);
// the whole field of every pair with kStatusDivZero <- 0 (count: elements from
// m, the allocation's base, per pair)
void launch_zero_failed(float2 *m, long stride, int B, const unsigned *status, hipStream_t st);

// ---- analysis of every pair in one launch (batch_analysis_kernels.hip,
// DESIGN.md §4.6.2): one workgroup of kLoopThreads per pair, fixed-order fp64
// sums, no float atomics; two calls on the same input give the same bits.
// Fields are in the batch layout (stride = pair_stride, pitch P).
//
// The Jacobian determinant of id + u per pixel (jacobian_px) and per pair
// stats[5 * pair ...] = {min, max, mean, count(J <= 0), count(J < 0.5f)};
// dx, dy >= 2
struct JacobianArgs {
    const float2 *u;
    long stride;
    int dx, dy, P;
    float *jac;     // the map, a float field per pair (pixels only are written), or nullptr
    double *stats;  // [B][5]
};
void launch_batch_jacobian(const JacobianArgs &a, int B, hipStream_t st);
// invert_field's whole loop per pair (of2d_device.h), v_0 = 0 (v need not be
// zeroed: the first update does not read it): info[4 * pair ...] =
// {updates applied, m of the last one, out-of-bounds pixels at the last
// evaluated iterate, converged}; residuals[pair][k] = m_k, 0 beyond the last
// update.  Every pair stops on its own update.  dx, dy >= 2, max_iter >= 1
struct InvertArgs {
    const float2 *u;
    float2 *v;  // the result, updated in place; not u
    long stride;
    int dx, dy, P, max_iter;
    float tol;
    double *info;      // [B][4]
    float *residuals;  // [B][max_iter] or nullptr
};
void launch_batch_invert(const InvertArgs &a, int B, hipStream_t st);
// {mse, ncc} of images a and b of every pair (launch_similarity's definition:
// ncc is NaN when an image is constant) at out[pair * so], out[pair * so + 1]
struct SimilarityArgs {
    const float *a;
    long sa;  // a's pair stride, 0 for one image shared by every pair
    const float *b;
    long sb;
    int dx, dy, P;
    double *out;
    long so;
};
void launch_batch_similarity(const SimilarityArgs &a, int B, hipStream_t st);

template <class T>
struct BField {
    T *base = nullptr;
    T *p = nullptr;  // row 0 of pair 0
    size_t count = 0;
    BField() = default;
    BField(const BField &) = delete;
    BField &operator=(const BField &) = delete;
    BField(BField &&o) noexcept { *this = std::move(o); }
    BField &operator=(BField &&o) noexcept {
        std::swap(base, o.base);
        std::swap(p, o.p);
        std::swap(count, o.count);
        return *this;
    }
    ~BField() { release(); }
    void release() {
        if (base) (void)hipFree(base);
        base = p = nullptr;
        count = 0;
    }
    void alloc(int dimx, int dimy, int npairs) {
        release();
        count = (size_t)pair_stride(dimx, dimy) * npairs;
        OF2D_HIP(hipMalloc(&base, count * sizeof(T)));
        OF2D_HIP(hipMemset(base, 0, count * sizeof(T)));
        p = base + pitch_for(dimx);
    }
    size_t bytes() const { return count * sizeof(T); }
};

struct BLevel {
    int dx = 0, dy = 0, P = 0;
    long stride = 0;
    BField<float> Iref, Imov, Iaux, It;
    BField<float2> motion[2], dI, est[2];
    // Demons: It holds the image warped by the iterate and dI the correction;
    // mid (Demons only) the motion before the sigma_diffusion smoothing
    BField<float2> mid;
    // Curvature only: the pairs' fp64 scratch, and the tables every pair
    // shares (eigenvalues, dense; dct_table of each axis)
    DevArray<double> cX, cE, ctwx, ctwy;
    // Elastic only: the force of the iteration under way
    BField<float2> force;
    // option "fluid" only: the velocity (OpticalFlowFluid::velocity), allocated
    // by the first estimate that runs with it
    BField<float2> vel;
    int mcur = 0;
};

class Batch {
   public:
    // throws std::invalid_argument for everything of2d_batch_create refuses;
    // no device work
    Batch(int nbatch, int dimx, int dimy, const int *niter, int nscales, int reg,
          const float *params, unsigned nparams, int nrefine);
    ~Batch();
    void set_option(const std::string &key, double v);
    void set_images(const double *ref, bool shared_ref, const double *mov);
    void estimate();
    void get_motion(double *out);
    void warp(const double *in, double *out);
    // the same three on the caller's device arrays, ordered with the caller's
    // stream `user` (include/of2d.h, of2d_batch_set_images_device)
    void set_images_device(const DArrayView &ref, bool shared_ref, const DArrayView &mov,
                           hipStream_t user);
    void get_motion_device(const DArrayView &out, hipStream_t user);
    void warp_device(const DArrayView &in, const DArrayView &out, hipStream_t user);
    // ---- a motion from outside (include/of2d.h, of2d_batch_set_motion): into
    // level 0's current buffer, and as Motion::downSample of it into level
    // nscales's; no images are needed and the last estimate's status stays.
    // in: nbatch fields as get_motion writes them
    void set_motion(const double *in);
    void set_motion_device(const DArrayView &in, hipStream_t user);
    // every level's motion <- 0, mcur <- 0: a fresh handle's
    void reset_motion();
    // ---- analysis of the level-0 motion, per pair (batch_analysis_kernels.hip).
    // One or two launches whatever nbatch is.  The motion is zero before the
    // first estimate and for a pair whose status is OF2D_ERR_RUNTIME: such a
    // pair reports J = 1 everywhere, a zero inverse that converged at its first
    // update, and after == before, by the kernels' own arithmetic (no special
    // case).  The statistics, info and quality (5, 4 and 4 doubles per pair)
    // always return to host memory: every call here synchronises the library's
    // stream.  No call touches the images set_images stored or the motion: a
    // later estimate() gives the bits it would have given without them.
    //
    // jac (optional): nbatch maps as images; stats: nbatch x 5
    void jacobian(double *jac, double *stats);
    // out (optional): nbatch fields as get_motion's; info: nbatch x 4
    void invert_motion(int max_iter, double tol, double *out, double *info);
    // ref: one image (shared_ref) or nbatch, mov: nbatch, as set_images takes
    // them; out: nbatch x {mse_before, ncc_before, mse_after, ncc_after}
    void quality(const double *ref, bool shared_ref, const double *mov, double *out);
    // the same with the arrays on the device, ordered with the caller's stream
    // (jac may be null)
    void jacobian_device(const DArrayView *jac, double *stats, hipStream_t user);
    void invert_motion_device(int max_iter, double tol, const DArrayView &out, double *info,
                              hipStream_t user);
    void quality_device(const DArrayView &ref, bool shared_ref, const DArrayView &mov, double *out,
                        hipStream_t user);
    int nbatch() const { return B_; }
    int dimx() const { return dimx_; }
    int dimy() const { return dimy_; }
    int nloops() const { return nloops_; }
    const std::vector<unsigned> &status() const { return h_status_; }
    const std::vector<int> &iterations() const { return h_iters_; }
    std::vector<float> last_errors(int pair) const;
    // option "fluid": the records {maxabs, dt, jmin, regridded} of the
    // iterations pair's loop `loop` ran in the last estimate; empty without it
    std::vector<float> fluid_log(int pair, int loop) const;
    // launches of an estimate: max(nscales - 1, 0) downsamples + nloops * (4,
    // Demons 3) + nscales upsamples + 1 zeroing of failed pairs; with
    // warm_start nscales + 1 zeroings, one per level
    // {launches of the last estimate, loops per pair, levels, loop kernels'
    // device time of the last estimate in microseconds, then per level from 0:
    // placement in the last estimate (0: global memory; 1: on the CU, the
    // iterate with option "resident", the convolved field with option
    // "conv_lds"), threads of the pair's workgroup}
    std::vector<int> info() const;
    // "" or the first pair's divide-by-zero message
    const std::string &pair_error() const { return pair_err_; }

   private:
    void ensure_device();
    void allocate_device();
    void release_device();
    void ensure_reference(int npairs);
    void downsample_levels(int which, int npairs);
    void images_in_place(bool shared_ref);
    void motion_in_place();
    double *analysis_words();
    void ensure_quality_reference(int npairs);
    void run_jacobian(bool map);
    void run_invert(int max_iter, double tol);
    void run_quality(bool shared_ref);
    void fetch_words(double *host, int per_pair);
    // ---- the boundary copies through d_stage_: f(round) for the rounds that
    // move npairs pairs (stage_rounds), each followed by a synchronise (the
    // next round reuses the buffer); and what a round enqueues for a stack of
    // images or planar motion fields on the host and pitched fields
    template <class F>
    void for_rounds(int npairs, F f) {
        for (const StageRound &r : stage_rounds(npairs, stage_pairs_, lv_[0].stride, dimx_, dimy_)) {
            f(r);
            OF2D_HIP(hipStreamSynchronize(st_));
        }
    }
    void images_in(const StageRound &r, const double *host, float *field);
    void images_out(const StageRound &r, const float *field, double *host);
    void motion_in(const StageRound &r, const double *host, float2 *field);
    void motion_out(const StageRound &r, const float2 *field, double *host);
    // loop `loop` of level s between its two events, by the kernel that kind()
    // and placement_[s] name
    void launch_loop(int s, int loop, bool conv);
    // c and the kind's own arguments at level L
    LoopArgs hs_args(const LoopCommon &c, BLevel &L) const;
    CurvLoopArgs curv_args(const LoopCommon &c, BLevel &L) const;
    ElasticLoopArgs elastic_args(const LoopCommon &c, BLevel &L) const;
    FluidLoopArgs fluid_args(const LoopCommon &c, BLevel &L) const;
    DemonsLoopArgs demons_args(const LoopCommon &c, BLevel &L) const;
    // what the loops need of the driver follows from the kind (batch_plan.h)
    LoopKind kind() const { return loop_kind(reg_, fluid_); }
    int B_, dimx_, dimy_, nscales_, nrefine_, nloops_ = 0;
    std::vector<int> niter_, ldx_, ldy_;
    int reg_;
    std::vector<float> params_;
    float alpha_ = 0.0f;
    float tau_ = 1.0f;  // Curvature (OpticalFlowCurvature.h:8)
    SorCoef sor_{};     // Elastic: the sweep's constants of {mu, lambda, omega}
    // Demons: the two Gaussian tables (sigma_fluid, then sigma_diffusion), as
    // Registration's DemonsKernels
    std::vector<double> kfluid_, kdiff_;
    DevArray<float> d_kf_;
    DevArray<double> d_kd_;
    bool fixed_ = false, shared_ = false, have_images_ = false;
    bool diffeo_ = false;  // option "diffeomorphic" (Demons, Composition only)
    bool warm_ = false;    // option "warm_start": estimate() resets no motion
    // option "fluid" (an Elastic batch): the kind is Fluid.  The velocity
    // (BLevel::vel) and the log exist from the first estimate that runs with
    // it (prepare_fluid); the last level's is allocated last
    bool fluid_ = false;
    bool have_velocity() const { return !lv_.empty() && lv_.back().vel.base; }
    void prepare_fluid();
    void zero_velocity();
    DevArray<float> d_flog_;
    std::vector<float> h_flog_;
    // option "resident" or "conv_lds", the one a handle of this kind admits
    // (on_cu_option): the levels that fit (on_cu_fits) run launch_hs_resident
    // or launch_demons_lds.  on_cu_ok_: resident_prepare's or
    // conv_lds_prepare's answer on home_, -1 before it is asked; placement_:
    // per level, what the last estimate ran
    bool on_cu_ = false;
    int on_cu_ok_ = -1;
    std::vector<int> placement_;
    int device_ = -1, home_ = -1;
    bool ready_ = false;
    int ref_pairs_ = 0;  // images Iref holds at every level: 0, 1 (shared) or B
    hipStream_t st_ = nullptr;
    std::vector<BLevel> lv_;
    DevArray<double> d_stage_;
    // analysis: 5 doubles per pair (allocated on first use), and quality's
    // copy of the reference images (qref_pairs_ of them; the stored Iref stays
    // as set_images left it)
    DevArray<double> d_words_;
    BField<float> qref_;
    int qref_pairs_ = 0;
    size_t stage_pairs_ = 0;
    DevArray<unsigned> d_status_;
    DevArray<int> d_iters_;
    DevArray<float> d_errs_;  // allocated by the first estimate with convergence on
    int maxn_ = 0;
    std::vector<hipEvent_t> ev_;
    hipEvent_t ev_io_[2] = {};  // the caller's stream before / after the device-array launches
    int launches_ = 0;
    double loop_us_ = 0.0;
    std::vector<unsigned> h_status_;
    std::vector<int> h_iters_;
    std::vector<float> h_errs_;
    std::string pair_err_;
};

}  // namespace batch
}  // namespace of2d
