/*
 * of2d.h — C-ABI of the MI355X-native OpticalFlow2d registration library
 * (libof2d.so).  Plain pointers and sizes only; every entry point returns an
 * int status (OF2D_OK = 0) and never throws across the boundary.
 *
 * The boundary replaces the reference's MEX entry point and the operator
 * plug-in point underneath it:
 *
 *   reference                                   replaced by
 *   -----------------------------------------   ---------------------------------
 *   mexFunction (WrapperOpticalFlow2d.cpp:18-20) of2d_gateway (same 5 modes)
 *   init branch            (:23-83)              of2d_create
 *   register branch        (:86-102)             of2d_set_images + of2d_estimate
 *   get-motion branch      (:105-117)            of2d_get_motion
 *   warp branch            (:120-137)            of2d_warp
 *   close branch           (:140-147)            of2d_destroy
 *   ImageRegistration::estimate_motion
 *     (src/ImageRegistration.cpp:133-156) and every
 *     IterativeSolver::get_update
 *     (src/regularization/IterativeSolver.h:22)  of2d_estimate (device-resident)
 *   enum Regularisation/Verbose/MotionAccumulation
 *     (src/SolverOptions.h:4-8)                  OF2D_REG_* / OF2D_VERBOSE_* /
 *                                                OF2D_ACCUM_* (same values)
 *
 * Array layout at the boundary is the reference's: column-major with x fast,
 * idx = i + j*dimx (src/Field.tpp:13; MATLAB [dimx, dimy]); images are double
 * [dimx*dimy]; a motion field is planar double [dimx*dimy*2], x-plane first
 * (src/Motion.cpp:23-39).
 */
#ifndef OF2D_H
#define OF2D_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
#define OF2D_OK 0
#define OF2D_ERR_INVALID_ARGUMENT 1 /* std::invalid_argument / mexErrMsgTxt on bad input */
#define OF2D_ERR_RUNTIME 2          /* std::runtime_error, e.g. "Divide by zero exception" */
#define OF2D_ERR_DEVICE 3           /* HIP / RCCL failure */
#define OF2D_ERR_STATE 4            /* call sequence not allowed (mexErrMsgTxt :149-151) */

/* ---- SolverOptions.h:4-8, identical integer values ---- */
enum of2d_regularisation {
    OF2D_REG_DIFFUSION = 0,
    OF2D_REG_CURVATURE = 1,
    OF2D_REG_ELASTIC = 2,
    OF2D_REG_THIRIONS_DEMONS = 3,
    OF2D_REG_DIFFEOMORPHIC_DEMONS = 4,
    OF2D_REG_FLUID = 5
};
enum of2d_verbose { OF2D_VERBOSE_OFF = 0, OF2D_VERBOSE_ON = 1 };
enum of2d_motion_accumulation { OF2D_ACCUM_COMPOSITION = 0, OF2D_ACCUM_ADDITION = 1 };

typedef struct of2d_ctx of2d_ctx;

/* Text the reference prints with mexPrintf (parameter banner
 * ImageRegistration.cpp:6-47, Logger lines Logger.cpp:62-69, Fluid lines
 * OpticalFlowFluid.cpp:94, ImageRegistrationFluid.cpp:110) goes through this
 * hook; NULL restores the default (stdout).  Process-global. */
typedef void (*of2d_print_fn)(const char *text, void *user);
void of2d_set_print_hook(of2d_print_fn fn, void *user);

/* ---- registration object (replaces the init branch, :23-83) ----
 * niter has nscales+1 entries (finest level first, :35-38); regparams has
 * nparams entries whose meaning follows the reference per regularisation
 * (ImageRegistrationOpticalFlow.cpp:8-68, ImageRegistrationDemons.cpp:7-57,
 * ImageRegistrationFluid.cpp:5-36).  Invalid nparams fails with
 * OF2D_ERR_INVALID_ARGUMENT and the reference's message. */
int of2d_create(of2d_ctx **out, int dimx, int dimy, const int *niter, int nscales, int reg,
                const float *regparams, unsigned nparams, int nrefine, int verbose);
/* register branch (:86-102): images are double [dimx*dimy] */
int of2d_set_images(of2d_ctx *ctx, const double *Iref, const double *Imov);
int of2d_estimate(of2d_ctx *ctx);
/* get-motion branch (:105-117): out is double [dimx*dimy*2], planar */
int of2d_get_motion(of2d_ctx *ctx, double *out);
/* A motion from outside (not in the reference): a prior, another tool's field,
 * a coarser run's result.  motion is double [dimx*dimy*2], planar as
 * of2d_get_motion writes it; every value is cast to float and stored as given
 * (non-finite values are not looked for: the sampling kernels' behaviour for
 * them applies downstream).  It replaces the level-0 motion, so
 * of2d_get_motion, of2d_warp and the analysis entries see it at once, and,
 * when nscales >= 1, the motion of level nscales by Motion::downSample of it.
 * An estimate never resets the motion (ImageRegistration.cpp:133-156: a second
 * of2d_estimate continues from the first), so the next of2d_estimate starts
 * from the supplied field at every level: level nscales from its own motion,
 * the levels between from Motion::downSample of level 0, and level 0 itself
 * is overwritten by the upsample when nscales >= 1.  No images are needed.
 * Every regularisation takes it. */
int of2d_set_motion(of2d_ctx *ctx, const double *motion);
/* every level's motion back to zero (and Fluid's velocity, which also
 * survives an estimate): the next of2d_estimate gives a new context's bits */
int of2d_reset_motion(of2d_ctx *ctx);
/* warp branch (:120-137): out is double [dimx*dimy] */
int of2d_warp(of2d_ctx *ctx, const double *Imov, double *out);
/* close branch (:140-147) */
int of2d_destroy(of2d_ctx *ctx);
const char *of2d_last_error(const of2d_ctx *ctx);
/* iterations executed per (level, refine) of the last of2d_estimate, in
 * execution order (coarsest level first); returns the number of entries */
int of2d_iterations_executed(const of2d_ctx *ctx, int *out, int cap);
/* per-iteration Logger error (Logger.cpp:32-51) of the last loop executed */
int of2d_last_errors(const of2d_ctx *ctx, float *out, int cap);
/* Options that the reference does not have (bench / deployment only):
 *   "fixed_iters" (0/1): run every iteration, no convergence break
 *   "chunk" (>=1): iterations enqueued between host convergence checks
 *   "device" (>=0): HIP device ordinal, must be set before of2d_set_images
 *   "hs_gradients_from_image" (-1 auto = default, 0, 1): as for the slab
 *   solver (of2d_slab_set_option); bit-identical results either way
 *   "ngpus" (1 = default .. 16): Horn-Schunck levels run as that many row
 *   slabs, rank r on device (device + r) mod count, in this process (halos and
 *   the Logger's running sums cross the ranks by peer copies; the pyramid,
 *   warps and accumulation stay on the registration's device).  Results are
 *   the one-device results bit for bit with the default Logger norms.  Levels
 *   with fewer j-lines than ranks run on one device.  Ranks beyond the device
 *   count are merged (a device runs one slab of rows; splitting it only adds
 *   halo work) unless "ngpus_share" is set.
 *   "ngpus_share" (0 = default / 1): ranks may share a device, (device + r)
 *   mod count for every r < ngpus (the decomposition on fewer devices than
 *   ranks: tests, timings of the path's overhead on one GPU).
 *   "slab_split" (-1 auto = default, 0, 1): the ranks' slab option "split"
 *   (of2d_slab_set_option).
 *   "logger_fp64" (0 = default / 1): 0 computes the Logger norms as the
 *   reference does (float running sums in linear order), so the break of
 *   ImageRegistrationOpticalFlow.cpp:131-134 falls on the reference's
 *   iteration at every size; 1 sums the magnitudes in fp64 (faster: the fused
 *   multi-iteration kernels stay on; at >= 4096^2 the break can move by a few
 *   iterations).  fixed_iters runs take no break and use the fp64 sums.
 *   "curvature_dct" (0 = default / 1; anything else is refused): how
 *   Curvature evaluates its REDFT10 / REDFT01.  0: as fp64 GEMMs against dense
 *   cosine matrices, O(n^3) per iteration and n^2 doubles of tables per axis
 *   and direction.  1: as fast O(n^2 log n) line transforms on every axis of a
 *   level whose length is a power of two in [OF2D_DCT_NMIN, OF2D_DCT_NMAX];
 *   any other axis keeps its GEMM (a 64 x 37 level runs axis x fast and axis y
 *   by GEMM), and no cosine matrix is built for a fast axis.  The two agree to
 *   fp64 rounding (a different summation order); of2d_curvature_paths tells
 *   what ran.  May be changed between of2d_estimate calls.
 *   "demons_separable" (0 = default / 1; anything else is refused): how the
 *   Demons solvers smooth with their two Gaussians.  0: the reference's direct
 *   kw x kw convolution, bit for bit.  1: on every pixel whose kw x kw taps all
 *   have their linear index inside the field, a row pass along the linear
 *   index and then a column pass with the fp64 row / column marginals of the
 *   same normalised table (about 2 kw multiply-adds per pixel instead of
 *   kw^2); every other pixel (the first and last (kw-1)/2 j-lines and up to
 *   (kw-1)/2 pixels of the adjacent line) keeps the direct form bit for bit.
 *   The two differ by fp32 rounding only (1e-4 px on whole registrations,
 *   DESIGN.md 4.2).  Taken per level for every odd kw in [3, OF2D_SEP_KW_MAX]
 *   on a level with dimx >= kw; an even kw, kw = 1, kw > OF2D_SEP_KW_MAX or a
 *   narrower level runs the direct form for the whole level;
 *   of2d_demons_paths tells what ran.  May be changed between of2d_estimate
 *   calls; ignored by the other solvers. */
int of2d_set_option(of2d_ctx *ctx, const char *key, double value);
/* the widest kernel "demons_separable" takes */
#define OF2D_SEP_KW_MAX 15
/* the Demons loops of the last of2d_estimate, one per (level, refine) in
 * execution order: four ints {dimx, dimy, kw, separable} each (the level's
 * size, the kernel width and 1 when the loop smoothed with the separable
 * kernels, 0 with the direct ones), up to cap ints into out; returns the
 * number of loops (0 for another solver) */
int of2d_demons_paths(const of2d_ctx *ctx, int *out, int cap);
/* line lengths the fast transforms of "curvature_dct" take (powers of two):
 * the longest is the longest x | y line pair that fits a compute unit's LDS */
#define OF2D_DCT_NMIN 8
#define OF2D_DCT_NMAX 8192
/* the Curvature loops of the last of2d_estimate, one per (level, refine) in
 * execution order: four ints {dimx, dimy, fast_x, fast_y} each (the level's
 * size and, per axis, 1 when it ran the fast transforms, 0 the GEMMs), up to
 * cap ints into out; returns the number of loops (0 for another solver) */
int of2d_curvature_paths(const of2d_ctx *ctx, int *out, int cap);

/* ---- gateway: the process-global singleton of WrapperOpticalFlow2d.cpp:13.
 * Mode is keyed on (nlhs, nrhs, singleton present) exactly like mexFunction:
 *   init (0,8,no)  prhs = {[dimx dimy], niter, nscales, reg, regparams,
 *                          nparams, nrefine, verbose}
 *   init (0,9,no)  the same plus ngpus (of2d_set_option "ngpus"): not in the
 *                  reference, which has no multi-device mode
 *   register (0,2,yes) prhs = {Iref, Imov}
 *   get (1,0,yes)  plhs[0] = double [dimx*dimy*2]
 *   warp (1,1,yes) prhs = {Imov}, plhs[0] = double [dimx*dimy]
 *   close (0,0,yes)
 * anything else: OF2D_ERR_STATE with the reference's message (:149-151).
 * plhs buffers are caller-allocated; of2d_gateway_output_numel tells the size. */
int of2d_gateway(int nlhs, double **plhs, int nrhs, const double *const *prhs);
size_t of2d_gateway_output_numel(int nlhs, int nrhs);
int of2d_gateway_output_dims(int nlhs, int nrhs, size_t *dims, int *ndims);
const char *of2d_gateway_last_error(void);

/* ---- row-slab Horn-Schunck solver (multi-GPU north-star path) ----
 * One process per GPU.  Global grid dimx x dimy is split into contiguous slabs
 * of j-lines; rank r owns rows [row_begin, row_end) (of2d_slab_bounds).  The
 * halo (K j-lines to each neighbour before every fused launch of K = 3, 2 or 1
 * iterations) travels over RCCL, overlapped with the interior row bands.  A
 * slab needs >= 3 j-lines.
 * nranks == 1 needs no unique id (pass NULL); with one, a one-rank RCCL
 * communicator carries the Logger all-reduces (exercises RCCL on one GPU). */
int of2d_slab_bounds(int dimy, int rank, int nranks, int *row_begin, int *row_end);
int of2d_rccl_unique_id_size(void);
int of2d_rccl_get_unique_id(void *out, int len);
typedef struct of2d_slab of2d_slab;
int of2d_slab_create(of2d_slab **out, int dimx, int dimy, float alpha, int rank, int nranks,
                     int device, const void *rccl_unique_id, int id_len);
/* images: rows [row_begin-3, row_end+4) clipped to [0, dimy), double, x fast
 * (three halo rows: iterations run fused in threes, whose first step also
 * covers two halo j-lines on each side; the fourth row below: the moving image
 * is warped by the zero motion as the reference does, which reads the row
 * below every row it produces and spreads a NaN or inf pixel) */
int of2d_slab_set_images(of2d_slab *s, const double *Iref_rows, const double *Imov_rows);
/* The slab's per-run setup lives outside of2d_slab_run: set_images computes the
 * gradients and the divide-by-zero / division-range test (dI is fixed per image
 * pair), and every run ends by zeroing the buffer the next run starts from
 * (motion_est->reset(), ImageRegistrationOpticalFlow.cpp:141), enqueued behind
 * the run's end event.  of2d_slab_reserve sizes the per-iteration Logger sums
 * of a fixed_iters run of niter iterations (3000 are reserved at create), so a
 * run allocates nothing. */
int of2d_slab_reserve(of2d_slab *s, int niter);
/* runs niter Jacobi iterations (HS, Logger, convergence unless fixed_iters)
 * from zero motion (ImageRegistrationOpticalFlow.cpp:123-135); *iters_done
 * receives the iterations executed */
int of2d_slab_run(of2d_slab *s, int niter, int fixed_iters, int *iters_done);
/* owned rows of the motion, planar double [dimx*nrows*2] */
int of2d_slab_get_motion(of2d_slab *s, double *out);
/* average duration (microseconds) of one launch of the Jacobi kernel (the
 * fused kernel a fixed_iters run launches: THREE iterations per launch, or
 * FOUR where info[11] says so, over the whole slab in one launch) over
 * nlaunch launches, timed with HIP events on the stream it is
 * launched on.  The launches read the zeroed start buffer and write scratch:
 * the last run's motion (of2d_slab_get_motion) is left intact. */
int of2d_slab_time_kernel(of2d_slab *s, int nlaunch, double *avg_us);
/* slab facts for reports: info[0..11] = {nranks, ranks of the RCCL
 * communicator (ncclCommCount; 0 without one), in-process group (0/1),
 * row_begin, row_end, dimx, pitch (elements), halo j-lines exchanged per fused
 * launch, interior/edge split (0/1), triple kernel derives dI from Iaux (0/1),
 * Logger of a convergence-on run (1: the reference's float running sums,
 * 0: fp64 sums — "logger_fp64" resolved), iterations per fused launch of a
 * fixed_iters run (3, or 4: "hs_fixed_quads" resolved), "hs_quad_tail_exchange"
 * (0/1)}; returns the number of entries written */
int of2d_slab_info(const of2d_slab *s, int *info, int n);
/* the Logger errors of the last of2d_slab_run's iterations (the global ones:
 * the same on every rank), up to n into out; returns how many there are */
int of2d_slab_last_errors(const of2d_slab *s, float *out, int n);
/* wall time (ms, HIP events) of the last of2d_slab_run on this rank */
int of2d_slab_last_run_ms(const of2d_slab *s, double *ms);
/* the fused kernel's own average launch time (us) inside the last run (the
 * triple's, or the quad's in a run that launched quads: info[11]),
 * from HIP events bracketing the back-to-back fused launches of each of its
 * first 64 chunks on the solver's stream (halo exchange included for N > 1),
 * and the number of launches that average covers.  info[11] describes a
 * fixed_iters run whatever the last run was: a convergence-on run launches
 * triples even where info[11] is 4, and this average is then the triple's.
 * of2d_slab_time_kernel always launches the kernel info[11] names. */
int of2d_slab_last_run_kernel_us(const of2d_slab *s, double *avg_us, int *nlaunch);
/* the halo's cost inside the last run, sampled with HIP events on the first 8
 * split triples (interior launch beside the exchange and two edge launches):
 * us3[0] the solver stream's wait for the previous launch's edges before the
 * interior may start (the stall the halo puts on the critical stream),
 * us3[1] the exchange on the halo stream (ncclGroupStart .. ncclGroupEnd of
 * the sends / receives, or the in-process copies, including the wait for the
 * neighbours), us3[2] the two edge launches; averages per sampled launch, and
 * *nsampled the launches sampled (0 when the run had no split triples) */
int of2d_slab_last_run_halo_us(const of2d_slab *s, double *us3, int *nsampled);
/* options (no reference counterpart):
 *   "hs_fixed_quads" (1 = default, 0): a fixed_iters run of a one-rank slab
 *   that is not split and reads dI advances four iterations per launch
 *   (chunks of 25 launches) instead of three; 0 keeps the triples; the motion
 *   is bit-identical either way, the Logger errors agree to rounding
 *   "hs_quad_tail_exchange" (1 = default, 0): the wave pairs of the quad kernel
 *   exchange their end-of-band rows through LDS instead of recomputing them;
 *   0 launches the instantiation without the exchange; motion and errors are
 *   bit-identical either way
 *   "hs_gradients_from_image" (-1 auto = default, 0, 1): the triple kernel
 *   derives dI from Iaux in the kernel (24 B/px per launch) instead of reading
 *   dI (28); auto does so when dI + It (12 B/px) exceed the 256 MB MALL;
 *   bit-identical either way
 *   "logger_fp64" (-1 auto = default, 0, 1): as of2d_set_option's; 0 takes
 *   the convergence-on Logger norms as the reference does (one float running
 *   sum over the slabs in rank order, so the break falls on the one-grid
 *   reference's iteration), 1 sums the fused fp64 partials (fixed_iters runs
 *   always do); auto is 0 except on an RCCL communicator of two or more
 *   ranks, where the rank-to-rank chain of the running sums (two more
 *   communicators on two more streams) has not run on hardware: 1 there,
 *   unless 0 is set
 *   "split" (-1 auto = default, 0, 1): triples as an interior launch beside
 *   the halo exchange and two edge launches (auto: when a neighbour is on
 *   another device or behind RCCL), never, or whenever the slab has >= 48
 *   j-lines AND a halo to exchange — two or more ranks, or a one-rank
 *   communicator with "rccl_self_halo" (tests of the multi-device launch
 *   order on one device; a one-rank slab without either stays unsplit
 *   whatever is set); bit-identical either way
 *   "rccl_self_halo" (0 = default, 1; a one-rank RCCL communicator only):
 *   every halo exchange also sends the slab's boundary j-lines to rank 0
 *   itself (ncclSend / ncclRecv in a group, into a scratch buffer that is never
 *   read), and "split" 1 then splits the one-rank slab: the RCCL halo calls
 *   of an N-rank run, rehearsed on one GPU; bit-identical */
int of2d_slab_set_option(of2d_slab *s, const char *key, double value);
int of2d_slab_destroy(of2d_slab *s);
const char *of2d_slab_last_error(const of2d_slab *s);
/* In-process slab group: the nranks slabs of one grid in ONE process, driven by
 * one host thread per rank, exchanging the same halo lines and Logger sums by
 * device copies (ordered with HIP events, the threads meeting at a barrier per
 * exchange) instead of RCCL.  Same slab code and launches as the RCCL path; it
 * lets the decomposition run on a single GPU, where RCCL refuses two ranks on
 * one device (tests/test_gpu_slab_local.py).  nranks <= 16.  Create the group,
 * then one slab per rank with of2d_slab_create_local; call of2d_slab_run on all
 * ranks concurrently; destroy the slabs before the group. */
typedef struct of2d_slab_group of2d_slab_group;
int of2d_slab_group_create(of2d_slab_group **out, int nranks);
int of2d_slab_group_destroy(of2d_slab_group *g);
int of2d_slab_create_local(of2d_slab **out, int dimx, int dimy, float alpha, int rank,
                           int nranks, int device, of2d_slab_group *g);

/* ---- deformation analysis: is the registration any good? ----
 * Per-pixel passes over fields that are on the device, in the registration's
 * own layout; only the results cross the boundary.  Not in the reference's
 * interface; the Jacobian is Image::jacobian (src/Image.cpp:189-218) and the
 * composition Motion::accumulate (src/Motion.cpp:113-178), bit for bit.  Every
 * reduction runs in a fixed order: two calls on the same input give the same
 * bits.  The of2d_field_* / of2d_image_* entries take dense host arrays (an
 * image is float [dimx*dimy], idx = i + j*dimx; u is float [dimx*dimy*2], x and
 * y interleaved per pixel) and leave the message of a failure in
 * of2d_gateway_last_error; the entries on a context read its level-0 motion
 * (zero before the first of2d_estimate) and leave it untouched. */
/* J = (1 + du.x/dx) (1 + du.y/dy) - du.y/dx du.x/dy with the reference's
 * partial_x / partial_y (central differences, one-sided on the borders), the
 * number Fluid regrids on.  stats[5] = {min, max, mean, count(J <= 0) (folded
 * pixels), count(J < 0.5) (Fluid's regrid threshold)}; jac (float [dimx*dimy])
 * may be NULL: only the statistics are produced.  dimx < 2 or dimy < 2 is
 * refused with OF2D_ERR_INVALID_ARGUMENT before any device work (the one-sided
 * difference would read outside the field). */
int of2d_field_jacobian(const float *u, int dimx, int dimy, float *jac, double *stats);
/* of the registration's current level-0 motion, without leaving the device
 * except for the results; jac is double [dimx*dimy] (boundary layout) or NULL */
int of2d_jacobian(of2d_ctx *ctx, double *jac, double *stats);
/* The inverse field v with (id + u) o (id + v) = id, by the fixed-point
 * iteration v_0 = 0, r_k = accumulate(u, v_k) (= v_k + u(x + v_k), bilinear),
 * v_{k+1} = v_k - r_k, m_k = max |r_k| over pixels and components.  Where
 * floor(x + v_k) falls outside the grid r_k is 0 (v keeps its value there) and
 * the pixel is counted as out of bounds (Motion::accumulate would keep u's
 * value instead, and the iteration would run away along the border).  The
 * update is always applied; the loop stops after the first k with
 * m_k < (float)tol, or after max_iter updates.  The stop is decided on the
 * device: the host enqueues OF2D_INVERT_CHUNK updates at a time and reads the
 * report once per chunk; updates behind the stop do nothing.
 * info[4] = {iterations (updates applied), residual (m of the last one),
 * out-of-bounds pixels at the last evaluated iterate, converged 0/1};
 * residuals (optional, float[max_iter]): m_k per update applied, 0 beyond.
 * Refused with OF2D_ERR_INVALID_ARGUMENT before any device work: NULL u, v or
 * info, max_iter < 1, tol not finite or <= 0, dimx < 2 or dimy < 2.  A folded
 * field (min J <= 0) has no inverse: the call returns OF2D_OK with
 * converged = 0. */
#define OF2D_INVERT_CHUNK 8
int of2d_field_invert(const float *u, int dimx, int dimy, int max_iter, double tol, float *v,
                      double *info, float *residuals);
/* inverse of the registration's level-0 motion; out planar double like of2d_get_motion */
int of2d_invert_motion(of2d_ctx *ctx, int max_iter, double tol, double *out, double *info);
/* out[2] = {mse, ncc} of two float images [dimx*dimy]: the mean squared
 * difference and the zero-mean normalised cross-correlation, from fp64 sums
 * of a, b, a^2, b^2, ab and (a - b)^2.  ncc is NaN when either image is
 * constant (zero variance); the call still returns OF2D_OK. */
int of2d_image_similarity(const float *a, const float *b, int dimx, int dimy, double *out);
/* Iref against Imov and against warp2d(Imov, motion) (images as of2d_warp's):
 * out[4] = {mse_before, ncc_before, mse_after, ncc_after}; the warp is the one
 * of2d_warp takes, on the device */
int of2d_quality(of2d_ctx *ctx, const double *Iref, const double *Imov, double *out);

/* ---- batched Horn-Schunck and Thirion's Demons: many small pairs of one
 * size in one call ----
 * (Curvature, Elastic and Fluid: their own paragraphs below.)
 * nbatch independent registrations with the same parameters, reg =
 * OF2D_REG_DIFFUSION (regparams = {alpha}) or OF2D_REG_THIRIONS_DEMONS
 * (regparams = {sigma_i, sigma_x, sigma_diffusion, sigma_fluid, kernel_width,
 * accumulation}, of2d_create's six: Composition 0 or Addition 1, any other
 * value leaves the motion without the correction as of2d_create does; any
 * kernel_width >= 1, even and wider than the image included).  Each
 * pair is run by one workgroup with the whole iteration loop inside the
 * kernel; the passes around the loop (pyramid, warp, gradients, composition)
 * take the pair as a grid dimension, so the kernel launches of one estimate do
 * not depend on nbatch.  (Demons has no gradients pass: its loop warps the
 * moving image by the iterate and differentiates it in every iteration.)  The pyramid and refine sequence, the per-pixel
 * arithmetic and therefore the motion of every pair are those of of2d_create /
 * of2d_estimate on that pair alone (a new context's first estimate: every
 * of2d_batch_estimate starts from a zero motion field, unless "warm_start" is
 * 1), bit for bit when the pair runs the same number of iterations.
 *
 * Convergence (the default; "fixed_iters" 0): each pair stops on its own
 * iteration by the reference's test (error < 0.001f after iteration > 1).  The
 * error is formed with the Logger's float arithmetic from fp64 sums added in a
 * fixed order: the semantics of of2d_set_option "logger_fp64" = 1, not the
 * reference's sequential float sum; two calls give the same bits.  With
 * "fixed_iters" 1 every loop runs niter iterations and no error is recorded.
 *
 * A zero denominator on an image pixel (the reference's "Divide by zero
 * exception") is per pair: of2d_batch_estimate still returns OF2D_OK,
 * of2d_batch_status reports OF2D_ERR_RUNTIME for that pair, its motion is left
 * zero and of2d_batch_last_error names the first such pair.
 *
 * of2d_batch_create refuses with OF2D_ERR_INVALID_ARGUMENT and a message
 * (of2d_batch_last_error(NULL)), before any device work: nbatch < 1 or > 65535,
 * a reg other than OF2D_REG_DIFFUSION, OF2D_REG_CURVATURE, OF2D_REG_ELASTIC and
 * OF2D_REG_THIRIONS_DEMONS, a Curvature batch with a pyramid level whose side
 * is not a power of two in [OF2D_DCT_NMIN, OF2D_BATCH_CURV_NMAX] and an Elastic
 * batch with nparams != 3 (the same sentence as for a refused method: it names
 * the four and their rules, and points to the option "fluid"), nparams
 * != 1 (Diffusion), != 1 and != 2 (Curvature) or != 6 (Demons; the reference's
 * message), a Demons kernel_width < 1 (of2d_create's message),
 * dimx * dimy > OF2D_BATCH_MAXPX, the sizes of2d_create refuses, NULL arrays.
 * Options: "fixed_iters", "device" (before first use), "diffeomorphic",
 * "fluid", "warm_start", "resident", "conv_lds"; an
 * unknown key is refused ("demons_separable" among them: the batch smooths
 * with the direct convolution only).
 *
 * Curvature (reg = OF2D_REG_CURVATURE, regparams = {alpha} with tau = 1, or
 * {alpha, tau}): every pyramid level (dimx / 2^s, dimy / 2^s) must have both
 * sides a power of two in [OF2D_DCT_NMIN, OF2D_BATCH_CURV_NMAX], so a 64 x 32
 * batch takes nscales <= 2; the other sizes (the one-pair path's GEMMs) are not
 * offered.  One workgroup runs a pair's whole loop: per iteration the right-hand
 * side, the four line-transform passes of the one-pair "curvature_dct" = 1 path
 * (axis y then x, forward with the eigenvalues, then inverse) and the update,
 * the fp64 plane pair in a per-pair scratch of 16 bytes per pixel and level.
 * With "fixed_iters" 1 every pair's motion, warp and iteration counts are those
 * of of2d_create(reg 1) with "curvature_dct" 1 and "fixed_iters" 1 on that pair
 * alone, bit for bit.  Curvature has no zero denominator: every pair's status is
 * OF2D_OK.  "fixed_iters", "device" and "warm_start" apply; "resident",
 * "conv_lds" and "diffeomorphic" are refused as on any batch of another method.
 * of2d_batch_info reports placement 0 at every level, 512 threads, and the
 * launches of a Diffusion batch (4 per loop).
 *
 * Elastic (reg = OF2D_REG_ELASTIC, regparams = {mu, lambda, omega}, nparams =
 * 3): at every size the batch takes, with no rule of its own (a level with a
 * side below 3 has no interior pixel and its sweep changes nothing, as in the
 * one-pair path).  One workgroup runs a pair's whole loop of
 * OpticalFlowElastic::get_update: per iteration the force into a per-pair
 * scratch field, and the SOR sweep in place in the reference's order (column
 * after column, row after row within a column), run as the wavefront 2 i + j =
 * t with one thread per column and one workgroup barrier per step, none at a
 * level of 64 columns or fewer.  With "fixed_iters" 1 every pair's motion, warp
 * and iteration counts are those of of2d_create(reg 2) with "fixed_iters" 1 on
 * that pair alone, bit for bit.  of2d_create's two-parameter form {mu, lambda}
 * (omega = 0.66f, OpticalFlowElastic.h:9) stays refused here, with the sentence
 * that refuses a method: the batch has refused reg 2 with two parameters by
 * that sentence since it exists, and a caller writes the third one out
 * (opticalflow2d_amd.BatchRegistration appends it).  Elastic has no division:
 * every pair's status is OF2D_OK.  "fixed_iters", "device" and "warm_start"
 * apply; "resident", "conv_lds" and "diffeomorphic" are refused as on any batch
 * of another method.  of2d_batch_info reports placement 0 at every level, per
 * level min(roundup(dx, 64), 512) threads, and the launches of a Diffusion
 * batch (4 per loop).  reg = OF2D_REG_FLUID and OF2D_REG_DIFFEOMORPHIC_DEMONS
 * stay refused at create: each is an option of the batch whose parameters and
 * loop it shares, "fluid" of an Elastic batch and "diffeomorphic" of a
 * Thirion's Demons batch (below).
 *
 * "fluid" (0, the default, or 1): viscous fluid.  With 1, a batch created with
 * reg = OF2D_REG_ELASTIC is per pair the one-pair of2d_create(OF2D_REG_FLUID,
 * {mu, lambda, omega}) registration (omega = 0.66f is OpticalFlowFluid.h:10's
 * default as it is Elastic's): ImageRegistrationFluid::
 * estimate_motion_at_current_resolution with OpticalFlowFluid::get_update.  One
 * workgroup runs the pair's whole loop: per iteration the force, the Elastic
 * batch's SOR sweep on the pair's velocity, the increment with its maximum,
 * the time step dt = 0.65f / maxabs, the integration (skipped where dt >=
 * 65), the Logger sums, the minimum Jacobian of the new estimate, and, where
 * that is below 0.5f, the regrid (the motion accumulates the estimate, the
 * moving image is warped again and differentiated, the next iteration starts
 * from a zero estimate) inside the kernel.  With "fixed_iters" 1 every pair's
 * motion, warp, iteration counts and Dumax / Regridding record are those of
 * that pair alone on the one-pair path, bit for bit; the break is off and the
 * regrid stays on.  The next of2d_batch_estimate takes the value; with 0 the
 * batch is the Elastic batch, bit for bit.  Fluid has no division: every
 * pair's status is OF2D_OK.  "fixed_iters", "warm_start" and "device" compose
 * with it; "resident", "conv_lds" and "diffeomorphic" stay refused as on any
 * Elastic batch; of2d_batch_info reports what an Elastic batch reports.
 * The velocity is a field per pair and pyramid level that outlives an
 * estimate, as OpticalFlowFluid::velocity does: allocated by the first
 * estimate that runs with "fluid" 1 (8 bytes per pixel, pair and level),
 * carried across the refines of a level, zeroed at the start of every estimate
 * with "warm_start" 0 (a fresh handle's bits) and carried over with
 * "warm_start" 1 (a reused one-pair context, bit for bit), zeroed by
 * of2d_batch_reset_motion and by a change of the option's value.
 * of2d_batch_set_motion leaves it as it is, as of2d_set_motion does on the
 * one-pair path (only of2d_reset_motion touches the velocity there).
 * The batch prints nothing; the reference's lines are the record
 * of2d_batch_fluid_log returns (below).
 * Refused with OF2D_ERR_INVALID_ARGUMENT, the handle still usable and the
 * option unchanged: on a batch of another method ("fluid: the batch is not an
 * Elastic batch"), for a value other than 0 or 1 ("fluid: the value must be 0
 * or 1"), and when a pyramid level has a side below 2 ("fluid: every level
 * needs sides of at least 2": the Jacobian's one-sided differences need a
 * neighbour).
 *
 * "diffeomorphic" (0, the default, or 1): Diffeomorphic Demons.  With 1, a
 * batch created with reg = OF2D_REG_THIRIONS_DEMONS and accumulation 0
 * (Composition) is per pair the one-pair OF2D_REG_DIFFEOMORPHIC_DEMONS
 * registration with parameters [sigma_i, sigma_x, sigma_diffusion,
 * sigma_fluid, kernel_width]: the smoothed correction goes through
 * Motion::exp (scaling and squaring) before it is composed with the motion.
 * Each pair takes its own number of squarings in every iteration, the
 * reference's; there is no bound on it and no status for one.  The next
 * of2d_batch_estimate takes the value; 0 is Thirion's Demons bit for bit.
 * Refused with OF2D_ERR_INVALID_ARGUMENT, the handle still usable and the
 * option unchanged: on a batch of another method ("diffeomorphic: the batch is
 * not a Thirion's Demons batch"), with another accumulation ("diffeomorphic:
 * accumulation must be Composition (0)"), and for a value other than 0 or 1.
 * (reg = OF2D_REG_DIFFEOMORPHIC_DEMONS itself stays refused at create.)
 *
 * "warm_start" (0, the default, or 1), every method; the next
 * of2d_batch_estimate takes the value.  With 0 every estimate starts every
 * pair from zero motion.  With 1 an estimate resets no motion: per pair it is
 * of2d_estimate on a reused context (ImageRegistration::estimate_motion on a
 * reused object), bit for bit, with the reference's carry-over rule: level
 * nscales is never downsampled into and continues from its own motion of the
 * previous call; the levels between are downsampled from level 0; level 0 is
 * overwritten by the upsample whenever nscales >= 1.  So with a pyramid only
 * the coarsest level's motion carries over; to continue from the
 * full-resolution result at every level, hand it back first:
 * of2d_batch_get_motion_device then of2d_batch_set_motion_device (below).
 * A pair that fails (zero denominator) under warm_start has its motion zeroed
 * at every level, so its next estimate starts as a fresh handle's (the
 * one-pair context keeps the failed level's motion instead).  The status,
 * iteration counts and errors are per call either way.  The launches of an
 * estimate (of2d_batch_info) are max(nscales - 1, 0) + loops * (4, Demons 3)
 * + nscales + 1; with warm_start the last term, the zeroing of failed pairs,
 * is nscales + 1, one per level.  A value other than 0 or 1 is refused with
 * "warm_start: the value must be 0 or 1", the option unchanged.
 *
 * "resident" (0, the default, or 1), Diffusion batches; set before or after
 * the device is in use, the next of2d_batch_estimate takes the value.  With 1
 * every pyramid level that fits runs the Horn-Schunck loop with the pair's
 * iterate in the compute unit's LDS and dI, It in registers across all
 * iterations of the loop, instead of moving them through global memory in
 * every iteration; the other levels run the global-memory loop.  A level
 * (dx, dy) fits when (dx + 2) * (dy + 2) * 8 + 1024 bytes are within the
 * 160 KiB of LDS and dx * dy <= 16 * 1024 (16 pixels for each of the
 * workgroup's 1024 threads): every level up to 128 x 128 does.  Motion, warp,
 * iteration counts, errors and the per-pair divide-by-zero status are those of
 * 0, bit for bit; the launches of an estimate are the same; of2d_batch_info
 * reports placement 1 for the levels that ran so.  Should the runtime refuse
 * the kernel its LDS, every level runs as with 0 (placement 0) and nothing is
 * reported as an error.  Composes with "fixed_iters", "warm_start" and
 * "device".  Refused with OF2D_ERR_INVALID_ARGUMENT, the handle still usable
 * and the option unchanged: on a Demons, Curvature or Elastic batch ("resident: the batch is not a
 * Diffusion batch") and for a value other than 0 or 1 ("resident: the value
 * must be 0 or 1").
 *
 * "conv_lds" (0, the default, or 1), Thirion's Demons batches; set before or
 * after the device is in use, the next of2d_batch_estimate takes the value.
 * With 1 every pyramid level that fits runs the Demons loop with the field its
 * two Gaussian convolutions read (the correction, then the motion before the
 * last smoothing; with "diffeomorphic" every squaring of exp() as well) in the
 * compute unit's LDS instead of global memory; the other levels run the
 * global-memory loop.  A level (dx, dy) fits when (dx * dy + dx + 1) * 8 + 1024
 * bytes are within the 160 KiB of LDS and dx * dy <= 16 * 1024 (16 pixels for
 * each of the workgroup's 1024 threads): every level up to 128 x 128 does.
 * Motion, warp, iteration counts, errors and the per-pair divide-by-zero
 * status are those of 0, bit for bit; the launches of an estimate are the
 * same; of2d_batch_info reports placement 1 for the levels that ran so.
 * Should the runtime refuse the kernel its LDS, every level runs as with 0
 * (placement 0) and nothing is reported as an error.  Composes with
 * "fixed_iters", "warm_start", "device" and "diffeomorphic".  Refused with
 * OF2D_ERR_INVALID_ARGUMENT, the handle still usable and the option
 * unchanged: on a Diffusion, Curvature or Elastic batch ("conv_lds: the batch is not a Thirion's
 * Demons batch") and for a value other than 0 or 1 ("conv_lds: the value must
 * be 0 or 1").
 *
 * Splitting one pair over several workgroups is not offered: with
 * fewer pairs than compute units most of the device idles. */
typedef struct of2d_batch of2d_batch;
#define OF2D_BATCH_MAXPX (512 * 512)
/* the longest side of a Curvature batch's levels */
#define OF2D_BATCH_CURV_NMAX 512
int of2d_batch_create(of2d_batch **out, int nbatch, int dimx, int dimy, const int *niter,
                      int nscales, int reg, const float *regparams, unsigned nparams,
                      int nrefine);
int of2d_batch_set_option(of2d_batch *b, const char *key, double value);
/* Iref: nbatch images, or ONE image every pair is registered to (shared_ref =
 * 1); Imov: nbatch images; double [dimx*dimy] each, boundary layout */
int of2d_batch_set_images(of2d_batch *b, const double *Iref, int shared_ref, const double *Imov);
int of2d_batch_estimate(of2d_batch *b);
/* nbatch x planar [dimx*dimy*2], as of2d_get_motion per pair */
int of2d_batch_get_motion(of2d_batch *b, double *out);
/* of2d_set_motion per pair: motion is nbatch x planar [dimx*dimy*2], the
 * layout of2d_batch_get_motion writes (set(get()) is the identity on the
 * bits).  Level 0's motion, and with nscales >= 1 level nscales's by
 * Motion::downSample of it.  of2d_batch_get_motion, _warp and the analysis
 * entries see the field at once, so they also serve a field the batch did not
 * estimate.  The next of2d_batch_estimate starts from it at every level with
 * "warm_start" 1 and ignores it with 0.  No images are needed; the status of
 * the last estimate stays. */
int of2d_batch_set_motion(of2d_batch *b, const double *motion);
/* every level's motion back to zero, and with it the velocity of option
 * "fluid": the next estimate, warm or not, gives a fresh handle's bits */
int of2d_batch_reset_motion(of2d_batch *b);
/* pair k's image (Imov: nbatch images) warped by pair k's motion */
int of2d_batch_warp(of2d_batch *b, const double *Imov, double *out);
/* out[nbatch]: OF2D_OK or OF2D_ERR_RUNTIME per pair of the last estimate */
int of2d_batch_status(const of2d_batch *b, int *out);
/* iterations run, [pair][loop] with the (nscales + 1) * nrefine loops in
 * execution order; returns nbatch * loops */
int of2d_batch_iterations(const of2d_batch *b, int *out, int cap);
/* the errors of the pair's last loop (none with "fixed_iters"); returns their count */
int of2d_batch_last_errors(const of2d_batch *b, int pair, float *out, int cap);
/* option "fluid": one record {maxabs, dt, jmin, regridded (0 or 1)} per
 * iteration that pair's loop `loop` ran in the last estimate (loops in
 * execution order, as of2d_batch_iterations'), up to cap records (4 floats
 * each) into out; returns the number of records, 0 on a batch without "fluid"
 * or before an estimate, -1 for a pair or loop outside the batch.  The
 * reference prints "Dumax: 0.650\tMaxabs increment: maxabs\t Timestep: dt" per
 * iteration and, after an iteration that regridded, "Regridding on iteration:
 * it\tMin Jacobian: jmin".  The device buffer behind it is nbatch * loops *
 * max(niter) records of 16 bytes and exists only with "fluid" 1. */
int of2d_batch_fluid_log(const of2d_batch *b, int pair, int loop, float *out, int cap);
/* info = {kernel launches of the last estimate, loops per pair, levels, device
 * time of the last estimate's loop kernels in microseconds, then per level from
 * level 0: the placement in the last estimate (0: global memory; 1: on the
 * compute unit, the iterate with option "resident", the convolved field with
 * option "conv_lds"; 0 before the first estimate),
 * threads of a pair's workgroup}; returns the number of values */
int of2d_batch_info(const of2d_batch *b, int *info, int n);
/* Deformation analysis of every pair's level-0 motion (of2d_jacobian,
 * of2d_invert_motion and of2d_quality per pair): one or two kernel launches
 * whatever nbatch is, one workgroup per pair, every fp64 sum in a fixed order
 * (two calls give the same bits).  The maps and the inverse are those of the
 * one-pair entries on that pair alone, bit for bit; a pair's mean, mse and ncc
 * are fp64 sums in another order than the one-pair kernels' and agree with
 * them to the sums' rounding.  The motion is zero before the first estimate
 * and for a pair whose status is OF2D_ERR_RUNTIME: such a pair reports J = 1
 * everywhere, a zero inverse that converged at its first update, and
 * after == before; there is no special case for it.  The statistics, info and
 * quality are small (5, 4 and 4 doubles per pair) and always return to host
 * memory, so these calls (their _device forms too) wait for the library's
 * stream.  They leave the stored images and the motion as they are: a later
 * of2d_batch_estimate gives the bits it would have given without them.
 * Refused with OF2D_ERR_INVALID_ARGUMENT and a message before any device
 * work: NULL stats, info or out (of of2d_batch_quality; the others' maps are
 * optional), NULL Iref or Imov, max_iter < 1, tol not finite or <= 0, and for
 * the Jacobian and the inverse dimx < 2 or dimy < 2.
 *
 * jac: nbatch x [dimx*dimy] (boundary layout) or NULL; stats: nbatch x 5 as
 * of2d_jacobian's */
int of2d_batch_jacobian(of2d_batch *b, double *jac, double *stats);
/* every pair runs the loop of of2d_invert_motion inside the kernel and stops
 * on its own update (OF2D_INVERT_CHUNK plays no part).  out: nbatch x planar
 * [dimx*dimy*2] as of2d_batch_get_motion's, or NULL; info: nbatch x 4 as
 * of2d_invert_motion's */
int of2d_batch_invert_motion(of2d_batch *b, int max_iter, double tol, double *out, double *info);
/* Iref (one image with shared_ref, else nbatch) and Imov as
 * of2d_batch_set_images takes them; out: nbatch x {mse_before, ncc_before,
 * mse_after, ncc_after} */
int of2d_batch_quality(of2d_batch *b, const double *Iref, int shared_ref, const double *Imov,
                       double *out);
int of2d_batch_destroy(of2d_batch *b);
/* b == NULL: the message of the last refused of2d_batch_create of this thread */
const char *of2d_batch_last_error(const of2d_batch *b);

/* ---- device-resident I/O: images in, motion and warped images out, as
 * arrays that already live on the context's device ----
 * An of2d_darray describes a strided device array of float or double by its
 * element strides on the axes pair, x, y, component.  An entry looks only at
 * the axes its array has (an image of a context: x and y; a stack of a batch:
 * pair, x, y; a motion: also the component, x then y).  Pixel (i, j) of pair
 * k, component c, is ptr[k*stride[0] + i*stride[1] + j*stride[2] +
 * c*stride[3]]; every offset is computed in 64 bits.  The boundary layout of
 * the host entries is stride = {dimx*dimy, 1, dimx, 0} for an image and
 * {2*dimx*dimy, 1, dimx, dimx*dimy} for a motion; a contiguous [dimx][dimy]
 * array (C order) is {dimx*dimy, dimy, 1, 0}, a [dimx][dimy][2] motion
 * {2*dimx*dimy, 2*dimy, 2, 1}.  Both are moved with coalesced accesses on both
 * sides (the second through a transposing tile); any other strides are
 * correct.  An input may repeat elements (a stride of 0 reads one image for
 * every pair); an output's elements must be distinct.
 *
 * Values: an input's (float) in[...] is Image::set_image's conversion for
 * double and the value itself for float; an output receives the field's float
 * or its (double) widening.  So a double array gives and receives exactly what
 * the host entries do, bit for bit.
 *
 * Stream contract.  `stream` is the caller's hipStream_t (NULL: the null
 * stream).  The library works on non-blocking streams of its own, so on entry
 * it records an event on `stream` and makes its stream wait for it: work the
 * caller enqueued on `stream` before the call (filling an input, the last
 * reader of an output) is finished before the library touches the arrays.
 * After its last kernel that touches the caller's arrays it records an event
 * on its stream and makes `stream` wait for it: the caller may reuse or free
 * the arrays in stream order as soon as the call returns, and work enqueued on
 * `stream` afterwards sees the results without a host synchronise.  The calls
 * may still synchronise internally where their host counterparts do
 * (of2d_set_images_device and of2d_warp_device wait for their own stream), and
 * they are not for use while `stream` is being captured into a graph.
 *
 * Refused with OF2D_ERR_INVALID_ARGUMENT and a message, before any device
 * work: a NULL of2d_darray or ptr, a dtype other than OF2D_F32 / OF2D_F64, a
 * negative stride, and for an output a zero stride on an axis of extent > 1.
 * Once the device is known (first use), a ptr that hipPointerGetAttributes
 * does not place on the context's device is refused the same way. */
#define OF2D_F32 0
#define OF2D_F64 1
typedef struct of2d_darray {
    void *ptr;           /* device pointer on the context's device */
    int dtype;           /* OF2D_F32 | OF2D_F64 */
    long long stride[4]; /* element strides: pair, x, y, component (unused ones ignored) */
} of2d_darray;
/* of2d_set_images, of2d_get_motion, of2d_warp on device arrays; everything
 * after the level-0 images are in place is the host entries' code */
int of2d_set_images_device(of2d_ctx *ctx, const of2d_darray *Iref, const of2d_darray *Imov,
                           void *stream);
int of2d_get_motion_device(of2d_ctx *ctx, const of2d_darray *out, void *stream);
int of2d_warp_device(of2d_ctx *ctx, const of2d_darray *Imov, const of2d_darray *out,
                     void *stream);
/* of2d_set_motion / of2d_batch_set_motion from a device array with the axes
 * (pair,) x, y, component, validated as of2d_get_motion_device's out is (an
 * input: strides of 0 are allowed).  One launch packs all nbatch fields; the
 * library's stream waits for `stream` and `stream` waits for the pack, and the
 * calls wait for their own stream as of2d_set_images_device does. */
int of2d_set_motion_device(of2d_ctx *ctx, const of2d_darray *motion, void *stream);
int of2d_batch_set_motion_device(of2d_batch *b, const of2d_darray *motion, void *stream);
/* of2d_batch_set_images, _get_motion, _warp on device arrays: one launch moves
 * all nbatch pairs, without the host entries' staging rounds.  With shared_ref
 * Iref is one image and its pair stride is ignored. */
int of2d_batch_set_images_device(of2d_batch *b, const of2d_darray *Iref, int shared_ref,
                                 const of2d_darray *Imov, void *stream);
int of2d_batch_get_motion_device(of2d_batch *b, const of2d_darray *out, void *stream);
int of2d_batch_warp_device(of2d_batch *b, const of2d_darray *Imov, const of2d_darray *out,
                           void *stream);
/* of2d_batch_jacobian, _invert_motion, _quality with the maps, the inverse and
 * the images as device arrays (jac: pair, x, y, or NULL; out: pair, x, y,
 * component; Iref, Imov as of2d_batch_set_images_device's).  stats, info and
 * out of the quality are host memory: the calls wait for the library's stream
 * after ordering the caller's stream behind their last use of its arrays. */
int of2d_batch_jacobian_device(of2d_batch *b, const of2d_darray *jac, double *stats,
                               void *stream);
int of2d_batch_invert_motion_device(of2d_batch *b, int max_iter, double tol,
                                    const of2d_darray *out, double *info, void *stream);
int of2d_batch_quality_device(of2d_batch *b, const of2d_darray *Iref, int shared_ref,
                              const of2d_darray *Imov, double *out, void *stream);

/* ---- library info ---- */
const char *of2d_version(void);
int of2d_device_count(int *count);

#ifdef __cplusplus
}
#endif
#endif
