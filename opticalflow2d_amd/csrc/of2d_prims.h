/*
 * of2d_prims.h — the test and diagnostic entries of libof2d.so: one launch (or
 * one timing loop) per kernel, for the test suites and the tools.  Not part of
 * the drop-in contract (include/of2d.h) and not installed with it; the same
 * library exports them (capi_prims.cpp).  The status codes are of2d.h's; a
 * failure's message is read with of2d_gateway_last_error.
 */
#ifndef OF2D_PRIMS_H
#define OF2D_PRIMS_H

#include "../../include/of2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- kernel-level test entry: the Logger's norms ----
 * Motion::norm (src/Motion.cpp:42-49) as Logger::update_error (src/Logger.cpp:
 * 32-51) takes it: the float running sums, in linear order, of
 * sqrt((double)x^2 + (double)y^2) over (cur - prev) -> sums[2k] and over prev
 * -> sums[2k+1] (not divided by dimx*dimy), bit-identical to the reference's.
 * cur / prev: npairs host fields of float [dimx*dimy*2] each, interleaved x, y
 * per pixel (coord2d), idx = i + j*dimx; the pairs run in order on one
 * workspace, so pair k's walk predicts pair k+1's, as in a Logger loop.
 * stats (optional, int[8*npairs], cost figures, not results): per pair the
 * tiles the device walk resolved below tile level (|cur - prev|, |prev|), the
 * 64-term segments it stepped term by term (same order), the tiles whose
 * entries were recomputed, the walk's wall-clock ticks at 100 MHz (same
 * order) and those of the |cur - prev| walk's resolves. */
int of2d_motion_norms(const float *cur, const float *prev, int dimx, int dimy, int npairs,
                      float *sums, int *stats);
/* The Logger norms of a chain of iterates u[0 .. niter] (niter + 1 fields of
 * dimx*dimy*2 floats): sums[2k], sums[2k + 1] are those of the update from
 * u[k] to u[k + 1], as of2d_motion_norms gives them, computed the way the
 * registration loop batches them: `batch` (1..3) consecutive updates per
 * batch, whose pass reads each iterate once, on four sets of workspaces in
 * rotation (batch g's profile is batch g - 4's, Registration::kSeqSets).  The
 * launches run in order on one stream: the sums match the registration's,
 * its stream schedule (walks on three streams, the stop word) is not
 * reproduced.  stats as of2d_motion_norms, per update.  Not in the
 * reference: a test entry for the batched device norms. */
int of2d_motion_norms_chain(const float *u, int dimx, int dimy, int niter, int batch,
                            float *sums, int *stats);

/* ---- kernel-level test entry: Curvature's 2-D transforms ----
 * The separable REDFT10 (kind 10) or REDFT01 (kind 1) of a dense host array a
 * (double, idx = i + j*dimx), in place: exactly the device transforms one
 * Curvature iteration runs at a level of that size (axis y, then axis x; no
 * eigenvalues).  method 0 runs the GEMMs, 1 the fast line transforms on every
 * axis that qualifies ("curvature_dct") and the GEMM on any other; paths[0],
 * paths[1] receive what axis x and axis y ran (1 fast, 0 GEMM). */
int of2d_dct2d(double *a, int dimx, int dimy, int kind, int method, int *paths);
/* average duration (microseconds, HIP events around nlaunch back-to-back
 * launches after one untimed launch) of the fast path's passes over the plane
 * pair of a dimx x dimy level (both lengths must qualify): us[0] the forward
 * line pass along x with the eigenvalues, us[1] the inverse line pass along x,
 * us[2] one transposition, us[3] the forward line pass along y on the
 * transposed copy.  Every pass reads and writes 16 B per pixel.  A timing
 * entry for tools/curvature_bench.py, not a result. */
int of2d_dct_time_passes(int dimx, int dimy, int nlaunch, double *us);

/* ---- test and diagnostic entries: one launch of a field / Demons primitive ----
 * Each entry uploads dense host arrays into pitched device fields, makes one
 * call of the launch function the solvers call, and copies the result back.
 * Images are float [dimx*dimy], idx = i + j*dimx; motion fields are float
 * [dimx*dimy*2], x and y interleaved per pixel (coord2d).  Errors are reported
 * as by of2d_dct2d (of2d_gateway_last_error).  Not in the reference. */
/* Image::warp2d of src by u */
int of2d_prim_warp(const float *src, const float *u, int dimx, int dimy, float *out);
/* Motion::accumulate: out(x) = v(x) + m_old(x + v(x)) */
int of2d_prim_accumulate(const float *m_old, const float *v, int dimx, int dimy, float *out);
/* Fluid's regrid: m_new = accumulate(m_old, est), est0 = 0 (the device buffer
 * holds est before the launch), Iaux = warp2d(Imov, m_new) */
int of2d_prim_regrid(const float *m_old, const float *est, const float *Imov, int dimx, int dimy,
                     float *m_new, float *est0, float *Iaux);
/* accumulate onto a zero motion, for rows [row0, row0 + nrows) of a dimy-row
 * grid: v and out hold those nrows rows only */
int of2d_prim_compose_zero(const float *v, int dimx, int nrows, int row0, int dimy, float *out);
/* Field::operator+= */
int of2d_prim_add_motion(const float *a, const float *b, int dimx, int dimy, float *out);
/* what 0: Image::downSample, 1: Motion::downSample, 2: Motion::upSample from
 * dxi x dyi to dxo x dyo.  out is in/out: a pixel with no valid tap keeps the
 * value the caller put there. */
int of2d_prim_resample(int what, const float *in, int dxi, int dyi, float *out, int dxo, int dyo);
/* IterativeSolver::set_derivatives in the slab form: dI and It of rows [row0,
 * row0 + nrows) of the dimx x dimy images Iref and Iaux (whole images in, nrows
 * rows out; the device slab holds those rows and one ghost row either side) */
int of2d_prim_gradients(const float *Iref, const float *Iaux, int dimx, int dimy, int row0,
                        int nrows, float *dI, float *It);
/* Demons' correspondence force of Imov warped by u against Iref; *status
 * receives the kernels' status word (bit 0: a zero denominator) */
int of2d_prim_demons_force(const float *Iref, const float *Imov, const float *u, int dimx,
                           int dimy, float sigma_i, float sigma_x, float *corr,
                           unsigned *status);
/* The three launches below take the smoothing to run: method 0 the direct
 * convolution, 1 the separable one where "demons_separable" would take it
 * (of2d_set_option) and the direct one elsewhere; *path: 1 when the separable
 * kernels ran, 0 the direct ones.  Another method is refused before any
 * device work. */
/* corr smoothed by the kw x kw Gaussian of `sigma` (Kernel::set_gaussian), then
 * mode 0: accumulate(u, .), 1: u + ., 2: u, 3: the smoothed corr itself.
 * *wfull (optional): the kernel's full weight sum as the launch receives it. */
int of2d_prim_smooth_compose(const float *corr, const float *u, int dimx, int dimy, int kw,
                             float sigma, int mode, float *out, double *wfull, int method,
                             int *path);
/* out = umid smoothed; sums (optional, double[2]): the fp64 Logger sums
 * sum |out - prev|, sum |prev| of the launch's block partials.  Without sums
 * the launch is the one of the default Logger mode (no partials). */
int of2d_prim_smooth_norm(const float *umid, const float *prev, int dimx, int dimy, int kw,
                          float sigma, float *out, double *sums, int method, int *path);
/* one Demons correction update (force, sigma_fluid smoothing, motion update by
 * `mode` as of2d_prim_smooth_compose): the fused kernel where the solver
 * would take it, the unfused pair elsewhere */
int of2d_prim_demons_update(const float *Iref, const float *Imov, const float *u, int dimx,
                            int dimy, float sigma_i, float sigma_x, int kw, float sigma_fluid,
                            int mode, float *out, unsigned *status, int method, int *path);
/* Motion::exp of f, in place, with the squaring bound the diffeomorphic loop
 * derives from sigma_i / sigma_x (32 when their ratio is 0 or not finite);
 * *nsq: the squarings the device counted, *status bit 1: above the bound */
int of2d_prim_motion_exp(float *f, int dimx, int dimy, float sigma_i, float sigma_x, int *nsq,
                         unsigned *status);
/* the boundary copies: Image::set_image, Image::copy_image_to_input,
 * Motion::copy_motion_to_input (planar double [2*dimx*dimy], x plane first) */
int of2d_prim_d2f(const double *in, int dimx, int dimy, float *out);
int of2d_prim_f2d(const float *in, int dimx, int dimy, double *out);
int of2d_prim_motion_to_planar(const float *m, int dimx, int dimy, double *out);

/* ---- test and diagnostic entries: Curvature, one call each ----
 * One call of the function the Curvature loop calls, on a bare level of that
 * size (as of2d_dct2d).  Planes are dense double [dimx*dimy], idx = i + j*dimx;
 * method as of2d_dct2d.  Bad arguments are refused before any device work. */
/* the rhs kernel: out = u - tau * f, f the optical flow force of (u, dI, It),
 * in float, widened; out_x, out_y the two planes */
int of2d_prim_curv_rhs(const float *u, const float *dI, const float *It, float tau, int dimx,
                       int dimy, double *out_x, double *out_y);
/* the eigenvalue table the level is built with, out[p + q*dimx] = E(p, q) */
int of2d_prim_curv_eigen(int dimx, int dimy, float alpha, float tau, int method, double *out);
/* of2d_dct2d on the plane pair ax | ay, in place: both planes go through the
 * one transform call of an iteration.  with_eig 1 (kind 10 only, as in the
 * solver) multiplies by the eigenvalues of (alpha, tau) in the axis-x pass. */
int of2d_prim_curv_dct2d(double *ax, double *ay, int dimx, int dimy, int kind, int method,
                         int with_eig, float alpha, float tau, int *paths);
/* the construct kernel: out = (float)z / div per component, and sums[0] =
 * sum |out - u|, sums[1] = sum |u|: the launch's per-block Logger partials
 * added in block order on the host */
int of2d_prim_curv_construct(const double *zx, const double *zy, const float *u, float div,
                             int dimx, int dimy, float *out, double *sums);

/* ---- test and diagnostic entries: the SOR sweep, Fluid and Elastic, per launch ----
 * Each entry allocates a bare level of that size with the solver's own
 * helpers (the skewed working array, the hand-off granules, the ticket and
 * counter words, the partials), uploads its arguments, makes the launch calls
 * the Fluid or Elastic loop makes and no others, and downloads the results
 * unskewed.  Layouts as above; granules are unsigned [dimy*4]: row j of region
 * 0 as {x bits, y bits, tag, tag}.  Every entry refuses a NULL array (other
 * than those marked optional), a size below 1 and an unknown mode with
 * OF2D_ERR_INVALID_ARGUMENT and a message (of2d_gateway_last_error) before
 * any device work.  Not in the reference. */
/* launch_sor_pack.  elastic 0 (Fluid): force only, the working array's v plane
 * holds v0 before the launch; elastic 1: v = u as well (v0 unused).  v, b: the
 * planes after the launch; gran: region 0 (tags 0 before the launch). */
int of2d_prim_sor_pack(const float *u, const float *dI, const float *It, const float *v0,
                       int elastic, int dimx, int dimy, unsigned epoch, float *v, float *b,
                       unsigned *gran);
/* launch_regrid_pack with the Fluid loop's control words, the regrid word =
 * regridded (0: the launch must do nothing).  dI, It, b and gran are in/out:
 * the buffers hold the caller's values before the launch.  dimx, dimy >= 2. */
int of2d_prim_regrid_pack(const float *Iref, const float *Iaux, const float *v0, int regridded,
                          int dimx, int dimy, unsigned epoch, float *dI, float *It, float *b,
                          unsigned *gran);
/* nsweeps sweeps (epochs 1, 2, ...) of v with right-hand side b on one
 * workspace; between sweeps only the region-0 granules are re-tagged (a copy).
 * method 0: launch_sor on Elastic's buffers.  method 1: launch_sor_increment
 * on Fluid's, with the estimate u; after the last sweep R, scal = {maxabs, dt},
 * part = the increment_nblocks per-tile maxima and *path = 1 when the increment
 * workers ran, 0 for the fallback pair (R, scal, part, u optional at method 0).
 * zero_est: the regrid word is set.  skip_at = k (-1: none): the stop word says
 * the loop broke before sweep k, which must do nothing.  poison: every word of
 * the working array and of all granule regions is poison_word before v, b and
 * the region-0 granules are written.  words = {sweep ticket, role ticket, tile
 * counter} after the last sweep; *status the kernels' status word. */
int of2d_prim_sor_sweep(const float *v, const float *b, const float *u, int dimx, int dimy,
                        float mu, float lambda, float omega, int method, int nsweeps,
                        int zero_est, int skip_at, int poison, unsigned poison_word,
                        float *v_out, float *R, float *scal, float *part, int *path,
                        unsigned long long *words, unsigned *status);
/* launch_increment: R of the estimate u (read as zero with zero_est) and the
 * velocity v, scal = {maxabs, dt}, part as above */
int of2d_prim_fluid_increment(const float *u, const float *v, int dimx, int dimy, int zero_est,
                              float *R, float *scal, float *part);
/* launch_fluid_step with scal[1] = dt, then launch_fluid_report: uo, sums =
 * {sum |uo - prev|, sum |prev|} (prev optional: NULL takes u), the Jacobian
 * minimum, the packed force b and the region-0 granules (column 0 of v0)
 * tagged epoch + 1 */
int of2d_prim_fluid_step(const float *u, const float *R, const float *prev, const float *dI,
                         const float *It, const float *v0, float dt, int zero_est, int dimx,
                         int dimy, unsigned epoch, float *uo, double *sums, float *jmin, float *b,
                         unsigned *gran);
/* launch_fluid_report_decide on nb partial pairs lpart[2*nb] and minima
 * jpart[nb]; seq (optional): the exact float sums; scal = {maxabs, dt}.  words
 * (in/out) = {status, stop, regrid, mcur}.  The report starts as bytes 0xAB:
 * sums[2], repf = {maxabs, dt, jmin, seq[0], seq[1], err, scal[2]} (repf[6] is
 * in/out: scal[2] before the launch), repu = {status, flags}. */
int of2d_prim_fluid_decide(const double *lpart, const float *jpart, int nb, const float *seq,
                           double npx, int fixed, int it, const float *scal, unsigned *words,
                           double *sums, float *repf, unsigned *repu);
/* launch_logger on a working array whose v plane is v, then
 * launch_reduce_partials: u, the new prev, sums as of2d_prim_fluid_step */
int of2d_prim_elastic_logger(const float *v, const float *prev, int dimx, int dimy, float *u,
                             float *prev_out, double *sums);

/* ---- timing entry: the deformation analysis kernels ----
 * average duration (microseconds, HIP events around nlaunch back-to-back
 * launches after one untimed launch) at dimx x dimy: us[0] the Jacobian map
 * with its statistics (the map launch and its one-block reduction), us[1] one
 * update of the inverse at an iterate near the fixed point of a smooth 3-pixel
 * field.  A timing entry for tools/analysis_bench.py, not a result. */
int of2d_analysis_time_kernels(int dimx, int dimy, int nlaunch, double *us);

/* ---- test entries: the device-resident I/O kernels, one launch each ----
 * One launch each of the kernels behind the of2d_*_device entries, on the null
 * stream: pack `in` into npairs pitched fields and download them dense, float
 * [npairs][dimy][dimx]; upload dense fields (m_host interleaved x, y as the
 * other primitives' motion) and unpack them into `out`.  Refusals as for the
 * of2d_*_device entries, with the message in of2d_gateway_last_error.
 * The pack entries (an image stack, a motion stack [npairs][dimy][dimx][2], and
 * the host form's planar doubles [npairs][2][dimy][dimx]) fill the pitched
 * fields with the byte 0xC5 before the launch (as a float -6328.72), not with
 * the allocator's zeros.  raw_host (optional) receives the whole allocation
 * from its base, npairs * stride elements of the field's type: every pair's
 * ghost j-line above (P elements), its dimy rows of pitch P, the ghost j-line
 * below and the slack; what no store touched holds the sentinel.
 * of2d_prim_pack_layout reports that stride and P, in elements.
 * of2d_prim_pack_motion also refuses a pointer that is no device pointer. */
int of2d_prim_pack_layout(int dimx, int dimy, long long *stride, int *pitch);
int of2d_prim_pack_image(const of2d_darray *in, int npairs, int dimx, int dimy, float *out_host,
                         float *raw_host);
int of2d_prim_unpack_image(const float *in_host, int npairs, int dimx, int dimy,
                           const of2d_darray *out);
int of2d_prim_unpack_motion(const float *m_host, int npairs, int dimx, int dimy,
                            const of2d_darray *out);
int of2d_prim_pack_motion(const of2d_darray *in, int npairs, int dimx, int dimy, float *out_host,
                          float *raw_host);
int of2d_prim_planar_to_motion(const double *planar_host, int npairs, int dimx, int dimy,
                               float *out_host, float *raw_host);

/* ---- batched analysis kernels (batch_analysis_kernels.hip), one launch each ----
 * Dense host stacks of B pairs: u, v float [B][dimy][dimx][2], images and jac
 * float [B][dimy][dimx].  stats: B x 5, info: B x 4 (of2d_jacobian's and
 * of2d_invert_motion's per pair); jac and residuals (float [B][max_iter]) may
 * be NULL; a: one image with shared_a, else B; out: B x {mse, ncc}.  Refusals
 * as for of2d_field_jacobian / _invert / of2d_image_similarity, and B < 1 or
 * > 65535. */
int of2d_prim_batch_jacobian(const float *u, int B, int dimx, int dimy, float *jac,
                             double *stats);
int of2d_prim_batch_invert(const float *u, int B, int dimx, int dimy, int max_iter, double tol,
                           float *v, double *info, float *residuals);
int of2d_prim_batch_similarity(const float *a, int shared_a, const float *b, int B, int dimx,
                               int dimy, double *out);

#ifdef __cplusplus
}
#endif
#endif
