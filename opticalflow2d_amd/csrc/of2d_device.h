// of2d_device.h — shared definitions for the gfx950 kernels and the host
// driver of libof2d.so.
//
// HBM layout (DESIGN.md "Data layout"): every field of a pyramid level is a
// pitched, row-major (j-line major, x fastest) array whose pitch P is dimx
// rounded up to a multiple of 128 elements, with one zeroed ghost j-line above
// row 0 and one below row dimy-1.  Images are float (4 B/px), motion fields
// interleaved float2 (8 B/px) — the reference's layout (src/Field.tpp:13,
// src/Motion.h:7) plus padding, so 2-px float4 loads of a motion row and 4-px
// float4 loads of an image row are 16-B aligned.
#pragma once

#include <vector>

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

namespace of2d {

constexpr int kPitchAlign = 128;  // elements

inline int pitch_for(int dimx) { return (dimx + kPitchAlign - 1) / kPitchAlign * kPitchAlign; }
// a pitched field of dimy + 2 * ghost j-lines (plus the alignment slack) has
// fewer than 2^32 elements: the gather kernels' unsigned 32-bit offsets hold
inline bool field_fits_u32(int dimx, int dimy, int ghost) {
    return ((unsigned long long)dimy + 2ull * ghost) * (unsigned long long)pitch_for(dimx) +
               kPitchAlign < (1ull << 32);
}

struct DeviceError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define OF2D_HIP(call)                                                                    \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess)                                                             \
            throw ::of2d::DeviceError(std::string("HIP error: ") + hipGetErrorString(e_) + \
                                      " at " __FILE__ ":" + std::to_string(__LINE__));   \
    } while (0)

// Restores the calling thread's current device when the scope ends (normally
// or by an exception); bind() switches it meanwhile.  The multi-device paths
// switch devices per rank, and a caller's own device must survive every entry
// point.
class DeviceScope {
   public:
    DeviceScope() { (void)hipGetDevice(&prev_); }
    explicit DeviceScope(int dev) : DeviceScope() { bind(dev); }
    ~DeviceScope() {
        if (prev_ >= 0) (void)hipSetDevice(prev_);
    }
    void bind(int dev) { OF2D_HIP(hipSetDevice(dev)); }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;

   private:
    int prev_ = -1;
};

// status bits written by kernels (one word per context, zeroed per call)
constexpr unsigned kStatusDivZero = 1u;
constexpr unsigned kStatusExpBound = 2u;  // scaling-and-squaring count above the host bound
constexpr unsigned kStatusSpinTimeout = 4u;  // a bounded inter-workgroup wait gave up

// ---------------------------------------------------------------- HS Jacobi
// Each wave marches kHsRows j-lines of a kHsStrip-px strip (kHsPxl px per
// lane); a block is kHsWaves waves stacked in y (hs_jacobi_impl.h).
constexpr int kHsRows = 32;
constexpr int kHsPxl = 2;
constexpr int kHsStrip = 64 * kHsPxl;
constexpr int kHsWaves = 4;
inline dim3 hs_grid(int P, int nrows) {
    return dim3(P / kHsStrip, (nrows + kHsRows * kHsWaves - 1) / (kHsRows * kHsWaves));
}
inline int hs_nblocks(int P, int nrows) {
    dim3 g = hs_grid(P, nrows);
    return int(g.x * g.y);
}

// One Jacobi step of OpticalFlowDiffusion::get_update with the Logger's norm
// partials fused (sum ||u_new-u_old||, sum ||u_old|| per block, fp64).
// Row pointers address the first owned row; rows -1 and nrows must be valid
// memory (ghost j-lines).  row0 is the global j of the first owned row.
void launch_hs_jacobi(const float2 *u_old, float2 *u_new, const float2 *dI, const float *It,
                      int P, int dimx, int nrows, int row0, int dimy, float alphasq,
                      double *partial, unsigned *status, hipStream_t st);
// Two Jacobi iterations per launch (temporal blocking, hs::jacobi2_kernel):
// u_new = step(step(u_old)), bit-identical to two launch_hs_jacobi calls.
// Rows [glo, ghi) (relative to the first owned row; ghost j-lines included)
// are readable: u and dI/It outside the owned rows feed the first step's halo
// row on each side.  Logger partials of the first iteration go to partial,
// of the second to partial2 (hs2_nblocks blocks each).
constexpr int kHs2Out = 124;  // output columns per wave (hs_jacobi_impl.h)
constexpr int kHs2Rows = 32;
constexpr int kHs2Waves = 4;
inline dim3 hs2_grid(int dimx, int nrows) {
    return dim3((dimx + kHs2Out - 1) / kHs2Out,
                (nrows + kHs2Rows * kHs2Waves - 1) / (kHs2Rows * kHs2Waves));
}
inline int hs2_nblocks(int dimx, int nrows) {
    dim3 g = hs2_grid(dimx, nrows);
    return int(g.x * g.y);
}
// band_lo / band_hi: the row bands (kHs2Rows * kHs2Waves j-lines each) this
// launch covers; -1 / -1 = all of them.
inline int hs2_nbands(int nrows) {
    return (nrows + kHs2Rows * kHs2Waves - 1) / (kHs2Rows * kHs2Waves);
}
void launch_hs_jacobi2(const float2 *u_old, float2 *u_new, const float2 *dI, const float *It,
                       int P, int dimx, int nrows, int row0, int dimy, float alphasq, int glo,
                       int ghi, double *partial, double *partial2, unsigned *status,
                       hipStream_t st, int band_lo = -1, int band_hi = -1);
// Three Jacobi iterations per launch (hs::jacobi3_kernel): bit-identical to
// three launch_hs_jacobi calls; rows [glo, ghi) readable as for the pair
// kernel (the first two steps also cover two / one halo rows each side).
constexpr int kHs3Out = 120;  // output columns per wave (hs_jacobi_impl.h)
constexpr int kHs3Waves = 4;
// j-lines per wave.  A block's time is about (rows + 2) row steps (the
// prologue computes the halo rows of the first two iterations), and the 4-wave
// blocks (4 resident per CU, 256 CUs: `cap` = 1024 block slots, less when
// another launch is to run beside it) run in rounds, so the choice minimises
// rounds x (rows + 2) over rows in [4, 64], fewest rows on ties.  4096^2: 36
// (1015 blocks, one round; 32 gave 1120 blocks and a 9 % second round);
// 16384^2: 50 (11 rounds of 1006-1024 blocks, against 59 and 9.4 rounds);
// grids too small to fill one round get short bands and more blocks.
inline int hs3_rows(int dimx, int nrows, int cap = 1024) {
    const long gx = (dimx + kHs3Out - 1) / kHs3Out;
    int best = 4;
    long best_t = -1;
    for (int r = 4; r <= 64; r++) {
        const long bands = (nrows + kHs3Waves * r - 1) / (kHs3Waves * r);
        const long rounds = (gx * bands + cap - 1) / cap;
        const long t = rounds * (r + 2);
        if (best_t < 0 || t < best_t) {
            best_t = t;
            best = r;
        }
        if (bands == 1) break;  // more rows per wave change nothing
    }
    return best;
}
inline int hs3_nbands(int dimx, int nrows) {
    const int r = kHs3Waves * hs3_rows(dimx, nrows);
    return (nrows + r - 1) / r;
}
inline dim3 hs3_grid(int dimx, int nrows) {
    return dim3((dimx + kHs3Out - 1) / kHs3Out, hs3_nbands(dimx, nrows));
}
inline int hs3_nblocks(int dimx, int nrows) {
    dim3 g = hs3_grid(dimx, nrows);
    return int(g.x * g.y);
}
// range_flag: the word launch_hs_precheck wrote for this dI (required: the
// kernel leaves the divide-by-zero test to it)
// The triple kernel reads dI + It (12 B/px) at every launch.  While both fit
// in the 256 MB MALL (Infinity Cache) they stay resident between launches
// and reading them costs no HBM bandwidth; past that the launch is HBM-bound
// and deriving dI from Iaux in the kernel (GI, 4 B/px instead of 8) saves a
// seventh of its bytes.  Measured per launch (profiles/r02_d_gi_pf_ab*.log):
// 4096^2 81.4 (dI) vs 81.1 us (GI), 16384^2 1553 vs 1335 us.
constexpr double kMallBytes = 256.0 * 1024 * 1024;
inline bool hs3_gradients_from_image(int dimx, int nrows) {
    return 12.0 * dimx * nrows > kMallBytes;
}
// HS's exact-Logger loop streams more than the triple: per three iterations
// the MID triple (u0 in, three iterates out) and the Logger pass (four
// iterates in, non-temporal) move 64 B/px beside the gradients' 12, so dI + It
// stay in the MALL only where all of it fits (4096^2: GI and the pass's
// non-temporal loads 140 -> 131 us per iteration texture, 118 -> 107
// procedural, profiles/r05o_gi_nt_ab.log)
inline bool hs3_exact_gradients_from_image(int dimx, int nrows) {
    return 76.0 * dimx * nrows > kMallBytes;
}
// Ia (Iaux, the image dI was taken of) non-null: the kernel derives the
// gradients from it (24 instead of 28 B/px per launch, same bits); null: it
// reads dI
void launch_hs_jacobi3(const float2 *u_old, float2 *u_new, const float2 *dI, const float *It,
                       int P, int dimx, int nrows, int row0, int dimy, float alphasq, int glo,
                       int ghi, double *partial, double *partial2, double *partial3,
                       unsigned *status, const unsigned *range_flag, hipStream_t st,
                       int band_lo = -1, int band_hi = -1, const float *Ia = nullptr,
                       float2 *u1 = nullptr, float2 *u2 = nullptr, const int *stop = nullptr,
                       int stop_t0 = 0, int slots = 1024);
// (slots: resident 4-wave blocks the launch may have, for its j-lines per
// wave, hs3_rows; 1024 = every CU of the device)
// (u1, u2 non-null: the first two iterates of the owned rows are stored there
// too, for the reference-exact Logger; +16 B/px; with stop, the launch does
// nothing when *stop < stop_t0: the loop broke before the triple's first
// iteration stop_t0, seqnorm_decide)
// Once per gradient field, before the triple kernel runs on it
// (hs_jacobi_impl.h hs_precheck_kernel): zeroes *range_flag, then sets it if
// any gradient / denominator of the allocation [base, base + count) lies
// outside the unscaled-division range, and ORs kStatusDivZero into *status if
// an image pixel's denominator is 0.  ghost: j-lines before row 0 in base.
// The triple kernel over j-lines [jlo, jhi) of the level, rows_per_wave
// j-lines per wave, Logger partials from slot band `slot_band0` on (slot =
// (slot_band0 + block row) * gx + strip): the slab's interior / edge launches.
// Returns the launch's block rows.
int launch_hs_jacobi3_window(const float2 *u_old, float2 *u_new, const float2 *dI,
                             const float *It, int P, int dimx, int nrows, int row0, int dimy,
                             float alphasq, int glo, int ghi, int jlo, int jhi,
                             int rows_per_wave, int slot_band0, double *partial,
                             double *partial2, double *partial3, unsigned *status,
                             const unsigned *range_flag, hipStream_t st,
                             const float *Ia = nullptr);
void launch_hs_precheck(const float2 *base, size_t count, int P, int ghost, int dimx, int dimy,
                        float alphasq, unsigned *range_flag, unsigned *status, hipStream_t st);
// Four Jacobi iterations per launch (hs::jacobi4_kernel) over a whole image
// (rows 0 .. dimy-1 of the level: no neighbour above or below, so the j-lines
// outside [0, dimy) only feed pixels the border rule zeroes), bit-identical to
// four launch_hs_jacobi calls.  The triple's grid and partial slots
// (hs3_rows(dimx, dimy, slots)); rows [glo, ghi) of u, dI and It readable
// (rows beyond are clamped into it); the gradients are read from dI;
// range_flag as for the triple (launch_hs_precheck's word, required).  The
// j-lines per wave are hs3_rows', whose cost model (rounds x (rows + 2)) is the
// triple's, reused on purpose: the quad's prologue is a row step or two longer,
// which moves the optimum only where two candidates are that close, and equal
// rows keep the quad's blocks and Logger partials those of the triple.
// tail_exchange: the instantiation whose wave pairs exchange their end-of-band
// rows through LDS (hs_jacobi_impl.h XCH); the same bits either way.
void launch_hs_jacobi4(const float2 *u_old, float2 *u_new, const float2 *dI, const float *It,
                       int P, int dimx, int dimy, float alphasq, int glo, int ghi,
                       double *partial, double *partial2, double *partial3, double *partial4,
                       const unsigned *range_flag, hipStream_t st, int slots = 1024,
                       bool tail_exchange = true);
constexpr int kRangeFlagWord = 32;  // word of the 64-word status buffers holding range_flag
constexpr int kStopWord = 33;  // the exact-Logger loop's break (seqnorm_decide)
// the Fluid loop's device-side decisions (Registration::loop_fluid, FluidCtl):
// the iteration just decided regridded (the next iteration's estimate reads as
// zero, its Logger prev is the buffer's content), and which of the level's two
// motion fields holds the accumulated motion
constexpr int kFluidRegridWord = 34;
constexpr int kFluidMcurWord = 35;
// A Fluid iteration's kernels and its place in the loop: w = the 64-word
// status buffer (kStopWord: the first breaking iteration, 0x7f7f7f7f none;
// kFluidRegridWord, kFluidMcurWord), it = the iteration.  Every kernel of an
// iteration past the break returns at once; w == nullptr: no control words
// (the kernels' plain behaviour, other callers)
struct FluidCtl {
    unsigned *w = nullptr;
    int it = 0;
};
// blocks of the launches that the control words usually make no-ops (the
// regrid's): grid-stride loops over a capped grid, so an idle launch costs a
// few microseconds instead of dispatching a block per tile
constexpr int kCappedGrid = 2048;
// (plain loads: the words are written by earlier kernels of the same stream)
__device__ __forceinline__ bool fluid_stopped(const FluidCtl &c) {
    return c.w && (int)c.w[kStopWord] < c.it;
}
// the iteration's input estimate is the zero field of a regrid (its buffer
// still holds the pre-regrid estimate, the Logger's prev)
__device__ __forceinline__ bool fluid_zero_est(const FluidCtl &c) {
    return c.w && c.w[kFluidRegridWord] != 0u;
}
// partial-row length that fits every HS kernel (single, pair, triple)
inline int hs_partial_blocks(int P, int dimx, int nrows) {
    int nb = hs_nblocks(P, nrows);
    nb = nb > hs2_nblocks(dimx, nrows) ? nb : hs2_nblocks(dimx, nrows);
    return nb > hs3_nblocks(dimx, nrows) ? nb : hs3_nblocks(dimx, nrows);
}
// Sum C iterations' per-block partials in a fixed order: sums[2t+{0,1}] =
// {sum ||diff||, sum ||prev||} for t < C.
// out[i] = sum over r < n of src[r][i], added in rank order (the in-process
// slab group's all-reduce, slab.cpp); n <= kMaxLocalRanks
constexpr int kMaxLocalRanks = 16;
// device-to-device copy of whole float2s on one device, by a few blocks
void launch_copy_lines(void *dst, const void *src, size_t bytes, hipStream_t st);
void launch_sum_ranks(const double *const *src, int n, size_t count, double *out, hipStream_t st);
// Row t of `partial` starts at t * stride * 2 doubles (stride = nblocks if < 0).
void launch_reduce_partials(const double *partial, int nblocks, int C, double *sums,
                            hipStream_t st, int stride = -1);
// The launches of one chunk: runs of consecutive iterations whose kernels wrote
// the same number of block partials, so that rows are reduced over exactly the
// blocks that wrote them (no zero fill of the partial rows per chunk).
struct PartialRuns {
    struct Run {
        int t0, len, nblocks;
    };
    std::vector<Run> runs;
    void add(int t, int len, int nblocks);
    void reduce(const double *partial, int stride, double *sums, hipStream_t st) const;
};

// ---------------------------------------------------------------- Logger sums
// The one definition of the fp64 Logger sums' arithmetic and of the fixed
// order in which every kernel adds them (DESIGN.md "fixed order"; the
// multi-rank path is bit-identical to one GPU because of it;
// tests/test_gpu_logger_partials.py restates the order in numpy).
//
// Motion::norm's magnitude (src/Motion.cpp:42-47): the float components
// widened, squared and added in double (-ffp-contract=off: no fused
// multiply-add), then the correctly rounded double root.  Every kernel's
// Logger terms are these; the one exception is the HS Jacobi kernels' norm_d
// (hs_jacobi_impl.h), a float32 root by measurement.
__device__ __forceinline__ double logger_mag(float x, float y) {
    const double a = x, b = y;
    return sqrt(a * a + b * b);
}
// a pixel's two terms (Logger.cpp:34-42): |cur - prev| of the float32
// difference onto sd, |prev| onto sp
__device__ __forceinline__ void logger_add(float2 cur, float2 prev, double &sd, double &sp) {
    sd += logger_mag(cur.x - prev.x, cur.y - prev.y);
    sp += logger_mag(prev.x, prev.y);
}
// Wave trees: lane i takes lane i + off for off = 32 ... 1; the result is in
// lane 0 (the other lanes hold partial trees)
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}
template <class T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T o = __shfl_down(v, off);
        v = (o < v) ? o : v;
    }
    return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T o = __shfl_down(v, off);
        v = (v < o) ? o : v;
    }
    return v;
}
// The N sums of a block of WAVES waves (thread = wave * 64 + lane): wave
// trees, lane 0 of each wave to LDS, one barrier, then the block's first
// thread adds waves 0 ... WAVES-1 in that order into its v[] (the other
// threads' v[] hold partial trees).  Its sums start from 0.0 + wave 0, the
// same bits as wave 0 itself for these sums (non-negative or NaN).  One call
// per instantiation and kernel: the LDS array is the instantiation's.  The
// tails of the three HS Jacobi kernels (hs_jacobi_impl.h) keep their own
// copies of exactly this order, with the status word's atomicOr before the
// barrier: moving them here changed the hot kernels' code size.
template <int N, int WAVES>
__device__ __forceinline__ void block_sums(double (&v)[N], int wave, int lane) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int q = 0; q < N; q++) v[q] += __shfl_down(v[q], off);
    __shared__ double red[N][WAVES];
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < N; q++) red[q][wave] = v[q];
    }
    __syncthreads();
    if (wave == 0 && lane == 0) {
#pragma unroll
        for (int q = 0; q < N; q++) v[q] = 0.0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w)
#pragma unroll
            for (int q = 0; q < N; q++) v[q] += red[q][w];
    }
}
// The Logger pair of a 64 x 4 block -> partial[2 blk], partial[2 blk + 1],
// blk = blockIdx.y * gridDim.x + blockIdx.x
__device__ __forceinline__ void block_logger_partial(double sd, double sp,
                                                     double *__restrict__ partial) {
    double v[2] = {sd, sp};
    block_sums<2, 4>(v, threadIdx.y, threadIdx.x);
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
        partial[2 * blk] = v[0];
        partial[2 * blk + 1] = v[1];
    }
}
// nb (diff, prev) partial pairs by one 1024-thread block: thread t adds pairs
// t, t + 1024, ... in order, then block_sums over the 16 waves; the sums are
// thread 0's s[]
__device__ __forceinline__ void partial_pairs_sum(const double *__restrict__ p, int nb,
                                                  double (&s)[2]) {
    s[0] = s[1] = 0.0;
    for (int i = threadIdx.x; i < nb; i += 1024) {
        s[0] += p[2 * i];
        s[1] += p[2 * i + 1];
    }
    block_sums<2, 16>(s, threadIdx.x >> 6, threadIdx.x & 63);
}
// min / max over a block of WAVES waves, valid in its first thread; includes
// a barrier.  The order of a min or max does not change its value.
template <int WAVES>
__device__ __forceinline__ float block_min(float m, int wave, int lane) {
    m = wave_min(m);
    __shared__ float red[WAVES];
    if (lane == 0) red[wave] = m;
    __syncthreads();
    for (int w = 1; w < WAVES; w++) m = (red[w] < m) ? red[w] : m;
    return m;
}
template <int WAVES>
__device__ __forceinline__ float block_max(float m, int wave, int lane) {
    m = wave_max(m);
    __shared__ float red[WAVES];
    if (lane == 0) red[wave] = m;
    __syncthreads();
    for (int w = 1; w < WAVES; w++) m = (m < red[w]) ? red[w] : m;
    return m;
}

// ---------------------------------------------------------------- Logger norms
// The reference's Motion::norm (src/Motion.cpp:42-49) bit for bit: the float
// running sum S <- (float)((double)S + sqrt((double)x^2 + (double)y^2)) over
// the pixels in linear order, of |cur - prev| (out[0]) and |prev| (out[1])
// (Logger::update_error, src/Logger.cpp:32-51; seqnorm_kernels.hip).  out[]
// holds the sums, not yet divided by N.  ws: seqnorm_workspace_bytes; it also
// keeps each call's running-sum profile, which the next call on the same grid
// uses as its prediction when use_profile is set (the result is exact either
// way; a poor prediction costs time).  dbg (optional, int[10]): the walk's
// cost counters (resolves, raw segments, listed tiles, clocks, tiles given
// its own segment entries).
constexpr int kSnTile = 4096;  // consecutive terms per tile
size_t seqnorm_workspace_bytes(int dimx, int dimy);
void launch_seqnorm(const float2 *cur, const float2 *prev, int dimx, int dimy, int P, void *ws,
                    bool use_profile, float *out, int *dbg, hipStream_t st);
// the two halves of launch_seqnorm: the bandwidth passes (tables) and the
// latency-bound walk, so that a pipeline can run them on separate streams
// (the walk reads what tables wrote; tables reads the profile the last walk
// on the same workspace wrote)
void launch_seqnorm_tables(const float2 *cur, const float2 *prev, int dimx, int dimy, int P,
                           void *ws, bool use_profile, hipStream_t st);
// s_in (optional, device float[2]): the exact running sums of the terms
// before this grid — a row slab's norms continue its predecessor's
void launch_seqnorm_walk(const float2 *cur, const float2 *prev, int dimx, int dimy, int P,
                         void *ws, const float *s_in, float *out, int *dbg, hipStream_t st);
// launch_seqnorm_tables in parts for row slabs: the pass over the slab, its
// fp64 total (returned: device double[2] inside ws), the predecessors' totals
// chained in rank order for K pairs (poff = the previous rank's nxt, or 0
// without one; nxt = poff + tot: device double[K][2] each, prev_nxt
// peer-readable), and the
// check / fix with that offset (p_off, device double[2], optional)
void launch_seqnorm_pass(const float2 *cur, const float2 *prev, int dimx, int dimy, int P,
                         void *ws, bool use_profile, hipStream_t st);
const double *seqnorm_total(int dimx, int dimy, int P, void *ws, hipStream_t st);
void launch_seqnorm_offset_chain(const double *prev_nxt, const double *const *tot, int K,
                                 double *poff, double *nxt, hipStream_t st);
void launch_seqnorm_refine(const float2 *cur, const float2 *prev, int dimx, int dimy, int P,
                           void *ws, bool use_profile, const double *p_off, hipStream_t st);
// A batch of K <= 3 consecutive Logger updates of one loop: pair i is
// (prev, cur) = (u[i], u[i + 1]) on workspace ws[i] (its own profile), so the
// pass reads the K + 1 iterates once (a Jacobi triple's four arrays for three
// updates) and each of check, fix and walk is one launch for the batch.
struct SeqnormBatch {
    int K = 1;
    const float2 *u[4] = {};
    void *ws[3] = {};
    bool use_profile[3] = {};
    const double *p_off[3] = {};  // refine: a row slab's predecessors' fp64 sums
    const float *s_in[3] = {};    // walk: a row slab's predecessors' exact sums
    float *out[3] = {};           // walk: the sums of pair i (device float[2])
    int *dbg[3] = {};             // walk: cost counters (int[10]), optional
    // the loop's break word (launch_seqnorm_decide): with it, every kernel of
    // the batch returns at once when *stop < t0 (t0: the batch's first
    // iteration)
    const int *stop = nullptr;
    int t0 = 0;
    // the pass (launch_seqnorm_pass) over tiles [tile_lo, tile_hi) only
    // (tile_hi 0: every tile); the launch with tile_lo 0 resets the check's list
    unsigned tile_lo = 0, tile_hi = 0;
    // the pass's scale prediction (OF2D_SN_NEAR): workspaces of pair i in the
    // three groups before this one (their checks' fp64 totals, taken when the
    // check has stamped them with `epoch` + its iteration + 1), null: none
    void *near[3][3] = {};
    unsigned epoch = 0;  // the loop's tag in the stamps' high 12 bits
};
// the Logger errors of a walked batch (pair i's sums at seq[2i], seq[2i + 1]),
// as logger_error does on the host: the first iteration t0 + i > 1 whose
// error is below 0.001 into *stop (atomicMin); the sums copied to host
// (mapped host memory, float[2K])
void launch_seqnorm_decide(const float *seq, int K, int t0, double npx, int *stop, float *host,
                           hipStream_t st);
// diagnostics (tools/seqnorm_bench; synchronous): the workspace's list count
// and profile flags (cnt[0..3]), then per norm the tiles with segment entries,
// with more than one candidate, with none (out[12])
void seqnorm_ws_stats(const void *ws, int dimx, int dimy, unsigned *out);
void launch_seqnorm_pass(const SeqnormBatch &b, int dimx, int dimy, int P, hipStream_t st);
void launch_seqnorm_refine(const SeqnormBatch &b, int dimx, int dimy, int P, hipStream_t st);
void launch_seqnorm_walk(const SeqnormBatch &b, int dimx, int dimy, int P, hipStream_t st);

// ---------------------------------------------------------------- fields
void launch_d2f(const double *in, int dimx, int dimy, float *out, int P, int row_offset,
                hipStream_t st);
void launch_f2d(const float *in, int P, int dimx, int dimy, double *out, hipStream_t st);
void launch_motion_to_planar(const float2 *m, int P, int dimx, int dimy, double *out,
                             hipStream_t st);
// A caller's strided device array (include/of2d.h of2d_darray, validated):
// element strides of the pair, x, y and component axes
struct DArrayView {
    void *ptr = nullptr;
    bool f64 = false;
    long long sp = 0, sx = 0, sy = 0, sc = 0;
};
// io_kernels.hip: npairs images or motion fields in one launch; the pitched
// side holds pair k at k * so (si, sm) elements, pitch P
void launch_pack_image(const DArrayView &in, int npairs, int dimx, int dimy, float *out, long so,
                       int P, hipStream_t st);
void launch_unpack_image(const float *in, long si, int P, int npairs, int dimx, int dimy,
                         const DArrayView &out, hipStream_t st);
void launch_unpack_motion(const float2 *m, long sm, int P, int npairs, int dimx, int dimy,
                          const DArrayView &out, hipStream_t st);
// launch_unpack_motion's mirror, each component cast to float; and the host
// form: npairs planar double fields (as launch_motion_to_planar writes them)
void launch_pack_motion(const DArrayView &in, int npairs, int dimx, int dimy, float2 *m, long sm,
                        int P, hipStream_t st);
void launch_planar_to_motion(const double *in, int npairs, int dimx, int dimy, float2 *m, long sm,
                             int P, hipStream_t st);
// `waiter` behind everything enqueued on `signal` so far
inline void stream_after(hipStream_t waiter, hipStream_t signal, hipEvent_t ev) {
    OF2D_HIP(hipEventRecord(ev, signal));
    OF2D_HIP(hipStreamWaitEvent(waiter, ev, 0));
}
// refuses (std::invalid_argument) a pointer that is not device memory of `dev`
void check_device_pointer(const void *p, int dev, const char *what);
void launch_downsample_image(const float *in, int dxi, int dyi, int Pi, float *out, int dxo,
                             int dyo, int Po, hipStream_t st);
void launch_downsample_motion(const float2 *in, int dxi, int dyi, int Pi, float2 *out, int dxo,
                              int dyo, int Po, hipStream_t st);
void launch_upsample_motion(const float2 *in, int dxi, int dyi, int Pi, float2 *out, int dxo,
                            int dyo, int Po, hipStream_t st);
void launch_warp(const float *src, const float2 *u, float *dst, int dimx, int dimy, int P,
                 hipStream_t st);
void launch_gradients(const float *Iref, const float *Iaux, float2 *dI, float *It, int dimx,
                      int dimy, int P, hipStream_t st);
// slab variant: rows [0, nrows) of a slab whose first row is global j-line row0;
// rows -1 and nrows are ghost j-lines holding the neighbours' image rows
void launch_gradients_rows(const float *Iref, const float *Iaux, float2 *dI, float *It, int dimx,
                           int nrows, int P, int row0, int dimy, hipStream_t st);
void launch_accumulate(const float2 *m_old, const float2 *v, float2 *m_new, int dimx, int dimy,
                       int P, hipStream_t st);
// Fluid regridding: m_new <- accumulate(m_old, est), est0 <- 0 over the image
// pixels (ghost lines and pitch padding are never written), Iaux <- warp(Imov, m_new)
void launch_regrid(const float2 *m_old, const float2 *est, float2 *est0, float2 *m_new,
                   const float *Imov, float *Iaux, int dimx, int dimy, int P, hipStream_t st);
void launch_compose_zero(const float2 *v, float2 *out, int dimx, int nrows, int P, int row0,
                         int dimy, hipStream_t st);
// out rows [0, nrows) = warp2d of `raw` by a zero motion (field_kernels.hip):
// the identity except beside non-finite pixels; reads raw row nrows where
// row0 + nrows < dimy
void launch_warp_zero_rows(const float *raw, float *out, int dimx, int nrows, int P, int row0,
                           int dimy, hipStream_t st);
void launch_add_motion(const float2 *a, const float2 *b, float2 *out, int dimx, int dimy, int P,
                       hipStream_t st);
// (int)floorf(v) as the reference's x86-64 build converts it: a NaN gives
// INT_MIN (cvttss2si), which the callers' range tests reject, where the
// device's conversion gives 0, a pixel inside the grid.  (Values beyond int
// give INT_MIN there and INT_MAX here: outside the grid either way.)  Every
// conversion of a sampling coordinate goes through it: accumulate_px below,
// warp_px (field_px.h), compose_zero_kernel (field_kernels.hip), warp_batch,
// compose_px and exp_square_kernel (demons_kernels.hip) and the out-of-bounds
// count of invert_step_kernel (analysis_kernels.hip).  upsample_motion_px
// converts finite grid coordinates only and keeps the bare conversion.
// Held by tests/test_gpu_nonfinite_sampling.py.
__device__ __forceinline__ int floor_int(float v) {
    return v == v ? (int)floorf(v) : (int)0x80000000;
}

// One pixel of Motion::accumulate (src/Motion.cpp:113-178): c + mo(x + c),
// bilinear and renormalised by the valid weight; `own` where floor(x + c) falls
// outside the grid.  Branch-free (field_kernels.hip, warp_px): the taps are
// loaded unconditionally (an out-of-range pattern reads element 0; g[1], g[P],
// g[P+1] of an in-image pixel stay in the allocation: pitch padding and the
// zeroed ghost j-line below the last row) and the reference's conditional terms
// are selects.
__device__ __forceinline__ float2 accumulate_px(const float2 *__restrict__ mo, float2 c,
                                                float2 own, int i, int j, int dimx, int dimy,
                                                int P) {
    const float px = (float)i + c.x;
    const int dx = floor_int(px);
    const float fx = px - (float)dx;
    const float py = (float)j + c.y;
    const int dy = floor_int(py);
    const float fy = py - (float)dy;
    const bool ok = !(dx < 0 || dx >= dimx || dy < 0 || dy >= dimy);
    const bool ax = dx < dimx - 1, ay = dy < dimy - 1, axy = ax && ay;
    const float2 *b = mo + (ok ? ((unsigned)dy * (unsigned)P + (unsigned)dx) : 0u);
    const float2 t00 = b[0], t10 = b[1], t01 = b[P], t11 = b[P + 1];
    float vx = (t00.x * (1 - fx)) * (1 - fy);
    float vy = (t00.y * (1 - fx)) * (1 - fy);
    float w = (1 - fx) * (1 - fy);
    const float x10 = vx + (t10.x * fx) * (1 - fy), y10 = vy + (t10.y * fx) * (1 - fy);
    const float w10 = w + fx * (1 - fy);
    vx = ax ? x10 : vx;
    vy = ax ? y10 : vy;
    w = ax ? w10 : w;
    const float x01 = vx + (t01.x * (1 - fx)) * fy, y01 = vy + (t01.y * (1 - fx)) * fy;
    const float w01 = w + (1 - fx) * fy;
    vx = ay ? x01 : vx;
    vy = ay ? y01 : vy;
    w = ay ? w01 : w;
    const float x11 = vx + (t11.x * fx) * fy, y11 = vy + (t11.y * fx) * fy;
    const float w11 = w + fx * fy;
    vx = axy ? x11 : vx;
    vy = axy ? y11 : vy;
    w = axy ? w11 : w;
    float2 q = make_float2(c.x + vx, c.y + vy);  // vx / 1.0f is vx
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(ok && w != 1.0f) != 0, 0))
        q = make_float2(c.x + vx / w, c.y + vy / w);
    return ok ? (w != 0 ? q : c) : own;
}

// ---------------------------------------------------------------- analysis
// Deformation analysis of a motion field that is already on the device
// (analysis_kernels.hip; DESIGN.md "Deformation analysis").  Every reduction
// runs over per-block partials in a fixed order, without float atomics: two
// calls on the same input give the same bits.
//
// Jacobian determinant map (Image::jacobian, src/Image.cpp:189-218, the
// expression fluid_step_kernel evaluates inline) with its statistics in the
// same launch; a second, one-block launch reduces the partials.
struct JacPartial {
    float mn, mx;
    double sum;
    unsigned le0, lt05;  // J <= 0 (folded), J < 0.5f (Fluid's regrid threshold)
};
int jacobian_nblocks(int dimx, int dimy);
// jac (optional): pitched float map (pitch P; the pitch padding of a written
// row is zeroed); part: jacobian_nblocks partials; stats: device double[5] =
// {min, max, mean, count(J <= 0), count(J < 0.5)}.  dimx, dimy >= 2.
void launch_jacobian(const float2 *u, int dimx, int dimy, int P, float *jac, JacPartial *part,
                     double *stats, hipStream_t st);

// Similarity of two pitched float images: fp64 sums of a, b, a^2, b^2, ab and
// (a - b)^2 and the images' extrema per block, reduced by a one-block launch to
// out = device double[2] = {mse, ncc}; ncc (zero-mean normalised
// cross-correlation) is NaN when an image is constant (min == max).
struct SimPartial {
    double s[6];
    float mn[2], mx[2];
};
int similarity_nblocks(int dimx, int dimy);
void launch_similarity(const float *a, const float *b, int dimx, int dimy, int P,
                       SimPartial *part, double *out, hipStream_t st);

// Inverse field by fixed-point iteration: v_{k+1} = v_k - r_k with r_k =
// accumulate(u, v_k), 0 where floor(x + v_k) is outside the grid (the pixel is
// counted, v kept), m_k = max |r_k| over both components.  Control words
// (device, invert_ctl_words(max_iter), prepared by invert_field): [0] the
// updates applied when the loop stopped (kInvertRunning until then), [1 + k]
// the bits of m_k, [1 + max_iter + k] the out-of-bounds pixels of update k.
// Update k > 0 first reads its predecessor's m: below tol it writes the stop
// word and, like every later launch, does nothing.
constexpr int kInvertChunk = 8;  // updates enqueued between the host's reads
constexpr unsigned kInvertRunning = 0x7f7f7f7fu;
inline size_t invert_ctl_words(int max_iter) { return 1 + 2 * (size_t)max_iter; }
void launch_invert_step(const float2 *u, const float2 *vin, float2 *vout, int dimx, int dimy,
                        int P, int k, float tol, unsigned *ctl, int max_iter, hipStream_t st);
struct InvertResult {
    int iterations = 0;
    float residual = 0.0f;  // m of the last update applied
    unsigned oob = 0;       // out-of-bounds pixels at the last evaluated iterate
    bool converged = false;
    float2 *v = nullptr;    // v0 or v1: the buffer holding the result
};
// The loop from v_0 = 0 (v0 zeroed by the caller over the image; v1 scratch),
// kInvertChunk launches between reads of the control words.  residuals
// (optional, host float[max_iter]): m_k of every update applied, 0 beyond.
// Synchronises st.
InvertResult invert_field(const float2 *u, float2 *v0, float2 *v1, int dimx, int dimy, int P,
                          int max_iter, float tol, unsigned *ctl, float *residuals,
                          hipStream_t st);

// ---------------------------------------------------------------- Demons
void launch_demons_force(const float *Iref, const float *Imov, const float2 *u, float2 *corr,
                         int dimx, int dimy, int P, float sigma_isq, float sigma_xsq,
                         unsigned *status, hipStream_t st);
dim3 conv_grid(int dimx, int dimy);
int conv_nblocks(int dimx, int dimy);
// the widest kernel the separable smoothing is compiled for (OF2D_SEP_KW_MAX)
constexpr int kSepKwMax = 15;
// the separable smoothing takes a level: kw odd, 3 <= kw <= kSepKwMax (an even
// table's taps do not cover it and its marginals are not its factors), and
// dimx >= kw
bool demons_separable_ok(int kw, int dimx);
// One correction update (DemonsThirions.cpp:20-38): force, sigma_fluid
// smoothing and the motion update (mode as launch_smooth_compose) -> out.
// One fused launch over every tile (demons_fused_kernel; the x-edge tiles hold
// the wrapped tap pixels) for kw 3 / 5 / 7 with (float)wfull == 1 (separable:
// every width it takes)
// and dimx >= 128; otherwise the unfused kernels through corr (scratch).
// gs (this and the two launches below): nullptr for the direct convolution;
// otherwise the kernel's (float) row marginals then column marginals (kw
// each, gaussian_marginals) for the separable smoothing where
// demons_separable_ok, the direct one elsewhere.  Returns 1 when the separable
// kernels ran, 0 for the direct ones.
int launch_demons_update(const float *Iref, const float *Imov, const float2 *u, float2 *corr,
                         float2 *out, int dimx, int dimy, int P, float sigma_isq,
                         float sigma_xsq, const float *kf, const double *kd, int kw,
                         double wfull, int mode, unsigned *status, hipStream_t st,
                         const float *gs = nullptr);
// mode 0 Composition, 1 Addition, 2 no update, 3 store the smoothed corr only
int launch_smooth_compose(const float2 *corr, const float2 *u, float2 *out, int dimx, int dimy,
                          int P, const float *kf, const double *kd, int kw, double wfull,
                          int mode, hipStream_t st, const float *gs = nullptr);
int launch_smooth_norm(const float2 *umid, const float2 *prev, float2 *out, int dimx, int dimy,
                       int P, const float *kf, const double *kd, int kw, double wfull,
                       double *partial, hipStream_t st, const float *gs = nullptr);
// Motion::exp (Motion.cpp:253-277) on f; *result is f or scratch
void launch_motion_exp(float2 *f, float2 *scratch, int dimx, int dimy, int P, int nsq_max,
                       float *d_part, int nparts, int *d_nsq, float *d_maxabs, unsigned *status,
                       float2 **result, hipStream_t st);

// ---------------------------------------------------------------- Curvature
// C = A B (column-major fp64, MFMA), times E elementwise when E != nullptr;
// batch z offsets A, B, C by sA, sB, sC elements
void launch_dgemm(int M, int N, int K, const double *A, long lda, long sA, const double *B,
                  long ldb, long sB, double *C, long ldc, long sC, const double *E, long lde,
                  int batch, hipStream_t st);
// X planes (x at 0, y at `plane`, pitch P) <- (double)(u - tau * force(u))
void launch_curv_rhs(const float2 *u, const float2 *dI, const float *It, float tau, int dimx,
                     int dimy, int P, double *X, long plane, hipStream_t st);
int curv_nblocks(int dimx, int dimy);
// out <- (float)Z / div, Logger partials against u
void launch_curv_construct(const double *Z, long plane, const float2 *u, float2 *out, float div,
                           int dimx, int dimy, int P, double *partial, hipStream_t st);

// Fast line transforms (dct_kernels.hip): lengths that are a power of two in
// [kDctMinN, kDctMaxN].  kDctMaxN is the longest line pair (16 B per point)
// that fits the 160 KiB of LDS of a CU: 8192 points are 128 KiB.
constexpr int kDctMinN = 8;
constexpr int kDctMaxN = 8192;
bool dct_fast_length(int n);
// the twiddles of length n as 2n (re, im) pairs: exp(-2 pi i m / n), then
// exp(-i pi k / (2n)), evaluated in fp64 on the host
std::vector<double> dct_table(int n);
// kind 0: REDFT10 (times E[k + line * P] when E != nullptr), 1: REDFT01, of
// lines [0, nlines) of length n, in place: element k of line l at X[l * P + k]
// and X[plane + l * P + k]; tw is dct_table(n) on the device
void launch_dct_lines(double *X, long plane, int P, int nlines, int n, int kind, const double *tw,
                      const double *E, hipStream_t st);
// D[j + i * Pd] = S[i + j * Ps] for i < n0, j < n1, both planes
void launch_transpose_pair(const double *S, long Ps, long planeS, double *D, long Pd, long planeD,
                           int n0, int n1, hipStream_t st);

// ---------------------------------------------------------------- Fluid / Elastic
int sor_nstrips(int dimx);
// The SOR working array vb is stored skewed along the Gauss-Seidel wavefront:
// pixel (i, j) at row 2i + j, column i (fluid_kernels.hip).  A row is 16 P
// bytes: P float2 values of the field being relaxed (v), then P float2
// right-hand sides (b), so the passes that write only b (the force) or read
// only v write / read contiguous runs of 8-B elements.  It has
// sor_rows(dimx, dimy) rows; the last kSorPadRows are padding for lanes that
// run past the image (as do the kSorPadRows above and below each granule region).
constexpr int kSorPadRows = 256;
// float2 index of v(i, j) / b(i, j) in vb
__host__ __device__ inline long sor_v(int i, int j, int P) { return (2L * i + j) * 2L * P + i; }
__host__ __device__ inline long sor_b(int i, int j, int P) { return sor_v(i, j, P) + P; }
inline int sor_rows(int dimx, int dimy) { return 2 * dimx + dimy + kSorPadRows; }
long sor_granule_stride(int dimy);
// (nstrips + 1) regions of 16-B granules, zeroed once
size_t sor_granule_bytes(int dimx, int dimy);
// in-place Gauss-Seidel SOR sweep (OpticalFlowFluid.cpp:7-41), wavefront-exact,
// on the skewed vb (v and b halves per row, sor_rows rows of 16 P bytes).
// epoch: > every earlier epoch on H, the same epoch as the sor_pack before it;
// ticket: per-H counter, a multiple of nstrips before the launch.
void launch_sor(float4 *vb, int dimx, int dimy, int P, float mu, float lambda, float omega,
                void *H, unsigned epoch, unsigned *ticket, unsigned *status, hipStream_t st,
                FluidCtl ctl = {});
// vb's b <- force(u, dI, It); if v != nullptr also vb's v <- v; granule region
// 0 <- column 0 of v tagged with epoch
void launch_sor_pack(float4 *vb, const float2 *u, const float2 *dI, const float *It,
                     const float2 *v, int dimx, int dimy, int P, void *H, unsigned epoch,
                     hipStream_t st);
// after a regrid: dI, It <- gradients of Iaux (set_derivatives) and vb's b <-
// force of a zero estimate, granule region 0 <- column 0 of v tagged epoch
void launch_regrid_pack(const float *Iref, const float *Iaux, float2 *dI, float *It, float4 *vb,
                        int dimx, int dimy, int P, void *H, unsigned epoch, hipStream_t st,
                        FluidCtl ctl = {});
void launch_force(const float2 *u, const float2 *dI, const float *It, float2 *f, int dimx,
                  int dimy, int P, hipStream_t st);
int increment_nblocks(int dimx, int dimy);
// the Fluid sweep with the increment behind it (fluid_kernels.hip SorInc): the
// sweep of launch_sor plus launch_increment's R, partials and scal in one
// launch (+ the timestep reduction).  ticket: 1 + nstrips words of the level
// (the sweep ticket, then per strip its last finished epoch), zero at
// allocation; ctr: 2 counters, zero at allocation.  Falls back to launch_sor
// + launch_increment where too few CUs are left for workers; with
// sor_increment_workers() == 0 (OF2D_SOR_NCONS=0) the caller runs those.
int sor_increment_workers();
// what launch_sor_increment does at this size on the current device: the
// worker workgroups of the fused launch, 0 for the fallback pair
int sor_increment_plan(int dimx, int dimy);
void launch_sor_increment(float4 *vb, int dimx, int dimy, int P, float mu, float lambda,
                          float omega, void *H, unsigned epoch, unsigned *ticket,
                          unsigned long long *ctr, const float2 *u, float2 *R, float *part,
                          float *scal, unsigned *status, hipStream_t st, FluidCtl ctl = {});
// R and scal[0] = maxabs(R), scal[1] = 0.65f / maxabs
void launch_increment(const float2 *u, const float4 *vel, float2 *R, int dimx, int dimy, int P,
                      float *part, float *scal, hipStream_t st, FluidCtl ctl = {});
// uo <- u + R dt (dt < 65) or u; Logger partials of uo against prev (against u
// when prev is null); per-block Jacobian minima of uo into jpart (their min:
// launch_fluid_report); vb's b <- force(uo) and granule region 0 tagged with
// `epoch` for the next sweep (fluid_kernels.hip fluid_step_kernel)
void launch_fluid_step(const float2 *u, const float2 *R, float2 *uo, const float2 *prev,
                       const float *scal, const float2 *dI, const float *It, float4 *vb, int dimx,
                       int dimy, int P, void *H, unsigned epoch, double *lpart, float *jpart,
                       hipStream_t st, FluidCtl ctl = {});
// Per-iteration report a kernel writes straight into host memory (fine-grained
// pinned, so no copy launches): the Fluid loop's Logger sums, maxabs, dt,
// min Jacobian and status word
struct FluidReport {
    double sums[2];
    float maxabs, dt, jmin;
    unsigned status;
    float seq[2];   // the reference's float Logger sums (exact mode)
    float err;      // the Logger error as the host computes it (logger_error)
    unsigned flags;  // kFluidBreak, kFluidRegrid; kFluidDone once written
};
constexpr unsigned kFluidBreak = 1u, kFluidRegrid = 2u, kFluidDone = 4u;
// The end of a Fluid iteration's device work: the nb Logger partial pairs
// reduced as launch_reduce_partials does (same order, same bits), the minimum
// of the nb Jacobian partials into scal[2], and {sums, scal[0..2], *status}
// written to the host-mapped FluidReport (one launch instead of reduce + min +
// three copies)
void launch_fluid_report(const double *lpart, int nb, const float *jpart, float *scal,
                         const unsigned *status, FluidReport *report, hipStream_t st);
// ... and the iteration's decisions on the device (ImageRegistrationFluid.cpp:
// 99-124): err from the exact float sums `seq` (the reference's Logger) or from
// the fp64 sums (seq null), the break (!fixed, err < 0.001f, it > 1: the stop
// word), the regrid (no break and min Jacobian < 0.5: kFluidRegridWord, and the
// motion index flips); the report carries them for the host's lines
void launch_fluid_report_decide(const double *lpart, int nb, const float *jpart, float *scal,
                                const float *seq, double npx, bool fixed, FluidReport *report,
                                hipStream_t st, FluidCtl ctl);
// the regrid of an iteration that decided one (kFluidRegridWord; a no-op
// otherwise): motion[mcur'] <- accumulate(motion[1 - mcur'], est) with mcur'
// the flipped index, Iaux <- warp2d(Imov, new motion); est is left as it is
// (the next iteration reads it as zero and as the Logger's prev)
void launch_regrid_if(float2 *m0, float2 *m1, const float2 *est, const float *Imov, float *Iaux,
                      int dimx, int dimy, int P, hipStream_t st, FluidCtl ctl);
void launch_logger(const float4 *vb, float2 *u, float2 *prev, int dimx, int dimy, int P,
                   double *partial, hipStream_t st);

}  // namespace of2d
