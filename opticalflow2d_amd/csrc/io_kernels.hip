// io_kernels.hip — device-resident boundary I/O for gfx950:
// a caller's strided device array <-> the library's pitched fields, the pair
// as grid dimension z so that one launch covers every pair of a batch.
//
//   pack           strided float | double image stack -> pitched float fields,
//                  (float) in[...]: Image::set_image (src/Image.cpp:15-29)
//   unpack image   pitched float fields -> strided float | double,
//                  (double) widening: Image::copy_image_to_input (:36-50)
//   unpack motion  pitched float2 fields -> strided float | double with a
//                  component stride (Motion::copy_motion_to_input's planar
//                  layout, src/Motion.cpp:23-39, or an interleaved [.., 2])
//   pack motion    the reverse, (float) of each component: a caller's field
//                  into the pitched float2 fields (the set_motion entries);
//                  and the host form's planar double fields from the staging
//                  buffer (planar_to_motion_kernel)
//
// The conversions are exact or a single rounding, so results are bit for bit
// those of the host boundary (d2f_kernel, f2d_kernel, motion_to_planar_kernel
// of field_kernels.hip).  Every offset into the caller's array is 64-bit.
//
// Two access patterns, chosen by the launches from the caller's strides:
//
// (a) rows, sx <= sy: x is the caller's faster axis, as it is the fields'.
//     64 x 4 pixels per block, lane = x on both sides, no LDS; coalesced on
//     both sides when sx == 1 (the boundary layout).
//
// (b) transposed, sx > sy: y is the caller's faster axis (a contiguous torch
//     [dimx, dimy] has sy == 1).  A 64 x 64 tile goes through LDS: on the
//     fields' side lane = x, on the caller's side lane = y, so both global
//     accesses run along their fast axis.  LDS banking (a wave's access is
//     served in two 32-lane halves; only lanes of one half conflict):
//       4-byte tile (images, float [64][S]): a row access is 32 consecutive
//         dwords per half, conflict-free for any S under the writes' bank rule
//         (dword address mod 32).  A column access is ds_read_b32 of dword
//         lane * S + c, bank (lane * S + c) mod 32: 32 distinct banks for
//         lane = 0..31 iff S is odd.  S = 64 would put every lane on bank
//         c mod 32 (32-way); S = 65 = one 4-byte element of padding gives bank
//         (lane + c) mod 32.
//       8-byte tile (motion, float2 [64][S]): a row write is ds_write_b64 of
//         64 consecutive dwords per half, each of the 32 banks twice, which is
//         the 256 bytes' two cycles and no more.  A column access is
//         ds_read_b64 of dwords 2 * (lane * S + c) and the next, banked mod 64
//         dwords: the even dwords 2 * (lane * S mod 32) + const are distinct
//         for lane = 0..31 iff S is odd, and with them the pairs cover all 64
//         banks once.  S = 65 = one 8-byte element of padding; rows stay
//         8-byte aligned (65 * 8 = 520 bytes).
//     No 16-byte tile: a double output is widened after the LDS read.
// Any other stride combination is correct through whichever pattern the rule
// picks, only not coalesced on the caller's side.  Partial tiles are guarded
// on both axes in both phases.
#include "of2d_device.h"

namespace of2d {

namespace {
constexpr int kBx = 64, kBy = 4;
constexpr int kTile = 64;        // pixels per tile edge of pattern (b)
constexpr int kTileS = kTile + 1;  // its LDS row stride in elements (above)

// the caller's element strides
struct IoStrides {
    long long p, x, y, c;
};
inline IoStrides strides_of(const DArrayView &a) { return {a.sp, a.sx, a.sy, a.sc}; }
inline dim3 grid_rows(int dx, int dy, int np) {
    return dim3((dx + kBx - 1) / kBx, (dy + kBy - 1) / kBy, np);
}
inline dim3 grid_tiles(int dx, int dy, int np) {
    return dim3((dx + kTile - 1) / kTile, (dy + kTile - 1) / kTile, np);
}
// pattern (a) when x is the caller's faster axis
inline bool rows_pattern(const DArrayView &a) { return a.sx <= a.sy; }

template <class T>
struct Pair;
template <>
struct Pair<float> {
    using type = float2;
    static __device__ __forceinline__ float2 make(float2 v) { return v; }
    static __device__ __forceinline__ float2 narrow(float2 v) { return v; }
};
template <>
struct Pair<double> {
    using type = double2;
    static __device__ __forceinline__ double2 make(float2 v) {
        return make_double2((double)v.x, (double)v.y);
    }
    static __device__ __forceinline__ float2 narrow(double2 v) {
        return make_float2((float)v.x, (float)v.y);
    }
};
// both components of a motion vector; VEC2: sc == 1 and p aligned to the pair
template <class T, bool VEC2>
__device__ __forceinline__ void store_motion(T *p, long long sc, float2 v) {
    if constexpr (VEC2) {
        *reinterpret_cast<typename Pair<T>::type *>(p) = Pair<T>::make(v);
    } else {
        p[0] = (T)v.x;
        p[sc] = (T)v.y;
    }
}
// the same read, each component cast to float
template <class T, bool VEC2>
__device__ __forceinline__ float2 load_motion(const T *p, long long sc) {
    if constexpr (VEC2) {
        return Pair<T>::narrow(*reinterpret_cast<const typename Pair<T>::type *>(p));
    } else {
        return make_float2((float)p[0], (float)p[sc]);
    }
}

#define OF2D_IO_ROWS_PROLOGUE                             \
    const int i = blockIdx.x * kBx + threadIdx.x;         \
    const int j = blockIdx.y * kBy + threadIdx.y;         \
    const long long k = blockIdx.z;                       \
    if (i >= dimx || j >= dimy) return;
// a tile's origin; tx runs along the fast axis of the side being accessed
#define OF2D_IO_TILE_PROLOGUE                             \
    const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile; \
    const int tx = threadIdx.x, ty = threadIdx.y;         \
    const long long k = blockIdx.z;
}  // namespace

// ------------------------------------------------------------ pack
template <class T>
__global__ __launch_bounds__(kBx *kBy) void pack_rows_kernel(const T *__restrict__ in, IoStrides s,
                                                             int dimx, int dimy,
                                                             float *__restrict__ out, long so,
                                                             int P) {
    OF2D_IO_ROWS_PROLOGUE
    out[k * so + (long)j * P + i] = (float)in[k * s.p + i * s.x + j * s.y];
}

template <class T>
__global__ __launch_bounds__(kBx *kBy) void pack_tr_kernel(const T *__restrict__ in, IoStrides s,
                                                           int dimx, int dimy,
                                                           float *__restrict__ out, long so,
                                                           int P) {
    __shared__ float tile[kTile][kTileS];  // [x][y]
    OF2D_IO_TILE_PROLOGUE
    {
        const int y = y0 + tx;
        for (int xx = ty; xx < kTile; xx += kBy) {
            const int x = x0 + xx;
            if (x < dimx && y < dimy) tile[xx][tx] = (float)in[k * s.p + x * s.x + y * s.y];
        }
    }
    __syncthreads();
    const int x = x0 + tx;
    for (int yy = ty; yy < kTile; yy += kBy) {
        const int y = y0 + yy;
        if (x < dimx && y < dimy) out[k * so + (long)y * P + x] = tile[tx][yy];
    }
}

void launch_pack_image(const DArrayView &in, int npairs, int dimx, int dimy, float *out, long so,
                       int P, hipStream_t st) {
    const IoStrides s = strides_of(in);
    const bool rows = rows_pattern(in);
    const dim3 g = rows ? grid_rows(dimx, dimy, npairs) : grid_tiles(dimx, dimy, npairs);
    const dim3 b(kBx, kBy);
    if (in.f64) {
        const double *p = static_cast<const double *>(in.ptr);
        if (rows)
            hipLaunchKernelGGL(pack_rows_kernel<double>, g, b, 0, st, p, s, dimx, dimy, out, so, P);
        else
            hipLaunchKernelGGL(pack_tr_kernel<double>, g, b, 0, st, p, s, dimx, dimy, out, so, P);
    } else {
        const float *p = static_cast<const float *>(in.ptr);
        if (rows)
            hipLaunchKernelGGL(pack_rows_kernel<float>, g, b, 0, st, p, s, dimx, dimy, out, so, P);
        else
            hipLaunchKernelGGL(pack_tr_kernel<float>, g, b, 0, st, p, s, dimx, dimy, out, so, P);
    }
    OF2D_HIP(hipGetLastError());
}

// ------------------------------------------------------------ unpack image
template <class T>
__global__ __launch_bounds__(kBx *kBy) void unpack_image_rows_kernel(const float *__restrict__ in,
                                                                     long si, int P, int dimx,
                                                                     int dimy, T *__restrict__ out,
                                                                     IoStrides s) {
    OF2D_IO_ROWS_PROLOGUE
    out[k * s.p + i * s.x + j * s.y] = (T)in[k * si + (long)j * P + i];
}

template <class T>
__global__ __launch_bounds__(kBx *kBy) void unpack_image_tr_kernel(const float *__restrict__ in,
                                                                   long si, int P, int dimx,
                                                                   int dimy, T *__restrict__ out,
                                                                   IoStrides s) {
    __shared__ float tile[kTile][kTileS];  // [y][x]
    OF2D_IO_TILE_PROLOGUE
    {
        const int x = x0 + tx;
        for (int yy = ty; yy < kTile; yy += kBy) {
            const int y = y0 + yy;
            if (x < dimx && y < dimy) tile[yy][tx] = in[k * si + (long)y * P + x];
        }
    }
    __syncthreads();
    const int y = y0 + tx;
    for (int xx = ty; xx < kTile; xx += kBy) {
        const int x = x0 + xx;
        if (x < dimx && y < dimy) out[k * s.p + x * s.x + y * s.y] = (T)tile[tx][xx];
    }
}

void launch_unpack_image(const float *in, long si, int P, int npairs, int dimx, int dimy,
                         const DArrayView &out, hipStream_t st) {
    const IoStrides s = strides_of(out);
    const bool rows = rows_pattern(out);
    const dim3 g = rows ? grid_rows(dimx, dimy, npairs) : grid_tiles(dimx, dimy, npairs);
    const dim3 b(kBx, kBy);
    if (out.f64) {
        double *p = static_cast<double *>(out.ptr);
        if (rows)
            hipLaunchKernelGGL(unpack_image_rows_kernel<double>, g, b, 0, st, in, si, P, dimx, dimy,
                               p, s);
        else
            hipLaunchKernelGGL(unpack_image_tr_kernel<double>, g, b, 0, st, in, si, P, dimx, dimy,
                               p, s);
    } else {
        float *p = static_cast<float *>(out.ptr);
        if (rows)
            hipLaunchKernelGGL(unpack_image_rows_kernel<float>, g, b, 0, st, in, si, P, dimx, dimy,
                               p, s);
        else
            hipLaunchKernelGGL(unpack_image_tr_kernel<float>, g, b, 0, st, in, si, P, dimx, dimy,
                               p, s);
    }
    OF2D_HIP(hipGetLastError());
}

// ------------------------------------------------------------ unpack motion
template <class T, bool VEC2>
__global__ __launch_bounds__(kBx *kBy) void unpack_motion_rows_kernel(const float2 *__restrict__ m,
                                                                      long sm, int P, int dimx,
                                                                      int dimy, T *__restrict__ out,
                                                                      IoStrides s) {
    OF2D_IO_ROWS_PROLOGUE
    store_motion<T, VEC2>(out + (k * s.p + i * s.x + j * s.y), s.c, m[k * sm + (long)j * P + i]);
}

template <class T, bool VEC2>
__global__ __launch_bounds__(kBx *kBy) void unpack_motion_tr_kernel(const float2 *__restrict__ m,
                                                                    long sm, int P, int dimx,
                                                                    int dimy, T *__restrict__ out,
                                                                    IoStrides s) {
    __shared__ float2 tile[kTile][kTileS];  // [y][x]
    OF2D_IO_TILE_PROLOGUE
    {
        const int x = x0 + tx;
        for (int yy = ty; yy < kTile; yy += kBy) {
            const int y = y0 + yy;
            if (x < dimx && y < dimy) tile[yy][tx] = m[k * sm + (long)y * P + x];
        }
    }
    __syncthreads();
    const int y = y0 + tx;
    for (int xx = ty; xx < kTile; xx += kBy) {
        const int x = x0 + xx;
        if (x < dimx && y < dimy)
            store_motion<T, VEC2>(out + (k * s.p + x * s.x + y * s.y), s.c, tile[tx][xx]);
    }
}

namespace {
template <class T>
void launch_unpack_motion_t(const float2 *m, long sm, int P, int npairs, int dimx, int dimy,
                            const DArrayView &out, hipStream_t st) {
    const IoStrides s = strides_of(out);
    const bool rows = rows_pattern(out);
    const dim3 g = rows ? grid_rows(dimx, dimy, npairs) : grid_tiles(dimx, dimy, npairs);
    const dim3 b(kBx, kBy);
    T *p = static_cast<T *>(out.ptr);
    // one store of both components: they are adjacent and every vector's
    // address is a multiple of the pair's size
    const bool vec2 = s.c == 1 && reinterpret_cast<uintptr_t>(p) % (2 * sizeof(T)) == 0 &&
                      s.p % 2 == 0 && s.x % 2 == 0 && s.y % 2 == 0;
    if (rows && vec2)
        hipLaunchKernelGGL((unpack_motion_rows_kernel<T, true>), g, b, 0, st, m, sm, P, dimx, dimy,
                           p, s);
    else if (rows)
        hipLaunchKernelGGL((unpack_motion_rows_kernel<T, false>), g, b, 0, st, m, sm, P, dimx,
                           dimy, p, s);
    else if (vec2)
        hipLaunchKernelGGL((unpack_motion_tr_kernel<T, true>), g, b, 0, st, m, sm, P, dimx, dimy,
                           p, s);
    else
        hipLaunchKernelGGL((unpack_motion_tr_kernel<T, false>), g, b, 0, st, m, sm, P, dimx, dimy,
                           p, s);
    OF2D_HIP(hipGetLastError());
}
}  // namespace

void launch_unpack_motion(const float2 *m, long sm, int P, int npairs, int dimx, int dimy,
                          const DArrayView &out, hipStream_t st) {
    if (out.f64)
        launch_unpack_motion_t<double>(m, sm, P, npairs, dimx, dimy, out, st);
    else
        launch_unpack_motion_t<float>(m, sm, P, npairs, dimx, dimy, out, st);
}

// ------------------------------------------------------------ pack motion
// unpack motion's mirror: only the fields' pixels are written (the ghost
// j-lines and the pitch's slack keep their zeros)
template <class T, bool VEC2>
__global__ __launch_bounds__(kBx *kBy) void pack_motion_rows_kernel(const T *__restrict__ in,
                                                                    IoStrides s, int dimx,
                                                                    int dimy,
                                                                    float2 *__restrict__ m,
                                                                    long sm, int P) {
    OF2D_IO_ROWS_PROLOGUE
    m[k * sm + (long)j * P + i] = load_motion<T, VEC2>(in + (k * s.p + i * s.x + j * s.y), s.c);
}

template <class T, bool VEC2>
__global__ __launch_bounds__(kBx *kBy) void pack_motion_tr_kernel(const T *__restrict__ in,
                                                                  IoStrides s, int dimx, int dimy,
                                                                  float2 *__restrict__ m, long sm,
                                                                  int P) {
    __shared__ float2 tile[kTile][kTileS];  // [x][y]: row writes, column reads (above)
    OF2D_IO_TILE_PROLOGUE
    {
        const int y = y0 + tx;
        for (int xx = ty; xx < kTile; xx += kBy) {
            const int x = x0 + xx;
            if (x < dimx && y < dimy)
                tile[xx][tx] = load_motion<T, VEC2>(in + (k * s.p + x * s.x + y * s.y), s.c);
        }
    }
    __syncthreads();
    const int x = x0 + tx;
    for (int yy = ty; yy < kTile; yy += kBy) {
        const int y = y0 + yy;
        if (x < dimx && y < dimy) m[k * sm + (long)y * P + x] = tile[tx][yy];
    }
}

namespace {
template <class T>
void launch_pack_motion_t(const DArrayView &in, int npairs, int dimx, int dimy, float2 *m, long sm,
                          int P, hipStream_t st) {
    const IoStrides s = strides_of(in);
    const bool rows = rows_pattern(in);
    const dim3 g = rows ? grid_rows(dimx, dimy, npairs) : grid_tiles(dimx, dimy, npairs);
    const dim3 b(kBx, kBy);
    const T *p = static_cast<const T *>(in.ptr);
    // one load of both components, under launch_unpack_motion_t's conditions
    const bool vec2 = s.c == 1 && reinterpret_cast<uintptr_t>(p) % (2 * sizeof(T)) == 0 &&
                      s.p % 2 == 0 && s.x % 2 == 0 && s.y % 2 == 0;
    if (rows && vec2)
        hipLaunchKernelGGL((pack_motion_rows_kernel<T, true>), g, b, 0, st, p, s, dimx, dimy, m,
                           sm, P);
    else if (rows)
        hipLaunchKernelGGL((pack_motion_rows_kernel<T, false>), g, b, 0, st, p, s, dimx, dimy, m,
                           sm, P);
    else if (vec2)
        hipLaunchKernelGGL((pack_motion_tr_kernel<T, true>), g, b, 0, st, p, s, dimx, dimy, m, sm,
                           P);
    else
        hipLaunchKernelGGL((pack_motion_tr_kernel<T, false>), g, b, 0, st, p, s, dimx, dimy, m, sm,
                           P);
    OF2D_HIP(hipGetLastError());
}
}  // namespace

void launch_pack_motion(const DArrayView &in, int npairs, int dimx, int dimy, float2 *m, long sm,
                        int P, hipStream_t st) {
    if (in.f64)
        launch_pack_motion_t<double>(in, npairs, dimx, dimy, m, sm, P, st);
    else
        launch_pack_motion_t<float>(in, npairs, dimx, dimy, m, sm, P, st);
}

// The host form, motion_to_planar_kernel's mirror: npairs planar double fields
// (x-plane, then y-plane, x fastest: Motion::copy_motion_to_input's layout)
// from the staging buffer into the pitched float2 fields
__global__ __launch_bounds__(kBx *kBy) void planar_to_motion_kernel(const double *__restrict__ in,
                                                                    int dimx, int dimy,
                                                                    float2 *__restrict__ m,
                                                                    long sm, int P) {
    OF2D_IO_ROWS_PROLOGUE
    const long long n = (long long)dimx * dimy, q = k * 2 * n + (long long)j * dimx + i;
    m[k * sm + (long)j * P + i] = make_float2((float)in[q], (float)in[q + n]);
}

void launch_planar_to_motion(const double *in, int npairs, int dimx, int dimy, float2 *m, long sm,
                             int P, hipStream_t st) {
    hipLaunchKernelGGL(planar_to_motion_kernel, grid_rows(dimx, dimy, npairs), dim3(kBx, kBy), 0,
                       st, in, dimx, dimy, m, sm, P);
    OF2D_HIP(hipGetLastError());
}

}  // namespace of2d
