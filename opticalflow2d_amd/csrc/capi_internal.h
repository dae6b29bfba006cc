// capi_internal.h — shared by capi.cpp (include/of2d.h, the product) and
// capi_prims.cpp (of2d_prims.h, the test entries).  One error channel: an entry
// without a context leaves its message where of2d_gateway_last_error reads it.
#pragma once

#include <initializer_list>
#include <string>

#include "../../include/of2d.h"
#include "of2d_host.h"

namespace of2d {
namespace capi {

// the calling thread's gateway error string (capi.cpp)
void set_gateway_error(const std::string &msg);
// a refusal before any device work, with its reason for of2d_gateway_last_error
// (and of2d_last_error of the context, where there is one)
int refuse(of2d_ctx *ctx, const char *why);

template <class F>
int guarded(std::string &err, F &&f) {
    try {
        f();
        err.clear();
        return OF2D_OK;
    } catch (const std::invalid_argument &e) {
        err = e.what();
        return OF2D_ERR_INVALID_ARGUMENT;
    } catch (const of2d::DeviceError &e) {
        err = e.what();
        return OF2D_ERR_DEVICE;
    } catch (const std::exception &e) {
        err = e.what();
        return OF2D_ERR_RUNTIME;
    } catch (...) {
        err = "unknown error";
        return OF2D_ERR_RUNTIME;
    }
}
// an entry on host arrays, without a context
template <class F>
int prim(bool args_ok, F &&f) {
    if (!args_ok) return OF2D_ERR_INVALID_ARGUMENT;
    std::string err;
    const int rc = guarded(err, f);
    if (rc != OF2D_OK) set_gateway_error(err);
    return rc;
}

// dense host rows of dimx elements of T <-> a pitched device array (P elements
// a row); the download waits for the null stream's launches first
template <class T>
void upload(T *dev, int P, const void *host, int dimx, int dimy) {
    const size_t row = (size_t)dimx * sizeof(T);
    OF2D_HIP(hipMemcpy2D(dev, (size_t)P * sizeof(T), host, row, row, dimy, hipMemcpyHostToDevice));
}
template <class T>
void download(void *host, const T *dev, int P, int dimx, int dimy) {
    const size_t row = (size_t)dimx * sizeof(T);
    OF2D_HIP(hipStreamSynchronize(nullptr));
    OF2D_HIP(hipMemcpy2D(host, row, dev, (size_t)P * sizeof(T), row, dimy, hipMemcpyDeviceToHost));
}
// a zeroed pitched field holding the dense host array (none: zeros)
template <class T>
void upload(of2d::Field<T> &f, const float *host, int dimx, int dimy) {
    f.alloc(dimx, dimy);
    if (host) upload(f.p, f.P, host, dimx, dimy);
}
// n device elements, after the null stream's launches
template <class T>
void fetch(T *host, const T *dev, size_t n) {
    OF2D_HIP(hipStreamSynchronize(nullptr));
    OF2D_HIP(hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost));
}

// ---- of2d_darray arguments (defined in capi.cpp)
// the axes of a call's array: pair, x, y, component (0: the axis is not used)
struct Extents {
    int n[4];
};
// an entry's arrays, checked in order; the first refusal is the message
struct DArrayArg {
    const of2d_darray *a;
    const char *name;
    bool output;
    Extents e;
};
// "" or "<fn>: why the first bad array is refused"; no device work.  Unused
// axes' strides are not looked at.
std::string first_refusal(const char *fn, std::initializer_list<DArrayArg> args);
of2d::DArrayView view_of(const of2d_darray *a, const Extents &e);

}  // namespace capi
}  // namespace of2d
