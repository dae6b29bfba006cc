"""Host-side mirror of the reference's operator interface.

* :class:`Regularisation`, :class:`Verbose`, :class:`MotionAccumulation` —
  ``src/SolverOptions.h:4-8`` with the same integer values.
* :func:`OpticalFlow2d` — the MEX entry point ``OpticalFlow2d(...)`` with the
  five call modes of ``WrapperOpticalFlow2d.cpp:23-151`` (keyed on nargout /
  nargin and whether the process-global singleton exists), routed through the
  C-ABI gateway ``of2d_gateway`` of libof2d.so.
* :class:`ImageRegistration` — an object-style handle on the same C-ABI
  (``of2d_create`` ... ``of2d_destroy``) for callers that want more than one
  registration per process.

Arrays follow MATLAB's convention used by the reference: an image is
``[dimx, dimy]`` in Fortran (column-major, x fastest) order and a motion field
is ``[dimx, dimy, 2]``.
"""
from __future__ import annotations

import ctypes as C
import enum
import threading
from typing import Callable, Optional, Sequence

import numpy as np

from . import _device, _lib
from ._lib import Of2dError, check


class Regularisation(enum.IntEnum):
    Diffusion = 0
    Curvature = 1
    Elastic = 2
    ThirionsDemons = 3
    DiffeomorphicDemons = 4
    Fluid = 5


class Verbose(enum.IntEnum):
    Off = 0
    On = 1


class MotionAccumulation(enum.IntEnum):
    Composition = 0
    Addition = 1


# ------------------------------------------------------------------ printing
_print_lock = threading.Lock()
_print_sink: Optional[Callable[[str], None]] = None
_print_cb = None


def set_print_sink(fn: Optional[Callable[[str], None]]) -> None:
    """Redirect the reference's mexPrintf text (banner, Logger and Fluid lines).
    ``None`` restores stdout."""
    global _print_sink, _print_cb
    L = _lib.lib()
    with _print_lock:
        _print_sink = fn
        if fn is None:
            _print_cb = None
            L.of2d_set_print_hook(_lib.PRINT_FN(), None)
        else:
            def _cb(text, _user):
                _print_sink(text.decode(errors="replace"))

            _print_cb = _lib.PRINT_FN(_cb)
            L.of2d_set_print_hook(_print_cb, None)


def _col(a, n: int) -> np.ndarray:
    """Column-major double copy of an array (the reference reads mxGetPr)."""
    v = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, order="F"))
    if v.size < n:
        raise ValueError(f"array has {v.size} elements, expected {n}")
    return v


def _vec(a) -> np.ndarray:
    return np.ascontiguousarray(np.atleast_1d(np.asarray(a, dtype=np.float64)).reshape(-1))


def _f32(a, shape=None) -> np.ndarray:
    """A contiguous float32 array for an entry on host arrays (of ``shape``)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"array is {a.shape}, expected {tuple(shape)}")
    return a


def _call(name, *args) -> None:
    """An entry without a context: its message is the gateway's last error."""
    L = _lib.lib()
    check(getattr(L, name)(*args), L.of2d_gateway_last_error().decode())


# ------------------------------------------------------------------ gateway
def OpticalFlow2d(*args, nargout: int = 0):
    """The MEX function, mode for mode (WrapperOpticalFlow2d.cpp:23-151).

    ``OpticalFlow2d([dimx, dimy], niter, nscales, reg, params, nparams, nrefine, verbose)``
        initialise the process-global registration object (a ninth argument,
        not in the reference: the number of devices Horn-Schunck runs on);
    ``OpticalFlow2d(Iref, Imov)``      register (estimate motion);
    ``OpticalFlow2d(nargout=1)``       return the motion field ``[dimx, dimy, 2]``;
    ``OpticalFlow2d(Imov, nargout=1)`` return Imov warped by the motion;
    ``OpticalFlow2d()``                close.
    Any other combination raises, like ``mexErrMsgTxt``.  The reference reads
    its inputs with ``mxGetPr`` unchecked; here short arrays are refused before
    they reach the library.
    """
    L = _lib.lib()
    nrhs = len(args)
    keep = [np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, order="F"))
            for a in args]
    n_img = int(L.of2d_gateway_output_numel(1, 1))  # 0 when no singleton exists
    if nargout == 0 and nrhs in (8, 9) and n_img == 0:
        nscales = int(keep[2][0]) if keep[2].size else 0
        nparams = int(keep[5][0]) if keep[5].size else 0
        if keep[0].size < 2 or keep[1].size < nscales + 1 or keep[4].size < nparams:
            raise ValueError("init: [dimx dimy], niter (nscales+1) and params (nparams) sizes")
    elif n_img and ((nargout == 0 and nrhs == 2) or (nargout == 1 and nrhs == 1)):
        if any(v.size < n_img for v in keep):
            raise ValueError(f"images must have {n_img} elements")
    prhs = (C.c_void_p * max(nrhs, 1))(*[v.ctypes.data for v in keep])
    plhs = (C.c_void_p * max(nargout, 1))()
    out = shape = None
    if nargout == 1:
        dims = (C.c_size_t * 3)()
        nd = C.c_int(0)
        if L.of2d_gateway_output_dims(1, nrhs, dims, C.byref(nd)) == _lib.OF2D_OK:
            shape = tuple(int(dims[i]) for i in range(nd.value))
            out = np.zeros(int(np.prod(shape)), np.float64)
            plhs[0] = out.ctypes.data
    st = L.of2d_gateway(nargout, plhs, nrhs, prhs)
    check(st, L.of2d_gateway_last_error().decode())
    if out is not None:
        return out.reshape(shape, order="F")
    return None


# ------------------------------------------------------------------ option limits
#: line lengths the fast transforms take (powers of two; include/of2d.h)
DCT_NMIN, DCT_NMAX = 8, 8192
# the widest Demons kernel "demons_separable" takes (include/of2d.h OF2D_SEP_KW_MAX)
SEP_KW_MAX = 15


# ------------------------------------------------------------------ deformation analysis
#: updates of the inverse enqueued between the host's reads (include/of2d.h)
INVERT_CHUNK = 8


def _jac_stats(st) -> dict:
    return {"min": float(st[0]), "max": float(st[1]), "mean": float(st[2]),
            "folded": int(st[3]), "below_half": int(st[4])}


def _invert_info(info) -> dict:
    return {"iterations": int(info[0]), "residual": float(info[1]),
            "out_of_bounds": int(info[2]), "converged": bool(info[3])}


def _invert_args(max_iter, tol):
    max_iter, tol = int(max_iter), float(tol)
    if max_iter < 1:
        raise ValueError("max_iter must be >= 1")
    if not np.isfinite(tol) or tol <= 0:
        raise ValueError("tol must be finite and > 0")
    return max_iter, tol


class field:
    """Deformation analysis of a motion field on the device (include/of2d.h,
    "deformation analysis"): the Jacobian determinant map, the inverse field
    and the similarity of two images.  Arrays are float32 in the C-ABI's own
    layout: an image ``[dimy, dimx]`` and a motion field ``[dimy, dimx, 2]`` in
    C order (idx = i + j*dimx, x and y interleaved)."""

    @staticmethod
    def _motion(u):
        u = _f32(u)
        if u.ndim != 3 or u.shape[2] != 2:
            raise ValueError(f"a motion field is [dimy, dimx, 2], got {u.shape}")
        if u.shape[0] < 2 or u.shape[1] < 2:
            raise ValueError("the field needs dimx >= 2 and dimy >= 2")
        return u

    @classmethod
    def jacobian(cls, u, jac=True):
        """``(jac [dimy, dimx], stats)``: the reference's Jacobian determinant
        of ``id + u`` and ``stats = {min, max, mean, folded (J <= 0),
        below_half (J < 0.5)}``; ``jac=False`` takes the statistics only and
        returns ``(None, stats)``."""
        u = cls._motion(u)
        dimy, dimx, _ = u.shape
        out = np.zeros((dimy, dimx), np.float32) if jac else None
        st = np.zeros(5, np.float64)
        _call("of2d_field_jacobian", u, dimx, dimy, out.ctypes.data if jac else None, st)
        return out, _jac_stats(st)

    @classmethod
    def invert(cls, u, max_iter=50, tol=1e-3):
        """``(v, info, residuals)`` with ``(id + u) o (id + v) = id``: the
        fixed-point iteration of of2d_field_invert.  ``info = {iterations,
        residual, out_of_bounds, converged}``; ``residuals`` (float32
        ``[iterations]``) holds max |r_k| of every update applied."""
        u = cls._motion(u)
        max_iter, tol = _invert_args(max_iter, tol)
        dimy, dimx, _ = u.shape
        v = np.zeros_like(u)
        info = np.zeros(4, np.float64)
        res = np.zeros(max_iter, np.float32)
        _call("of2d_field_invert", u, dimx, dimy, max_iter, tol, v, info, res.ctypes.data)
        info = _invert_info(info)
        return v, info, res[: info["iterations"]].copy()

    @classmethod
    def similarity(cls, a, b):
        """``(mse, ncc)`` of two images; ``ncc`` is NaN when one is constant."""
        a = _f32(a)
        if a.ndim != 2 or a.size == 0:
            raise ValueError(f"an image is [dimy, dimx], got {a.shape}")
        b = _f32(b, a.shape)
        out = np.zeros(2, np.float64)
        _call("of2d_image_similarity", a, b, a.shape[1], a.shape[0], out)
        return float(out[0]), float(out[1])


# ------------------------------------------------------------------ object API
class ImageRegistration:
    """Handle on one registration context (of2d_create ... of2d_destroy).

    Parameters mirror the init call: ``dims=(dimx, dimy)``, ``niter`` (nscales+1
    values, finest level first), ``nscales``, ``reg``, ``params`` (nparams
    floats), ``nrefine``, ``verbose``.  Extra keyword options map to
    ``of2d_set_option`` (``fixed_iters``, ``chunk``, ``device``,
    ``hs_gradients_from_image``, ``logger_fp64``, ``ngpus``,
    ``curvature_dct``, ``demons_separable``).
    """

    def __init__(self, dims: Sequence[int], niter: Sequence[int], nscales: int, reg: int,
                 params: Sequence[float], nrefine: int = 1, verbose: int = 0, **options):
        L = _lib.lib()
        self.dimx, self.dimy = int(dims[0]), int(dims[1])
        nit = np.ascontiguousarray(np.asarray(niter, dtype=np.int32).reshape(-1)[: nscales + 1])
        if nit.size < nscales + 1:
            raise ValueError("niter needs nscales+1 entries")
        p = np.ascontiguousarray(np.asarray(params, dtype=np.float32).reshape(-1))
        npar = int(p.size)
        if npar == 0:
            p = np.zeros(1, np.float32)
        h = C.c_void_p()
        st = L.of2d_create(C.byref(h), self.dimx, self.dimy, nit, int(nscales), int(reg), p,
                           npar, int(nrefine), int(verbose))
        check(st, L.of2d_last_error(None).decode())
        self._h = h
        self._device = None  # option "device": where motion_device allocates
        for k, v in options.items():
            self.set_option(k, v)

    def _chk(self, st):
        check(st, _lib.lib().of2d_last_error(self._h).decode())

    def set_option(self, key: str, value: float) -> None:
        self._chk(_lib.lib().of2d_set_option(self._h, key.encode(), float(value)))
        if key == "device":
            self._device = int(value)

    def register(self, Iref, Imov) -> None:
        self.set_images(Iref, Imov)
        self.estimate()

    def set_images(self, Iref, Imov) -> None:
        """Upload the image pair (the first half of register).  Two torch CUDA
        tensors ``[dimx, dimy]`` (float32 or float64, any strides) are read
        where they are, in the order of their device's current stream
        (of2d_set_images_device); mixing one with a host array is a
        ``ValueError``."""
        if _device.all_cuda(Iref=Iref, Imov=Imov):
            shape, axes = (self.dimx, self.dimy), (1, 2)
            r = _device.darray(Iref, shape, axes, "Iref")
            m = _device.darray(Imov, shape, axes, "Imov")
            self._chk(_lib.lib().of2d_set_images_device(self._h, C.byref(r), C.byref(m),
                                                        _device.stream_of(Imov)))
            return
        n = self.dimx * self.dimy
        r, m = _col(Iref, n), _col(Imov, n)
        self._chk(_lib.lib().of2d_set_images(self._h, r, m))

    def estimate(self) -> None:
        """Run the pyramid on the images already on the device."""
        self._chk(_lib.lib().of2d_estimate(self._h))

    def motion(self) -> np.ndarray:
        out = np.zeros(self.dimx * self.dimy * 2, np.float64)
        self._chk(_lib.lib().of2d_get_motion(self._h, out))
        return out.reshape((self.dimx, self.dimy, 2), order="F")

    def motion_device(self, dtype=None, out=None):
        """The motion as a CUDA tensor ``[dimx, dimy, 2]`` of ``dtype``
        (``torch.float32``, the default, or ``torch.float64``), or written into
        ``out`` (a CUDA tensor of that shape, any strides), in the order of the
        device's current stream (of2d_get_motion_device)."""
        shape = (self.dimx, self.dimy, 2)
        out = _device.output(out, shape, dtype, self._device)
        a = _device.darray(out, shape, (1, 2, 3), "out")
        self._chk(_lib.lib().of2d_get_motion_device(self._h, C.byref(a), _device.stream_of(out)))
        return out

    def set_motion(self, m) -> None:
        """Replace the motion by ``m``: a numpy array ``[dimx, dimy, 2]``
        (of2d_set_motion) or a CUDA tensor of that shape, float32 or float64,
        any strides (of2d_set_motion_device).  Values are cast to float32.
        :meth:`motion`, :meth:`warp` and the analysis see it at once, and the
        next :meth:`estimate` continues from it at every pyramid level, as it
        continues from its own last result."""
        shape = (self.dimx, self.dimy, 2)
        if _device.is_cuda(m):
            a = _device.darray(m, shape, (1, 2, 3), "motion")
            self._chk(_lib.lib().of2d_set_motion_device(self._h, C.byref(a),
                                                        _device.stream_of(m)))
            return
        m = np.asarray(m, dtype=np.float64)
        if m.shape != shape:
            raise ValueError(f"motion is {m.shape}, expected {shape}")
        buf = np.ascontiguousarray(m.reshape(-1, order="F"))
        self._chk(_lib.lib().of2d_set_motion(self._h, buf.ctypes.data))

    def reset_motion(self) -> None:
        """The motion of every level back to zero (Fluid: the velocity too):
        the next :meth:`estimate` gives a new object's result."""
        self._chk(_lib.lib().of2d_reset_motion(self._h))

    def warp(self, Imov, out=None):
        """``Imov`` warped by the current motion.  A CUDA tensor gives a CUDA
        tensor of its dtype, or ``out`` (of2d_warp_device)."""
        if _device.all_cuda(**({"Imov": Imov} if out is None else {"Imov": Imov, "out": out})):
            shape, axes = (self.dimx, self.dimy), (1, 2)
            m = _device.darray(Imov, shape, axes, "Imov")
            out = _device.output(out, shape, Imov.dtype, Imov.device)
            o = _device.darray(out, shape, axes, "out")
            self._chk(_lib.lib().of2d_warp_device(self._h, C.byref(m), C.byref(o),
                                                  _device.stream_of(Imov)))
            return out
        if out is not None:
            raise ValueError("out= is for CUDA tensors")
        n = self.dimx * self.dimy
        m = _col(Imov, n)
        out = np.zeros(n, np.float64)
        self._chk(_lib.lib().of2d_warp(self._h, m, out))
        return out.reshape((self.dimx, self.dimy), order="F")

    def jacobian(self, jac: bool = True):
        """``(jac [dimx, dimy], stats)`` of the current motion, on the device
        (of2d_jacobian): the Jacobian determinant map and ``{min, max, mean,
        folded, below_half}``; ``jac=False``: ``(None, stats)``."""
        n = self.dimx * self.dimy
        out = np.zeros(n, np.float64) if jac else None
        st = np.zeros(5, np.float64)
        self._chk(_lib.lib().of2d_jacobian(self._h, out.ctypes.data if jac else None, st))
        return (out.reshape((self.dimx, self.dimy), order="F") if jac else None), _jac_stats(st)

    def inverse_motion(self, max_iter: int = 50, tol: float = 1e-3):
        """``(motion [dimx, dimy, 2], info)``: the inverse of the current
        motion (of2d_invert_motion), ``info`` as :meth:`field.invert`'s."""
        max_iter, tol = _invert_args(max_iter, tol)
        out = np.zeros(self.dimx * self.dimy * 2, np.float64)
        info = np.zeros(4, np.float64)
        self._chk(_lib.lib().of2d_invert_motion(self._h, max_iter, tol, out, info))
        return out.reshape((self.dimx, self.dimy, 2), order="F"), _invert_info(info)

    def quality(self, Iref, Imov) -> dict:
        """MSE and zero-mean NCC of ``Iref`` against ``Imov`` and against
        ``Imov`` warped by the current motion (of2d_quality): ``{mse_before,
        ncc_before, mse_after, ncc_after}``."""
        n = self.dimx * self.dimy
        r, m = _col(Iref, n), _col(Imov, n)
        if r.size != n or m.size != n:
            raise ValueError(f"images must have {n} elements")
        out = np.zeros(4, np.float64)
        self._chk(_lib.lib().of2d_quality(self._h, r, m, out))
        return dict(zip(("mse_before", "ncc_before", "mse_after", "ncc_after"),
                        (float(v) for v in out)))

    def iterations(self) -> list:
        buf = np.zeros(4096, np.int32)
        n = _lib.lib().of2d_iterations_executed(self._h, buf, buf.size)
        return buf[: max(n, 0)].tolist()

    def last_errors(self) -> np.ndarray:
        buf = np.zeros(1 << 16, np.float32)
        n = _lib.lib().of2d_last_errors(self._h, buf, buf.size)
        return buf[: max(n, 0)].copy()

    def curvature_paths(self) -> list:
        """``(dimx, dimy, fast_x, fast_y)`` per Curvature loop of the last
        estimate, in execution order (of2d_curvature_paths)."""
        buf = np.zeros(4 * 1024, np.int32)
        n = _lib.lib().of2d_curvature_paths(self._h, buf, buf.size)
        return [tuple(int(v) for v in buf[4 * k: 4 * k + 4]) for k in range(max(n, 0))]

    def demons_paths(self) -> list:
        """``(dimx, dimy, kw, separable)`` per Demons loop of the last
        estimate, in execution order (of2d_demons_paths)."""
        buf = np.zeros(4 * 1024, np.int32)
        n = _lib.lib().of2d_demons_paths(self._h, buf, buf.size)
        return [tuple(int(v) for v in buf[4 * k: 4 * k + 4]) for k in range(max(n, 0))]

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.lib().of2d_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def __getattr__(name):  # the test entries' wrappers moved to prims.py: old imports still work
    if name in ("motion_norms", "motion_norms_chain", "dct2d", "prim"):
        from . import prims
        return getattr(prims, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["Regularisation", "Verbose", "MotionAccumulation", "OpticalFlow2d",
           "ImageRegistration", "set_print_sink", "Of2dError", "field", "INVERT_CHUNK"]
