"""Batched Horn-Schunck, Curvature, Elastic, Fluid and Thirion's Demons: many
small image pairs of one size in one call.

:class:`BatchRegistration` is the object-style handle on ``of2d_batch_*``
(include/of2d.h): ``nbatch`` independent Diffusion, Curvature, Elastic, Fluid or Thirion's Demons
registrations with the same parameters, each run by one workgroup with the
whole iteration loop inside the kernel.  Arrays follow :class:`ImageRegistration`'s convention with a leading
pair axis: an image is ``[dimx, dimy]`` (x first), a stack of them
``[nbatch, dimx, dimy]`` and the motion ``[nbatch, dimx, dimy, 2]``.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _device, _lib
from ._lib import check
from .registration import Regularisation, _invert_args, _invert_info, _jac_stats

#: most pixels a batch image may have (include/of2d.h OF2D_BATCH_MAXPX)
BATCH_MAXPX = 512 * 512


class BatchRegistration:
    """``nbatch`` registrations of ``dims = (dimx, dimy)`` images.

    ``niter`` (nscales+1 values, finest level first), ``nscales``, ``alpha``
    and ``nrefine`` are :class:`ImageRegistration`'s.  ``reg`` is
    ``Regularisation.Diffusion`` (the default; ``alpha`` is Horn-Schunck's one
    parameter), ``Regularisation.Curvature`` (1; ``alpha`` is ``[alpha]`` with
    tau = 1 or ``[alpha, tau]``, and both sides of every pyramid level must be
    powers of two from 8 to 512: per pair the one-pair ``curvature_dct=1``
    registration, bit for bit with ``fixed_iters=1``),
    ``Regularisation.Elastic`` (2; ``alpha`` is ``[mu, lambda, omega]``, or
    ``[mu, lambda]``, to which this class appends the reference's default
    omega ``np.float32(0.66)`` itself: ``of2d_batch_create`` takes the three
    only; per pair the one-pair Elastic registration, bit for bit with
    ``fixed_iters=1``, at any size the batch takes),
    ``Regularisation.Fluid`` (5; ``alpha`` as Elastic's, the default omega
    ``np.float32(0.66)`` appended likewise: the class creates the Elastic
    handle, sets its option ``fluid=1`` and keeps ``reg == 5``; ``reg=2,
    fluid=1`` is the same handle; every pyramid level needs sides of at least
    2; per pair the one-pair Fluid registration with its regrids, bit for bit
    with ``fixed_iters=1``; the batch prints nothing, :meth:`fluid_log` and
    :meth:`fluid_lines` give the reference's Dumax / Regridding lines) or
    ``Regularisation.ThirionsDemons`` (3), for which ``alpha``
    carries the one-pair path's six parameters ``[sigma_i, sigma_x,
    sigma_diffusion, sigma_fluid, kernel_width, accumulation]``; every other
    method is refused.  The other keyword options map to
    ``of2d_batch_set_option``: ``fixed_iters``, ``device``, ``diffeomorphic``,
    ``fluid``, ``warm_start``, ``resident``, ``conv_lds``.  ``resident=1`` (Diffusion only, refused with
    ``InvalidArgument`` otherwise) keeps a pair's iterate in LDS and its
    gradients in registers across the iterations at every pyramid level that
    fits (all up to 128 x 128; :meth:`info` reports ``placement`` 1 there);
    results are those of the default 0 bit for bit.  ``conv_lds=1`` (``reg=3``
    only, refused with ``InvalidArgument`` otherwise) keeps the field that the
    Demons loop's two convolutions read in LDS at every level that fits (all
    up to 128 x 128; ``placement`` 1), again with the bits of the default 0.
    ``warm_start=1`` (every method) makes :meth:`register`
    continue from the motion the handle holds, as a reused
    :class:`ImageRegistration` does, bit for bit per pair; see
    :meth:`set_motion` for a start from outside and for the pyramid's
    carry-over rule.  The default 0 starts every call from zero.
    ``diffeomorphic=1`` on a ``reg=3`` batch whose accumulation is 0
    (Composition) makes every pair the one-pair
    ``Regularisation.DiffeomorphicDemons`` (4) registration with the first five
    parameters, bit for bit: the smoothed correction goes through
    ``Motion::exp`` with the pair's own number of squarings.  It is refused
    (``InvalidArgument``) on any other batch; ``set_option("diffeomorphic", 0)``
    returns the next ``register`` to Thirion's Demons.
    With convergence on, every pair stops on its own iteration; the errors are
    those of ``logger_fp64=1`` (fp64 sums in a fixed order).
    """

    def __init__(self, nbatch: int, dims: Sequence[int], niter: Sequence[int], nscales: int,
                 alpha, nrefine: int = 1, *, reg: int = Regularisation.Diffusion, **options):
        L = _lib.lib()
        self.nbatch = int(nbatch)
        self.dimx, self.dimy = int(dims[0]), int(dims[1])
        self.nscales, self.nrefine = int(nscales), int(nrefine)
        self.reg = int(reg)
        nit = np.ascontiguousarray(np.asarray(niter, dtype=np.int32).reshape(-1)[: max(nscales, 0) + 1])
        if nit.size < nscales + 1:
            raise ValueError("niter needs nscales+1 entries")
        p = np.ascontiguousarray(np.asarray(alpha, dtype=np.float32).reshape(-1))
        # Fluid is the option "fluid" of an Elastic handle (include/of2d.h)
        create_reg = self.reg
        if self.reg == Regularisation.Fluid:
            create_reg = int(Regularisation.Elastic)
            options = dict(options, fluid=1)
        if create_reg == Regularisation.Elastic and p.size == 2:
            p = np.append(p, np.float32(0.66))  # OpticalFlowElastic.h:9, OpticalFlowFluid.h:10
        self._h = None
        h = C.c_void_p()
        st = L.of2d_batch_create(C.byref(h), self.nbatch, self.dimx, self.dimy, nit,
                                 self.nscales, create_reg,
                                 p if p.size else np.zeros(1, np.float32),
                                 int(p.size), self.nrefine)
        check(st, L.of2d_batch_last_error(None).decode())
        self._h = h
        self._device = None  # option "device": where motion_device allocates
        self.loops = (self.nscales + 1) * max(self.nrefine, 0)
        self._maxn = max(int(nit.max()), 1)  # a loop records at most niter errors
        try:
            for k, v in options.items():
                self.set_option(k, v)
        except Exception:
            self.close()
            raise

    def _chk(self, st):
        check(st, _lib.lib().of2d_batch_last_error(self._h).decode())

    def set_option(self, key: str, value: float) -> None:
        self._chk(_lib.lib().of2d_batch_set_option(self._h, key.encode(), float(value)))
        if key == "device":
            self._device = int(value)

    def _stack(self, a, name: str) -> np.ndarray:
        """``[nbatch, dimx, dimy]`` -> the boundary layout, x fastest per image."""
        a = np.asarray(a, dtype=np.float64)
        want = (self.nbatch, self.dimx, self.dimy)
        if a.shape != want:
            raise ValueError(f"{name} is {a.shape}, expected {want}")
        return np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(-1)

    def register(self, Iref, Imov) -> None:
        """``Iref``: ``[dimx, dimy]`` (one reference shared by every pair) or
        ``[nbatch, dimx, dimy]``; ``Imov``: ``[nbatch, dimx, dimy]``.  Two
        torch CUDA tensors (float32 or float64, any strides) are read where
        they are, in the order of their device's current stream
        (of2d_batch_set_images_device); mixing one with a host array is a
        ``ValueError``."""
        if _device.all_cuda(Iref=Iref, Imov=Imov):
            stack = (self.nbatch, self.dimx, self.dimy)
            shared = Iref.dim() == 2
            if shared:
                r = _device.darray(Iref, stack[1:], (1, 2), "Iref")
            elif tuple(Iref.shape) == stack:
                r = _device.darray(Iref, stack, (0, 1, 2), "Iref")
            else:
                raise ValueError(f"Iref is {tuple(Iref.shape)}, expected {stack[1:]} or {stack}")
            m = _device.darray(Imov, stack, (0, 1, 2), "Imov")
            L = _lib.lib()
            self._chk(L.of2d_batch_set_images_device(self._h, C.byref(r), int(shared), C.byref(m),
                                                     _device.stream_of(Imov)))
            self._chk(L.of2d_batch_estimate(self._h))
            return
        r = np.asarray(Iref, dtype=np.float64)
        shared = r.ndim == 2
        if shared:
            if r.shape != (self.dimx, self.dimy):
                raise ValueError(f"Iref is {r.shape}, expected {(self.dimx, self.dimy)} or "
                                 f"{(self.nbatch, self.dimx, self.dimy)}")
            r = np.ascontiguousarray(r.T).reshape(-1)
        else:
            r = self._stack(r, "Iref")
        m = self._stack(Imov, "Imov")
        L = _lib.lib()
        self._chk(L.of2d_batch_set_images(self._h, r, int(shared), m))
        self._chk(L.of2d_batch_estimate(self._h))

    def motion(self) -> np.ndarray:
        out = np.zeros(self.nbatch * 2 * self.dimx * self.dimy, np.float64)
        self._chk(_lib.lib().of2d_batch_get_motion(self._h, out))
        return np.ascontiguousarray(
            out.reshape(self.nbatch, 2, self.dimy, self.dimx).transpose(0, 3, 2, 1))

    def motion_device(self, dtype=None, out=None):
        """The motion as a CUDA tensor ``[nbatch, dimx, dimy, 2]`` of ``dtype``
        (``torch.float32``, the default, or ``torch.float64``), or written into
        ``out`` (a CUDA tensor of that shape, any strides), in the order of the
        device's current stream (of2d_batch_get_motion_device)."""
        shape = (self.nbatch, self.dimx, self.dimy, 2)
        out = _device.output(out, shape, dtype, self._device)
        a = _device.darray(out, shape, (0, 1, 2, 3), "out")
        self._chk(_lib.lib().of2d_batch_get_motion_device(self._h, C.byref(a),
                                                          _device.stream_of(out)))
        return out

    def set_motion(self, m) -> None:
        """Replace every pair's motion by ``m``: a numpy array ``[nbatch, dimx,
        dimy, 2]`` (of2d_batch_set_motion) or a CUDA tensor of that shape,
        float32 or float64, any strides, read where it is in the order of its
        device's current stream (of2d_batch_set_motion_device).  Values are
        cast to float32.  :meth:`motion`, :meth:`warp` and the analysis see
        the field at once; with ``warm_start=1`` the next :meth:`register`
        starts from it at every pyramid level, with ``warm_start=0`` it is
        ignored.  ``b.set_motion(b.motion_device())`` makes a warm estimate
        with a pyramid continue from the full-resolution result (otherwise
        only the coarsest level's motion carries over)."""
        shape = (self.nbatch, self.dimx, self.dimy, 2)
        if _device.is_cuda(m):
            a = _device.darray(m, shape, (0, 1, 2, 3), "motion")
            self._chk(_lib.lib().of2d_batch_set_motion_device(self._h, C.byref(a),
                                                              _device.stream_of(m)))
            return
        m = np.asarray(m, dtype=np.float64)
        if m.shape != shape:
            raise ValueError(f"motion is {m.shape}, expected {shape}")
        buf = np.ascontiguousarray(m.transpose(0, 3, 2, 1))
        self._chk(_lib.lib().of2d_batch_set_motion(self._h, buf.ctypes.data))

    def reset_motion(self) -> None:
        """Every pair's motion back to zero at every level (Fluid: the velocity
        too): the next :meth:`register`, warm or not, gives a fresh handle's
        result."""
        self._chk(_lib.lib().of2d_batch_reset_motion(self._h))

    def warp(self, Imov, out=None):
        """Pair k's image warped by pair k's motion, ``[nbatch, dimx, dimy]``.
        A CUDA tensor gives a CUDA tensor of its dtype, or ``out``
        (of2d_batch_warp_device)."""
        if _device.all_cuda(**({"Imov": Imov} if out is None else {"Imov": Imov, "out": out})):
            shape, axes = (self.nbatch, self.dimx, self.dimy), (0, 1, 2)
            m = _device.darray(Imov, shape, axes, "Imov")
            out = _device.output(out, shape, Imov.dtype, Imov.device)
            o = _device.darray(out, shape, axes, "out")
            self._chk(_lib.lib().of2d_batch_warp_device(self._h, C.byref(m), C.byref(o),
                                                        _device.stream_of(Imov)))
            return out
        if out is not None:
            raise ValueError("out= is for CUDA tensors")
        m = self._stack(Imov, "Imov")
        out = np.zeros_like(m)
        self._chk(_lib.lib().of2d_batch_warp(self._h, m, out))
        return np.ascontiguousarray(
            out.reshape(self.nbatch, self.dimy, self.dimx).transpose(0, 2, 1))

    # ---- deformation analysis of every pair's motion (of2d_batch_jacobian,
    # _invert_motion, _quality): one or two launches whatever nbatch is.  The
    # statistics always come back as host values, so the calls wait for the
    # device.
    def jacobian(self, jac=True, out=None):
        """``(maps, stats)``: the Jacobian determinant map of every pair's
        motion, ``[nbatch, dimx, dimy]``, and a list of
        :meth:`ImageRegistration.jacobian`'s ``stats`` dicts.  ``jac=False``:
        ``(None, stats)``.  ``out`` (a CUDA tensor of the maps' shape, float32
        or float64, any strides) receives the maps on the device
        (of2d_batch_jacobian_device) and is returned."""
        L = _lib.lib()
        st = np.zeros((self.nbatch, 5), np.float64)
        maps = None
        if out is not None:
            shape = (self.nbatch, self.dimx, self.dimy)
            out = _device.output(out, shape, None, self._device)
            a = _device.darray(out, shape, (0, 1, 2), "out")
            self._chk(L.of2d_batch_jacobian_device(self._h, C.byref(a), st.ctypes.data,
                                                   _device.stream_of(out)))
            maps = out
        elif jac:
            buf = np.zeros(self.nbatch * self.dimx * self.dimy, np.float64)
            self._chk(L.of2d_batch_jacobian(self._h, buf.ctypes.data, st.ctypes.data))
            maps = np.ascontiguousarray(
                buf.reshape(self.nbatch, self.dimy, self.dimx).transpose(0, 2, 1))
        else:
            self._chk(L.of2d_batch_jacobian(self._h, None, st.ctypes.data))
        return maps, [_jac_stats(s) for s in st]

    def inverse_motion(self, max_iter: int = 50, tol: float = 1e-3, out=None):
        """``(v, info)``: the inverse of every pair's motion, ``[nbatch, dimx,
        dimy, 2]``, and a list of :meth:`ImageRegistration.inverse_motion`'s
        ``info`` dicts; every pair stops on its own update.  ``out`` (a CUDA
        tensor of that shape) receives the fields on the device
        (of2d_batch_invert_motion_device) and is returned."""
        max_iter, tol = _invert_args(max_iter, tol)
        L = _lib.lib()
        info = np.zeros((self.nbatch, 4), np.float64)
        if out is not None:
            shape = (self.nbatch, self.dimx, self.dimy, 2)
            out = _device.output(out, shape, None, self._device)
            a = _device.darray(out, shape, (0, 1, 2, 3), "out")
            self._chk(L.of2d_batch_invert_motion_device(self._h, max_iter, tol, C.byref(a),
                                                        info.ctypes.data,
                                                        _device.stream_of(out)))
            v = out
        else:
            buf = np.zeros(self.nbatch * 2 * self.dimx * self.dimy, np.float64)
            self._chk(L.of2d_batch_invert_motion(self._h, max_iter, tol, buf.ctypes.data,
                                                 info.ctypes.data))
            v = np.ascontiguousarray(
                buf.reshape(self.nbatch, 2, self.dimy, self.dimx).transpose(0, 3, 2, 1))
        return v, [_invert_info(i) for i in info]

    def quality(self, Iref, Imov) -> list:
        """Per pair :meth:`ImageRegistration.quality`'s dict: MSE and zero-mean
        NCC of ``Iref`` against ``Imov`` and against ``Imov`` warped by the
        pair's motion.  The images are :meth:`register`'s (``Iref`` one image
        or a stack); two CUDA tensors are read where they are
        (of2d_batch_quality_device)."""
        L = _lib.lib()
        q = np.zeros((self.nbatch, 4), np.float64)
        stack = (self.nbatch, self.dimx, self.dimy)
        if _device.all_cuda(Iref=Iref, Imov=Imov):
            shared = Iref.dim() == 2
            if shared:
                r = _device.darray(Iref, stack[1:], (1, 2), "Iref")
            elif tuple(Iref.shape) == stack:
                r = _device.darray(Iref, stack, (0, 1, 2), "Iref")
            else:
                raise ValueError(f"Iref is {tuple(Iref.shape)}, expected {stack[1:]} or {stack}")
            m = _device.darray(Imov, stack, (0, 1, 2), "Imov")
            self._chk(L.of2d_batch_quality_device(self._h, C.byref(r), int(shared), C.byref(m),
                                                  q.ctypes.data, _device.stream_of(Imov)))
        else:
            r = np.asarray(Iref, dtype=np.float64)
            shared = r.ndim == 2
            if shared:
                if r.shape != stack[1:]:
                    raise ValueError(f"Iref is {r.shape}, expected {stack[1:]} or {stack}")
                r = np.ascontiguousarray(r.T).reshape(-1)
            else:
                r = self._stack(r, "Iref")
            m = self._stack(Imov, "Imov")
            self._chk(L.of2d_batch_quality(self._h, r.ctypes.data, int(shared), m.ctypes.data,
                                           q.ctypes.data))
        keys = ("mse_before", "ncc_before", "mse_after", "ncc_after")
        return [dict(zip(keys, (float(v) for v in row))) for row in q]

    def iterations(self) -> np.ndarray:
        """``[nbatch, loops]`` iterations run, loops in execution order
        (coarsest level first, its refines, ...)."""
        buf = np.zeros(max(1, self.nbatch * self.loops), np.int32)
        n = _lib.lib().of2d_batch_iterations(self._h, buf, buf.size)
        return buf[: max(n, 0)].reshape(self.nbatch, self.loops).copy()

    def last_errors(self, pair: int) -> np.ndarray:
        """The Logger errors of the pair's last loop (empty with ``fixed_iters``)."""
        if not 0 <= int(pair) < self.nbatch:
            raise ValueError(f"pair {pair} outside [0, {self.nbatch})")
        buf = np.zeros(self._maxn, np.float32)
        n = _lib.lib().of2d_batch_last_errors(self._h, int(pair), buf, buf.size)
        return buf[: max(n, 0)].copy()

    def fluid_log(self, pair: int) -> list:
        """Option ``fluid``: one ``float32 [n, 4]`` array per loop (execution
        order, as :meth:`iterations`), a row ``[maxabs, dt, jmin, regridded]``
        per iteration the pair's loop ran in the last :meth:`register`
        (of2d_batch_fluid_log).  Empty arrays without the option."""
        if not 0 <= int(pair) < self.nbatch:
            raise ValueError(f"pair {pair} outside [0, {self.nbatch})")
        out = []
        for loop in range(self.loops):
            buf = np.zeros(4 * self._maxn, np.float32)
            n = _lib.lib().of2d_batch_fluid_log(self._h, int(pair), loop, buf, self._maxn)
            out.append(buf[: 4 * max(n, 0)].reshape(-1, 4).copy())
        return out

    def fluid_lines(self, pair: int) -> list:
        """The lines the reference prints for the pair, in its order, without
        the newline (:func:`fluid_lines` of :meth:`fluid_log`)."""
        return fluid_lines(self.fluid_log(pair))

    def status(self) -> np.ndarray:
        """``[nbatch]`` OF2D_OK (0) or OF2D_ERR_RUNTIME (2) per pair."""
        out = (C.c_int * self.nbatch)()
        self._chk(_lib.lib().of2d_batch_status(self._h, out))
        return np.array(out[:], np.int32)

    def last_error(self) -> str:
        """The first failed pair's message ("Divide by zero exception (pair k)"), or ''."""
        return _lib.lib().of2d_batch_last_error(self._h).decode()

    def info(self) -> dict:
        """``launches`` of the last estimate (independent of nbatch), ``loops``
        per pair, ``loop_us`` (device time of the loop kernels), and per level
        from level 0 ``placement`` in the last estimate (0: global memory; 1:
        on the compute unit, the iterate with option ``resident``, the
        convolved field with option ``conv_lds``) and ``threads`` of a pair's
        workgroup."""
        buf = (C.c_int * 256)()
        n = _lib.lib().of2d_batch_info(self._h, buf, 256)
        v = list(buf[: max(n, 0)])
        nlev = v[2]
        return {"launches": v[0], "loops": v[1], "levels": nlev, "loop_us": v[3],
                "placement": v[4: 4 + 2 * nlev: 2], "threads": v[5: 5 + 2 * nlev: 2]}

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.lib().of2d_batch_destroy(self._h)
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


def _c_float(v: float) -> str:
    """``printf("%.3f", v)``: Python's ``%`` prints infinities and NaN as C does
    ('inf', '-inf', 'nan')."""
    return "%.3f" % float(v)


def fluid_lines(log) -> list:
    """The reference's printed lines from a Fluid log (a list with one ``[n, 4]``
    array of ``[maxabs, dt, jmin, regridded]`` rows per loop, as
    :meth:`BatchRegistration.fluid_log` returns): per iteration
    ``"Dumax: %.3f\\tMaxabs increment: %.3f\\t Timestep: %.3f"`` with
    ``(double)0.65f`` (OpticalFlowFluid.cpp), and after the Dumax line of an
    iteration that regridded ``"Regridding on iteration: %d\\tMin Jacobian:
    %.3f"`` with the iteration counted from 0 within its loop
    (ImageRegistrationFluid.cpp:107-124).  A pure function of the log."""
    dumax = float(np.float32(0.65))
    lines = []
    for rows in log:
        for it, (maxabs, dt, jmin, regridded) in enumerate(np.asarray(rows, np.float32).reshape(-1, 4)):
            lines.append("Dumax: %s\tMaxabs increment: %s\t Timestep: %s"
                         % (_c_float(dumax), _c_float(maxabs), _c_float(dt)))
            if regridded != 0:
                lines.append("Regridding on iteration: %d\tMin Jacobian: %s" % (it, _c_float(jmin)))
    return lines


__all__ = ["BatchRegistration", "BATCH_MAXPX", "fluid_lines"]
