"""The test and diagnostic entries of libof2d.so (csrc/of2d_prims.h), one launch
per kernel on host arrays, for the test suites and the tools; the interface
users import is :mod:`opticalflow2d_amd.registration`."""
import ctypes as C
from typing import Sequence

import numpy as np

from . import _device
from .registration import _call, _f32


# ------------------------------------------------------------------ Logger norms
def motion_norms(cur, prev, dims: Sequence[int]):
    """Motion::norm sums of (cur - prev) and of prev exactly as the reference's
    Logger takes them (src/Motion.cpp:42-49, src/Logger.cpp:32-51): float
    running sums in linear order, on the device.  ``cur`` / ``prev`` are
    float32 ``[dimx*dimy, 2]`` (interleaved x, y per pixel, idx = i + j*dimx),
    or ``[npairs, dimx*dimy, 2]`` for a sequence of Logger updates run on one
    workspace (each predicts the next).  Returns ``(sums float32[..., 2],
    stats int32[..., 8])``: stats are cost figures of the device walk
    (csrc/of2d_prims.h of2d_motion_norms), not results."""
    dimx, dimy = int(dims[0]), int(dims[1])
    c = np.ascontiguousarray(np.asarray(cur, np.float32).reshape(-1))
    p = np.ascontiguousarray(np.asarray(prev, np.float32).reshape(-1))
    n = 2 * dimx * dimy
    if c.size % n or p.size != c.size or c.size == 0:
        raise ValueError("cur / prev need npairs * dimx*dimy*2 floats")
    k = c.size // n
    sums = np.zeros(2 * k, np.float32)
    res = np.zeros(8 * k, np.int32)
    _call("of2d_motion_norms", c, p, dimx, dimy, k, sums, res)
    if np.asarray(cur).ndim == 3:
        return sums.reshape(k, 2), res.reshape(k, 8)
    return sums, res


def motion_norms_chain(u, dims: Sequence[int], batch: int = 3):
    """The Logger norms of each update of a chain of iterates ``u``
    (float32 ``[niter + 1, dimx*dimy, 2]``), computed in batches of ``batch``
    updates as the registration loop runs them (csrc/of2d_prims.h
    of2d_motion_norms_chain).  Returns ``(sums float32[niter, 2], stats
    int32[niter, 8])``."""
    dimx, dimy = int(dims[0]), int(dims[1])
    a = np.ascontiguousarray(np.asarray(u, np.float32).reshape(-1))
    n = 2 * dimx * dimy
    if a.size % n or a.size < 2 * n:
        raise ValueError("u needs (niter + 1) * dimx*dimy*2 floats")
    niter = a.size // n - 1
    sums = np.zeros(2 * niter, np.float32)
    res = np.zeros(8 * niter, np.int32)
    _call("of2d_motion_norms_chain", a, dimx, dimy, niter, int(batch), sums, res)
    return sums.reshape(niter, 2), res.reshape(niter, 8)


# ------------------------------------------------------------------ Curvature transforms
def dct2d(a, kind: int, method: int = 1):
    """Curvature's separable REDFT10 (``kind=10``) or REDFT01 (``kind=1``) of
    ``a`` (``[dimx, dimy]``), on the device, as one solver iteration runs it:
    axis y, then axis x, no eigenvalues (csrc/of2d_prims.h of2d_dct2d).
    ``method`` 0 takes the GEMMs, 1 the fast line transforms on every axis
    whose length qualifies.  Returns ``(result [dimx, dimy], (fast_x,
    fast_y))``."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("a must be [dimx, dimy]")
    dimx, dimy = a.shape
    buf = np.ascontiguousarray(a.reshape(-1, order="F")).copy()
    paths = np.zeros(2, np.int32)
    _call("of2d_dct2d", buf, dimx, dimy, int(kind), int(method), paths)
    return buf.reshape((dimx, dimy), order="F"), (int(paths[0]), int(paths[1]))


# ------------------------------------------------------------------ primitives
class prim:
    """One launch each of the field and Demons primitives the solvers call
    (csrc/of2d_prims.h, "test and diagnostic entries").  Arrays are float32 in
    the C-ABI's own layout: an image is ``[dimy, dimx]`` and a motion field
    ``[dimy, dimx, 2]`` in C order (idx = i + j*dimx, x and y interleaved).
    Results are new arrays; bits are never touched on the way."""

    _f = staticmethod(_f32)
    _call = staticmethod(_call)

    @classmethod
    def warp(cls, src, u):
        src = cls._f(src)
        dimy, dimx = src.shape
        out = np.zeros_like(src)
        cls._call("of2d_prim_warp", src, cls._f(u, (dimy, dimx, 2)), dimx, dimy, out)
        return out

    @classmethod
    def accumulate(cls, m_old, v):
        m_old = cls._f(m_old)
        dimy, dimx, _ = m_old.shape
        out = np.zeros_like(m_old)
        cls._call("of2d_prim_accumulate", m_old, cls._f(v, m_old.shape), dimx, dimy, out)
        return out

    @classmethod
    def regrid(cls, m_old, est, Imov):
        """Returns ``(m_new, est0, Iaux)``."""
        m_old = cls._f(m_old)
        dimy, dimx, _ = m_old.shape
        m_new, est0 = np.zeros_like(m_old), np.zeros_like(m_old)
        Iaux = np.zeros((dimy, dimx), np.float32)
        cls._call("of2d_prim_regrid", m_old, cls._f(est, m_old.shape),
                  cls._f(Imov, (dimy, dimx)), dimx, dimy, m_new, est0, Iaux)
        return m_new, est0, Iaux

    @classmethod
    def compose_zero(cls, v, row0=0, dimy=None):
        """``v`` holds rows ``[row0, row0 + nrows)`` of a ``dimy``-row grid."""
        v = cls._f(v)
        nrows, dimx, _ = v.shape
        out = np.zeros_like(v)
        cls._call("of2d_prim_compose_zero", v, dimx, nrows, int(row0),
                  nrows if dimy is None else int(dimy), out)
        return out

    @classmethod
    def add_motion(cls, a, b):
        a = cls._f(a)
        dimy, dimx, _ = a.shape
        out = np.zeros_like(a)
        cls._call("of2d_prim_add_motion", a, cls._f(b, a.shape), dimx, dimy, out)
        return out

    @classmethod
    def _resample(cls, what, a, out):
        a, out = cls._f(a), cls._f(out).copy()
        cls._call("of2d_prim_resample", what, a, a.shape[1], a.shape[0], out, out.shape[1],
                  out.shape[0])
        return out

    @classmethod
    def downsample_image(cls, a, out):
        """``out`` is the target's content before the call (kept where no tap
        is valid); the result is a copy."""
        return cls._resample(0, a, out)

    @classmethod
    def downsample_motion(cls, a, out):
        return cls._resample(1, a, out)

    @classmethod
    def upsample_motion(cls, a, out):
        return cls._resample(2, a, out)

    @classmethod
    def gradients(cls, Iref, Iaux, row0=0, nrows=None):
        """``(dI [nrows, dimx, 2], It [nrows, dimx])`` of rows ``[row0, row0 +
        nrows)`` of the whole images, by the slab form of the launch."""
        Iref = cls._f(Iref)
        dimy, dimx = Iref.shape
        nrows = dimy - row0 if nrows is None else int(nrows)
        dI = np.zeros((max(nrows, 0), dimx, 2), np.float32)
        It = np.zeros((max(nrows, 0), dimx), np.float32)
        cls._call("of2d_prim_gradients", Iref, cls._f(Iaux, Iref.shape), dimx, dimy, int(row0),
                  nrows, dI, It)
        return dI, It

    @classmethod
    def demons_force(cls, Iref, Imov, u, sigma_i, sigma_x):
        """Returns ``(corr, status)``."""
        Iref = cls._f(Iref)
        dimy, dimx = Iref.shape
        out = np.zeros((dimy, dimx, 2), np.float32)
        st = C.c_uint(0)
        cls._call("of2d_prim_demons_force", Iref, cls._f(Imov, Iref.shape),
                  cls._f(u, out.shape), dimx, dimy, float(sigma_i), float(sigma_x), out,
                  C.byref(st))
        return out, int(st.value)

    @classmethod
    def smooth_compose(cls, corr, u, kw, sigma, mode, method=None):
        """Returns ``(out, wfull)``; with ``method`` (0 the direct convolution,
        1 the separable one where it qualifies) ``(out, wfull, path)``, ``path``
        1 when the separable kernels ran."""
        corr = cls._f(corr)
        dimy, dimx, _ = corr.shape
        out = np.zeros_like(corr)
        w, path = C.c_double(0), C.c_int(-1)
        cls._call("of2d_prim_smooth_compose", corr, cls._f(u, corr.shape), dimx, dimy, int(kw),
                  float(sigma), int(mode), out, C.byref(w), int(method or 0), C.byref(path))
        res = (out, float(w.value))
        return res if method is None else res + (int(path.value),)

    @classmethod
    def smooth_norm(cls, umid, prev, kw, sigma, partials=True, method=None):
        """Returns ``(out, sums)``: ``sums`` the two fp64 Logger sums, or None
        from the launch without partials; with ``method`` (as smooth_compose)
        ``(out, sums, path)``."""
        umid = cls._f(umid)
        dimy, dimx, _ = umid.shape
        out = np.zeros_like(umid)
        sums, path = (C.c_double * 2)(), C.c_int(-1)
        cls._call("of2d_prim_smooth_norm", umid, cls._f(prev, umid.shape), dimx, dimy, int(kw),
                  float(sigma), out, sums if partials else None, int(method or 0),
                  C.byref(path))
        res = (out, (float(sums[0]), float(sums[1])) if partials else None)
        return res if method is None else res + (int(path.value),)

    @classmethod
    def demons_update(cls, Iref, Imov, u, sigma_i, sigma_x, kw, sigma_fluid, mode, method=None):
        """Returns ``(out, status)``; with ``method`` (as smooth_compose)
        ``(out, status, path)``."""
        Iref = cls._f(Iref)
        dimy, dimx = Iref.shape
        out = np.zeros((dimy, dimx, 2), np.float32)
        st, path = C.c_uint(0), C.c_int(-1)
        cls._call("of2d_prim_demons_update", Iref, cls._f(Imov, Iref.shape),
                  cls._f(u, out.shape), dimx, dimy, float(sigma_i), float(sigma_x), int(kw),
                  float(sigma_fluid), int(mode), out, C.byref(st), int(method or 0),
                  C.byref(path))
        res = (out, int(st.value))
        return res if method is None else res + (int(path.value),)

    @classmethod
    def motion_exp(cls, f, sigma_i=0.0, sigma_x=1.0):
        """Returns ``(exp(f), squarings, status)``."""
        f = cls._f(f).copy()
        dimy, dimx, _ = f.shape
        n, st = C.c_int(0), C.c_uint(0)
        cls._call("of2d_prim_motion_exp", f, dimx, dimy, float(sigma_i), float(sigma_x),
                  C.byref(n), C.byref(st))
        return f, int(n.value), int(st.value)

    @classmethod
    def d2f(cls, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        out = np.zeros(a.shape, np.float32)
        cls._call("of2d_prim_d2f", a, a.shape[1], a.shape[0], out)
        return out

    @classmethod
    def f2d(cls, a):
        a = cls._f(a)
        out = np.zeros(a.shape, np.float64)
        cls._call("of2d_prim_f2d", a, a.shape[1], a.shape[0], out)
        return out

    @classmethod
    def motion_to_planar(cls, m):
        """``[2, dimy, dimx]`` float64, the x plane first."""
        m = cls._f(m)
        out = np.zeros((2,) + m.shape[:2], np.float64)
        cls._call("of2d_prim_motion_to_planar", m, m.shape[1], m.shape[0], out)
        return out

    # Device-resident I/O (io_kernels.hip), one launch each.  ``t`` / ``out``
    # are torch CUDA tensors whose dimension d is the of2d_darray axis
    # ``axes[d]`` (0 pair, 1 x, 2 y, 3 component); the host side is float32 in
    # the layout above with a leading pair axis.
    #
    # The pack entries take ``raw=True`` and then return ``(out, raw)``: ``raw``
    # is the whole allocation of the pitched fields, ``[npairs, stride]`` (a
    # motion: ``[npairs, stride, 2]``) with ``pack_layout``'s stride, holding
    # ``PACK_SENTINEL`` in every word that no store touched; pixel (i, j) of a
    # pair is element ``P + j * P + i`` of its row.
    PACK_SENTINEL = 0xC5C5C5C5

    @classmethod
    def pack_layout(cls, dimx, dimy):
        """``(stride, P)`` of the batch's pitched fields, in elements."""
        stride, P = C.c_longlong(0), C.c_int(0)
        cls._call("of2d_prim_pack_layout", int(dimx), int(dimy), C.byref(stride), C.byref(P))
        return int(stride.value), int(P.value)

    @classmethod
    def _raw(cls, raw, npairs, dimx, dimy, tail=()):
        if not raw:
            return None
        return np.zeros((npairs, cls.pack_layout(dimx, dimy)[0]) + tail, np.float32)

    @classmethod
    def pack_image(cls, t, axes=(0, 1, 2), raw=False):
        ext = dict(zip(axes, t.shape))
        npairs, dimx, dimy = ext[0], ext[1], ext[2]
        out = np.zeros((npairs, dimy, dimx), np.float32)
        whole = cls._raw(raw, npairs, dimx, dimy)
        a = _device.darray(t, t.shape, axes, "in")
        cls._call("of2d_prim_pack_image", C.byref(a), npairs, dimx, dimy, out, whole)
        return (out, whole) if raw else out

    @classmethod
    def pack_motion(cls, t, axes=(0, 1, 2, 3), raw=False):
        """``t`` with extent 2 on the component axis -> ``[npairs, dimy, dimx, 2]``."""
        ext = dict(zip(axes, t.shape))
        npairs, dimx, dimy = ext[0], ext[1], ext[2]
        if ext[3] != 2:
            raise ValueError(f"the component axis has extent {ext[3]}, expected 2")
        out = np.zeros((npairs, dimy, dimx, 2), np.float32)
        whole = cls._raw(raw, npairs, dimx, dimy, (2,))
        a = _device.darray(t, t.shape, axes, "in")
        cls._call("of2d_prim_pack_motion", C.byref(a), npairs, dimx, dimy, out, whole)
        return (out, whole) if raw else out

    @classmethod
    def planar_to_motion(cls, a, raw=False):
        """``a`` float64 ``[npairs, 2, dimy, dimx]`` (``motion_to_planar``'s
        layout per pair) -> ``[npairs, dimy, dimx, 2]``, by the host form's kernel."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim != 4 or a.shape[1] != 2:
            raise ValueError(f"a stack of planar fields is [npairs, 2, dimy, dimx], got {a.shape}")
        npairs, _, dimy, dimx = a.shape
        out = np.zeros((npairs, dimy, dimx, 2), np.float32)
        whole = cls._raw(raw, npairs, dimx, dimy, (2,))
        cls._call("of2d_prim_planar_to_motion", a, npairs, dimx, dimy, out, whole)
        return (out, whole) if raw else out

    @classmethod
    def unpack_image(cls, a, out, axes=(0, 1, 2)):
        a = cls._f(a)
        npairs, dimy, dimx = a.shape
        shape = [0, 0, 0]
        for d, ax in enumerate(axes):
            shape[d] = (npairs, dimx, dimy)[ax]
        o = _device.darray(out, shape, axes, "out")
        cls._call("of2d_prim_unpack_image", a, npairs, dimx, dimy, C.byref(o))
        return out

    @classmethod
    def unpack_motion(cls, m, out, axes=(0, 1, 2, 3)):
        m = cls._f(m)
        npairs, dimy, dimx, _ = m.shape
        shape = [0, 0, 0, 0]
        for d, ax in enumerate(axes):
            shape[d] = (npairs, dimx, dimy, 2)[ax]
        o = _device.darray(out, shape, axes, "out")
        cls._call("of2d_prim_unpack_motion", m, npairs, dimx, dimy, C.byref(o))
        return out

    # The batched analysis kernels (batch_analysis_kernels.hip), one launch
    # each on stacks with a leading pair axis: u ``[B, dimy, dimx, 2]``, images
    # ``[B, dimy, dimx]``.
    @classmethod
    def batch_jacobian(cls, u, jac=True):
        """``(maps [B, dimy, dimx] or None, stats [B, 5])``."""
        u = cls._f(u)
        if u.ndim != 4 or u.shape[3] != 2:
            raise ValueError(f"a stack of motion fields is [B, dimy, dimx, 2], got {u.shape}")
        B, dimy, dimx, _ = u.shape
        out = np.zeros((B, dimy, dimx), np.float32) if jac else None
        st = np.zeros((B, 5), np.float64)
        cls._call("of2d_prim_batch_jacobian", u, B, dimx, dimy, out, st)
        return out, st

    @classmethod
    def batch_invert(cls, u, max_iter=50, tol=1e-3, residuals=True):
        """``(v [B, dimy, dimx, 2], info [B, 4], residuals [B, max_iter] or None)``."""
        u = cls._f(u)
        if u.ndim != 4 or u.shape[3] != 2:
            raise ValueError(f"a stack of motion fields is [B, dimy, dimx, 2], got {u.shape}")
        B, dimy, dimx, _ = u.shape
        v = np.zeros_like(u)
        info = np.zeros((B, 4), np.float64)
        res = np.zeros((B, max(int(max_iter), 1)), np.float32) if residuals else None
        cls._call("of2d_prim_batch_invert", u, B, dimx, dimy, int(max_iter), float(tol), v, info,
                  res)
        return v, info, res

    @classmethod
    def batch_similarity(cls, a, b):
        """``[B, 2]`` = (mse, ncc) per pair; ``a`` is ``[B, dimy, dimx]`` or one
        ``[dimy, dimx]`` image shared by every pair."""
        b = cls._f(b)
        if b.ndim != 3:
            raise ValueError(f"a stack of images is [B, dimy, dimx], got {b.shape}")
        a = cls._f(a)
        shared = a.ndim == 2
        if a.shape != (b.shape[1:] if shared else b.shape):
            raise ValueError(f"a is {a.shape}, expected {b.shape[1:]} or {b.shape}")
        B, dimy, dimx = b.shape
        out = np.zeros((B, 2), np.float64)
        cls._call("of2d_prim_batch_similarity", a, int(shared), b, B, dimx, dimy, out)
        return out

    # Curvature, one call each (csrc/of2d_prims.h).  curv_rhs and
    # curv_construct take fields in the layout above; curv_eigen and curv_dct2d
    # speak ``[dimx, dimy]`` arrays as :func:`dct2d` does.
    @classmethod
    def curv_rhs(cls, u, dI, It, tau):
        """``u - tau * force`` as float64 ``[2, dimy, dimx]``, the x plane first."""
        u = cls._f(u)
        dimy, dimx, _ = u.shape
        out = np.zeros((2, dimy, dimx), np.float64)
        cls._call("of2d_prim_curv_rhs", u, cls._f(dI, u.shape), cls._f(It, (dimy, dimx)),
                  float(tau), dimx, dimy, out[0], out[1])
        return out

    @classmethod
    def curv_eigen(cls, dims, alpha, tau, method=0):
        """The eigenvalue table of a ``dims = (dimx, dimy)`` level, ``E[p, q]``."""
        dimx, dimy = int(dims[0]), int(dims[1])
        out = np.zeros(dimx * dimy, np.float64)
        cls._call("of2d_prim_curv_eigen", dimx, dimy, float(alpha), float(tau), int(method), out)
        return out.reshape((dimx, dimy), order="F")

    @classmethod
    def curv_dct2d(cls, ax, ay, kind, method=0, eig=None):
        """:func:`dct2d` of both planes in the one call an iteration makes;
        ``eig = (alpha, tau)`` fuses the eigenvalue product (``kind`` 10 only).
        Returns ``(x [dimx, dimy], y [dimx, dimy], (fast_x, fast_y))``."""
        ax, ay = np.asarray(ax, dtype=np.float64), np.asarray(ay, dtype=np.float64)
        if ax.ndim != 2 or ay.shape != ax.shape:
            raise ValueError("ax and ay must be [dimx, dimy]")
        dimx, dimy = ax.shape
        bx = np.ascontiguousarray(ax.reshape(-1, order="F")).copy()
        by = np.ascontiguousarray(ay.reshape(-1, order="F")).copy()
        paths = np.zeros(2, np.int32)
        alpha, tau = (0.0, 0.0) if eig is None else eig
        cls._call("of2d_prim_curv_dct2d", bx, by, dimx, dimy, int(kind), int(method),
                  int(eig is not None), float(alpha), float(tau), paths)
        return (bx.reshape((dimx, dimy), order="F"), by.reshape((dimx, dimy), order="F"),
                (int(paths[0]), int(paths[1])))

    @classmethod
    def curv_construct(cls, z, u, div):
        """``z`` float64 ``[2, dimy, dimx]``; returns ``(out [dimy, dimx, 2],
        (sum |out - u|, sum |u|))``, the sums from the launch's Logger partials."""
        u = cls._f(u)
        dimy, dimx, _ = u.shape
        z = np.ascontiguousarray(z, dtype=np.float64)
        if z.shape != (2, dimy, dimx):
            raise ValueError(f"z is {z.shape}, expected {(2, dimy, dimx)}")
        out = np.zeros_like(u)
        sums = np.zeros(2, np.float64)
        cls._call("of2d_prim_curv_construct", z[0], z[1], u, float(div), dimx, dimy, out, sums)
        return out, (float(sums[0]), float(sums[1]))

    # The SOR sweep, Fluid and Elastic, per launch (csrc/of2d_prims.h).  Granules
    # are uint32 ``[dimy, 4]``: row j of region 0 as (x bits, y bits, tag, tag).
    @staticmethod
    def increment_nblocks(dimx, dimy):
        """The 64 x 32 tiles of the Fluid field kernels (their partial slots)."""
        return ((dimx + 63) // 64) * ((dimy + 31) // 32)

    @classmethod
    def sor_pack(cls, u, dI, It, v0=None, epoch=1):
        """``v0`` given: Fluid's force-only pack over a working array whose v
        plane holds ``v0``; None: Elastic's pack with v = u.  Returns
        ``(v, b, granules)``."""
        u = cls._f(u)
        dimy, dimx, _ = u.shape
        v, b = np.zeros_like(u), np.zeros_like(u)
        gran = np.zeros((dimy, 4), np.uint32)
        cls._call("of2d_prim_sor_pack", u, cls._f(dI, u.shape), cls._f(It, (dimy, dimx)),
                  None if v0 is None else cls._f(v0, u.shape), int(v0 is None), dimx, dimy,
                  int(epoch), v, b, gran)
        return v, b, gran

    @classmethod
    def regrid_pack(cls, Iref, Iaux, v0, regridded, dI, It, b, gran, epoch=1):
        """``dI``, ``It``, ``b``, ``gran``: the buffers' content before the
        launch.  Returns their content after it, ``(dI, It, b, granules)``."""
        Iref = cls._f(Iref)
        dimy, dimx = Iref.shape
        m = (dimy, dimx, 2)
        dI, It, b = cls._f(dI, m).copy(), cls._f(It, (dimy, dimx)).copy(), cls._f(b, m).copy()
        gran = np.ascontiguousarray(gran, dtype=np.uint32).copy()
        if gran.shape != (dimy, 4):
            raise ValueError(f"gran is {gran.shape}, expected {(dimy, 4)}")
        cls._call("of2d_prim_regrid_pack", Iref, cls._f(Iaux, (dimy, dimx)), cls._f(v0, m),
                  int(bool(regridded)), dimx, dimy, int(epoch), dI, It, b, gran)
        return dI, It, b, gran

    @classmethod
    def sor_sweep(cls, v, b, mu, lam, omega, nsweeps=1, method=0, u=None, zero_est=False,
                  skip_at=-1, poison=None):
        """``nsweeps`` sweeps of ``v``.  Returns a dict: ``v``, ``status``,
        ``words`` (sweep ticket, role ticket, tile counter) and, for
        ``method`` 1, ``R``, ``maxabs``, ``dt``, ``part``, ``path``."""
        v = cls._f(v)
        dimy, dimx, _ = v.shape
        out = np.zeros_like(v)
        words = np.zeros(3, np.uint64)
        path, status = C.c_int(-1), C.c_uint(0)
        R = scal = part = None
        if method:
            R, scal = np.zeros_like(v), np.zeros(2, np.float32)
            part = np.zeros(cls.increment_nblocks(dimx, dimy), np.float32)
        cls._call("of2d_prim_sor_sweep", v, cls._f(b, v.shape),
                  None if u is None else cls._f(u, v.shape), dimx, dimy, float(mu), float(lam),
                  float(omega), int(method), int(nsweeps), int(bool(zero_est)), int(skip_at),
                  int(poison is not None), int(poison or 0), out, R, scal, part, C.byref(path),
                  words, C.byref(status))
        res = {"v": out, "status": status.value, "words": tuple(int(w) for w in words),
               "path": path.value}
        if method:
            res.update(R=R, maxabs=scal[0], dt=scal[1], part=part)
        return res

    @classmethod
    def fluid_increment(cls, u, v, zero_est=False):
        """Returns ``(R, maxabs, dt, part)``."""
        u = cls._f(u)
        dimy, dimx, _ = u.shape
        R, scal = np.zeros_like(u), np.zeros(2, np.float32)
        part = np.zeros(cls.increment_nblocks(dimx, dimy), np.float32)
        cls._call("of2d_prim_fluid_increment", u, cls._f(v, u.shape), dimx, dimy,
                  int(bool(zero_est)), R, scal, part)
        return R, scal[0], scal[1], part

    @classmethod
    def fluid_step(cls, u, R, dI, It, v0, dt, prev=None, zero_est=False, epoch=1):
        """Returns a dict: ``uo``, ``sums``, ``jmin``, ``b``, ``gran``."""
        u = cls._f(u)
        dimy, dimx, _ = u.shape
        uo, b = np.zeros_like(u), np.zeros_like(u)
        gran = np.zeros((dimy, 4), np.uint32)
        sums, jmin = np.zeros(2, np.float64), C.c_float(0)
        cls._call("of2d_prim_fluid_step", u, cls._f(R, u.shape),
                  None if prev is None else cls._f(prev, u.shape), cls._f(dI, u.shape),
                  cls._f(It, (dimy, dimx)), cls._f(v0, u.shape), float(dt), int(bool(zero_est)),
                  dimx, dimy, int(epoch), uo, sums, C.byref(jmin), b, gran)
        return {"uo": uo, "sums": (float(sums[0]), float(sums[1])),
                "jmin": np.float32(jmin.value), "b": b, "gran": gran}

    @classmethod
    def fluid_decide(cls, lpart, jpart, npx, fixed, it, words, seq=None, scal=(0.0, 0.0),
                     marker=-1234.5):
        """``lpart`` float64 ``[nb, 2]``, ``jpart`` float32 ``[nb]``, ``words`` =
        (status, stop, regrid, mcur).  Returns a dict: ``words`` after the
        launch, the report's fields (``flags`` 0xABABABAB: not written) and
        ``scal2`` (``marker`` when not written)."""
        lpart = np.ascontiguousarray(lpart, dtype=np.float64)
        jpart = cls._f(jpart)
        nb = jpart.size
        if lpart.shape != (nb, 2):
            raise ValueError(f"lpart is {lpart.shape}, expected {(nb, 2)}")
        w = np.array(words, dtype=np.uint32)
        if w.shape != (4,):
            raise ValueError("words is (status, stop, regrid, mcur)")
        sums, repf, repu = np.zeros(2), np.zeros(7, np.float32), np.zeros(2, np.uint32)
        repf[6] = marker
        cls._call("of2d_prim_fluid_decide", lpart.reshape(-1), jpart, nb,
                  None if seq is None else cls._f(seq, (2,)), float(npx), int(bool(fixed)),
                  int(it), cls._f(scal, (2,)), w, sums, repf, repu)
        return {"words": tuple(int(x) for x in w), "sums": (float(sums[0]), float(sums[1])),
                "maxabs": repf[0], "dt": repf[1], "jmin": repf[2], "seq": (repf[3], repf[4]),
                "err": repf[5], "scal2": repf[6], "status": int(repu[0]), "flags": int(repu[1])}

    @classmethod
    def elastic_logger(cls, v, prev):
        """Returns ``(u, new prev, (sum |u - prev|, sum |prev|))``."""
        v = cls._f(v)
        dimy, dimx, _ = v.shape
        u, pv = np.zeros_like(v), np.zeros_like(v)
        sums = np.zeros(2, np.float64)
        cls._call("of2d_prim_elastic_logger", v, cls._f(prev, v.shape), dimx, dimy, u, pv, sums)
        return u, pv, (float(sums[0]), float(sums[1]))
