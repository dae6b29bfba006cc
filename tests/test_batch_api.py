"""The batched Horn-Schunck interface on the CPU (include/of2d.h of2d_batch_*):
the symbols, every refusal with its message, and BatchRegistration's shape
checks.  No device is needed: the checks precede any device work."""
import ctypes as C

import numpy as np
import pytest

BATCH_SYMBOLS = ["of2d_batch_create", "of2d_batch_set_option", "of2d_batch_set_images",
                 "of2d_batch_estimate", "of2d_batch_get_motion", "of2d_batch_warp",
                 "of2d_batch_status", "of2d_batch_iterations", "of2d_batch_last_errors",
                 "of2d_batch_info", "of2d_batch_destroy", "of2d_batch_last_error"]


def test_symbols_exported_and_in_signatures(of2d_lib):
    from opticalflow2d_amd import _lib
    for n in BATCH_SYMBOLS:
        assert hasattr(of2d_lib, n), f"libof2d.so does not export {n}"
        assert n in _lib.SIGNATURES


def _create(L, nbatch=2, dimx=16, dimy=12, niter=(5,), nscales=0, reg=0, params=(0.1,),
            nparams=None, nrefine=1):
    h = C.c_void_p()
    nit = np.ascontiguousarray(np.asarray(niter, np.int32))
    p = np.ascontiguousarray(np.asarray(params, np.float32))
    rc = L.of2d_batch_create(C.byref(h), nbatch, dimx, dimy, nit, nscales, reg, p,
                             len(params) if nparams is None else nparams, nrefine)
    return rc, h, L.of2d_batch_last_error(None).decode()


@pytest.mark.parametrize("kw, text", [
    (dict(nbatch=0), "nbatch >= 1"),
    (dict(nbatch=-3), "nbatch >= 1"),
    (dict(nbatch=65536), "at most 65535 pairs"),
    (dict(reg=1, params=(0.1, 0.2)), "Diffusion regularisation only"),
    (dict(reg=5, params=(0.1, 0.2)), "Diffusion regularisation only"),
    (dict(params=(0.1, 0.2)),
     "Invalid number of regularisation parameters for given regularisation method."),
    (dict(nparams=0),
     "Invalid number of regularisation parameters for given regularisation method."),
    (dict(dimx=513, dimy=512), "OF2D_BATCH_MAXPX"),
    (dict(dimx=0), "invalid image dimensions"),
    (dict(dimy=-1), "invalid image dimensions"),
    (dict(nscales=-1), "invalid image dimensions"),
    (dict(dimx=3, dimy=12, nscales=2, niter=(1, 1, 1)), "pyramid level with zero size"),
])
def test_create_refusals(of2d_lib, kw, text):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib, **kw)
    assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert not h.value
    assert text in msg


def test_maxpx_is_accepted_and_null_arrays_refused(of2d_lib):
    from opticalflow2d_amd import _lib
    L = of2d_lib
    rc, h, _ = _create(L, nbatch=65535, dimx=4, dimy=4)  # the most pairs: no device work yet
    assert rc == _lib.OF2D_OK and h.value
    assert L.of2d_batch_destroy(h) == _lib.OF2D_OK
    rc, h, _ = _create(L, dimx=512, dimy=512)
    assert rc == _lib.OF2D_OK and h.value
    # NULL arrays: through the raw symbols (the typed table refuses None itself)
    raw = C.CDLL(_lib.LIB_PATH)
    raw.of2d_batch_set_images.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    raw.of2d_batch_get_motion.argtypes = [C.c_void_p, C.c_void_p]
    raw.of2d_batch_warp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    raw.of2d_batch_create.argtypes = [C.c_void_p] * 1 + [C.c_int] * 3 + [C.c_void_p, C.c_int,
                                                                       C.c_int, C.c_void_p,
                                                                       C.c_uint, C.c_int]
    buf = np.zeros(4, np.float64)
    ptr = buf.ctypes.data
    assert raw.of2d_batch_set_images(h, None, 0, ptr) == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert "NULL" in L.of2d_batch_last_error(h).decode()
    assert raw.of2d_batch_set_images(h, ptr, 0, None) == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert raw.of2d_batch_get_motion(h, None) == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert "NULL" in L.of2d_batch_last_error(h).decode()
    assert raw.of2d_batch_warp(h, None, ptr) == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert raw.of2d_batch_warp(h, ptr, None) == _lib.OF2D_ERR_INVALID_ARGUMENT
    h2 = C.c_void_p()
    one = np.ones(1, np.float32)
    nit = np.ones(1, np.int32)
    assert raw.of2d_batch_create(C.byref(h2), 2, 8, 8, None, 0, 0, one.ctypes.data, 1,
                                 1) == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert "NULL" in L.of2d_batch_last_error(None).decode() and not h2.value
    assert raw.of2d_batch_create(C.byref(h2), 2, 8, 8, nit.ctypes.data, 0, 0, None, 1,
                                 1) == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert "NULL" in L.of2d_batch_last_error(None).decode() and not h2.value
    assert raw.of2d_batch_create(None, 2, 8, 8, nit.ctypes.data, 0, 0, one.ctypes.data, 1,
                                 1) == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert L.of2d_batch_destroy(h) == _lib.OF2D_OK


def test_unknown_option_refused(of2d_lib):
    from opticalflow2d_amd import BatchRegistration, InvalidArgument
    with BatchRegistration(3, (16, 12), [4], 0, 0.1) as b:
        b.set_option("fixed_iters", 1)
        b.set_option("device", 0)
        with pytest.raises(InvalidArgument, match="unknown option: logger_fp64"):
            b.set_option("logger_fp64", 1)
    with pytest.raises(InvalidArgument, match="unknown option: chunk"):
        BatchRegistration(3, (16, 12), [4], 0, 0.1, chunk=3)


def test_python_class_refusals_and_shapes(of2d_lib):
    import opticalflow2d_amd as M
    from opticalflow2d_amd import BatchRegistration, InvalidArgument
    from opticalflow2d_amd import batch as BM
    assert "BatchRegistration" in M.__all__ and "BatchRegistration" in BM.__all__
    with pytest.raises(InvalidArgument, match="nbatch >= 1"):
        BatchRegistration(0, (16, 12), [4], 0, 0.1)
    with pytest.raises(InvalidArgument, match="Invalid number of regularisation parameters"):
        BatchRegistration(2, (16, 12), [4], 0, [0.1, 0.2])
    with pytest.raises(InvalidArgument, match="OF2D_BATCH_MAXPX"):
        BatchRegistration(2, (1024, 512), [4], 0, 0.1)
    with pytest.raises(ValueError, match="nscales\\+1"):
        BatchRegistration(2, (64, 64), [4], 1, 0.1)
    with BatchRegistration(3, (16, 12), [4, 4], 1, 0.1, nrefine=2, fixed_iters=1) as b:
        assert (b.nbatch, b.dimx, b.dimy, b.loops) == (3, 16, 12, 4)
        ok = np.zeros((3, 16, 12))
        # every shape error is raised before the library is entered
        for ref, mov in [(np.zeros((12, 16)), ok), (np.zeros((2, 16, 12)), ok),
                         (np.zeros((3, 12, 16)), ok), (ok, np.zeros((16, 12))),
                         (ok, np.zeros((4, 16, 12))), (np.zeros(16 * 12), ok)]:
            with pytest.raises(ValueError, match="expected"):
                b.register(ref, mov)
        with pytest.raises(ValueError, match="expected"):
            b.warp(np.zeros((16, 12)))
        with pytest.raises(ValueError, match="outside"):
            b.last_errors(3)
        assert b.iterations().shape == (3, 4) and not b.iterations().any()
        assert b.status().tolist() == [0, 0, 0]
        assert b.last_error() == ""
