"""Thirion's Demons on the batched interface, on the CPU (include/of2d.h
of2d_batch_*): reg 3 with its six parameters creates a handle, every refusal
keeps its message, and BatchRegistration takes ``reg=``.  No device is needed:
the checks precede any device work."""
import ctypes as C

import numpy as np
import pytest

DEMONS = (1.0, 0.25, 1.5, 2.5, 5, 0)
PARAM_COUNT = "Invalid number of regularisation parameters for given regularisation method."


def _create(L, nbatch=2, dimx=16, dimy=12, niter=(5,), nscales=0, reg=3, params=DEMONS,
            nrefine=1):
    h = C.c_void_p()
    nit = np.ascontiguousarray(np.asarray(niter, np.int32))
    p = np.ascontiguousarray(np.asarray(params, np.float32))
    rc = L.of2d_batch_create(C.byref(h), nbatch, dimx, dimy, nit, nscales, reg, p, len(params),
                             nrefine)
    return rc, h, L.of2d_batch_last_error(None).decode()


def test_reg3_with_six_parameters_creates_a_handle(of2d_lib):
    from opticalflow2d_amd import _lib
    for params in (DEMONS, (1.0, 0.3, 1.5, 2.5, 4, 1), (1.0, 0.25, 1.5, 2.5, 1, 2),
                   (1.0, 0.25, 1.5, 2.5, 15, 0)):  # wider than the 12 j-lines
        rc, h, msg = _create(of2d_lib, params=params)
        assert rc == _lib.OF2D_OK and h.value, msg
        assert of2d_lib.of2d_batch_destroy(h) == _lib.OF2D_OK


@pytest.mark.parametrize("kw, text", [
    (dict(params=(1.0,)), PARAM_COUNT),
    (dict(params=DEMONS[:5]), PARAM_COUNT),
    (dict(params=(1.0, 0.25, 1.5, 2.5, 0, 0)), "Error: Demons kernel width must be >= 1"),
    # Diffeomorphic Demons and the other methods stay refused, whatever the count
    (dict(reg=4, params=DEMONS[:5]), "Diffusion regularisation only"),
    (dict(reg=4, params=DEMONS), "Diffusion regularisation only"),
    (dict(reg=1, params=(0.1, 0.2)), "Diffusion regularisation only"),
    (dict(reg=2, params=(0.1, 0.2)), "Diffusion regularisation only"),
    (dict(reg=5, params=(0.1, 0.2)), "Diffusion regularisation only"),
    # the batch's own limits hold for reg 3 too
    (dict(dimx=513, dimy=512), "OF2D_BATCH_MAXPX"),
    (dict(nbatch=0), "nbatch >= 1"),
])
def test_create_refusals(of2d_lib, kw, text):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib, **kw)
    assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert not h.value
    assert text in msg


def test_python_class_takes_reg(of2d_lib):
    from opticalflow2d_amd import BatchRegistration, InvalidArgument, Regularisation
    with BatchRegistration(3, (16, 12), [4, 4], 1, list(DEMONS), nrefine=2, reg=3,
                           fixed_iters=1) as b:
        assert (b.nbatch, b.dimx, b.dimy, b.loops, b.reg) == (3, 16, 12, 4, 3)
        assert b.iterations().shape == (3, 4) and not b.iterations().any()
        assert b.status().tolist() == [0, 0, 0]
        assert b.last_error() == ""
        with pytest.raises(ValueError, match="expected"):
            b.register(np.zeros((12, 16)), np.zeros((3, 16, 12)))
        # demons_separable is the one-pair path's option, not the batch's
        with pytest.raises(InvalidArgument, match="unknown option: demons_separable"):
            b.set_option("demons_separable", 1)
    with BatchRegistration(2, (16, 12), [4], 0, list(DEMONS),
                           reg=Regularisation.ThirionsDemons) as b:
        assert b.reg == 3 and b.loops == 1
    with pytest.raises(InvalidArgument, match="Invalid number of regularisation parameters"):
        BatchRegistration(2, (16, 12), [4], 0, 0.1, reg=3)
    with pytest.raises(InvalidArgument, match="Demons kernel width must be >= 1"):
        BatchRegistration(2, (16, 12), [4], 0, [1.0, 0.25, 1.5, 2.5, 0, 0], reg=3)
    with pytest.raises(InvalidArgument, match="Diffusion regularisation only"):
        BatchRegistration(2, (16, 12), [4], 0, list(DEMONS[:5]), reg=4)
    # the default stays Diffusion: two parameters are a wrong count, six too
    with pytest.raises(InvalidArgument, match="Invalid number of regularisation parameters"):
        BatchRegistration(2, (16, 12), [4], 0, [0.1, 0.2])
    with pytest.raises(InvalidArgument, match="Invalid number of regularisation parameters"):
        BatchRegistration(2, (16, 12), [4], 0, list(DEMONS))
    with BatchRegistration(2, (16, 12), [4], 0, 0.1) as b:
        assert b.reg == 0
