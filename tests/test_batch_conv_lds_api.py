"""The batch option "conv_lds" on the CPU (include/of2d.h
of2d_batch_set_option): accepted with 0 and 1 on a Thirion's Demons batch,
refused with a message that names the reason for any other value and on a
Diffusion batch, and a refusal leaves the handle usable.  No device is needed:
the checks precede any device work."""
import ctypes as C

import numpy as np
import pytest

DEMONS = (1.0, 2.0, 1.0, 1.0, 5, 0)


def _create(L, reg=3, params=DEMONS):
    from opticalflow2d_amd import _lib
    h = C.c_void_p()
    nit = np.ascontiguousarray(np.asarray((5,), np.int32))
    p = np.ascontiguousarray(np.asarray(params, np.float32))
    rc = L.of2d_batch_create(C.byref(h), 2, 16, 12, nit, 0, reg, p, len(params), 1)
    assert rc == _lib.OF2D_OK and h.value, L.of2d_batch_last_error(None).decode()
    return h


def _set(L, h, value, key=b"conv_lds"):
    rc = L.of2d_batch_set_option(h, key, float(value))
    return rc, L.of2d_batch_last_error(h).decode()


def test_accepted_on_a_demons_batch(of2d_lib):
    from opticalflow2d_amd import _lib
    h = _create(of2d_lib)
    for v in (1, 0, 1):
        rc, msg = _set(of2d_lib, h, v)
        assert rc == _lib.OF2D_OK, msg
    # beside the other options of such a batch
    for key in (b"fixed_iters", b"warm_start", b"diffeomorphic"):
        rc, msg = _set(of2d_lib, h, 1, key)
        assert rc == _lib.OF2D_OK, msg
    assert _set(of2d_lib, h, 0)[0] == _lib.OF2D_OK
    assert of2d_lib.of2d_batch_destroy(h) == _lib.OF2D_OK


def test_refused_on_a_diffusion_batch(of2d_lib):
    from opticalflow2d_amd import _lib
    h = _create(of2d_lib, reg=0, params=(0.1,))
    for v in (1, 0):  # the handle, not the value, is what is refused
        rc, msg = _set(of2d_lib, h, v)
        assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT
        assert "conv_lds: the batch is not a Thirion's Demons batch" in msg
    # still usable: another option is taken, and the handle closes
    rc, msg = _set(of2d_lib, h, 1, b"resident")
    assert rc == _lib.OF2D_OK, msg
    assert of2d_lib.of2d_batch_destroy(h) == _lib.OF2D_OK


@pytest.mark.parametrize("value", [2, -1, float("nan")])
def test_a_value_other_than_0_or_1_is_refused(of2d_lib, value):
    from opticalflow2d_amd import _lib
    h = _create(of2d_lib)
    assert _set(of2d_lib, h, 1)[0] == _lib.OF2D_OK
    rc, msg = _set(of2d_lib, h, value)
    assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert "conv_lds: the value must be 0 or 1" in msg
    # usable, and both values are still taken
    assert _set(of2d_lib, h, 0)[0] == _lib.OF2D_OK
    assert _set(of2d_lib, h, 1)[0] == _lib.OF2D_OK
    assert of2d_lib.of2d_batch_destroy(h) == _lib.OF2D_OK


def test_python_class_takes_the_keyword(of2d_lib):
    from opticalflow2d_amd import BatchRegistration, InvalidArgument
    with BatchRegistration(3, (16, 12), [4, 4], 1, list(DEMONS), nrefine=2, reg=3, fixed_iters=1,
                           warm_start=1, diffeomorphic=1, conv_lds=1) as b:
        assert (b.nbatch, b.loops, b.reg) == (3, 4, 3)
        assert b.status().tolist() == [0, 0, 0] and b.last_error() == ""
        b.set_option("conv_lds", 0)
        b.set_option("conv_lds", 1)
        with pytest.raises(InvalidArgument, match="conv_lds: the value must be 0 or 1"):
            b.set_option("conv_lds", 2)
        with pytest.raises(InvalidArgument, match="conv_lds: the value must be 0 or 1"):
            b.set_option("conv_lds", -1)
        b.set_option("conv_lds", 1)
        # nothing has run: no level reports a placement on the CU yet
        assert b.info()["placement"] == [0, 0] and b.info()["threads"] == [1024, 1024]
        assert not b.iterations().any()
    with pytest.raises(InvalidArgument, match="conv_lds: the batch is not a Thirion's Demons"):
        BatchRegistration(2, (16, 12), [4], 0, 0.1, conv_lds=1)
