"""The one-pair motion input on the CPU (include/of2d.h of2d_set_motion,
of2d_set_motion_device, of2d_reset_motion): the names are exported, NULL and
bad arrays are refused with a named message before any device work, and the
Python class checks the shape.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

NAMES = ("of2d_set_motion", "of2d_set_motion_device", "of2d_reset_motion")


def _create(L, reg=0, params=(0.1,)):
    from opticalflow2d_amd import _lib
    h = C.c_void_p()
    nit = np.ascontiguousarray(np.asarray((5, 5), np.int32))
    p = np.ascontiguousarray(np.asarray(params, np.float32))
    rc = L.of2d_create(C.byref(h), 16, 12, nit, 1, reg, p, len(params), 1, 0)
    assert rc == _lib.OF2D_OK and h.value, L.of2d_last_error(None).decode()
    return h


def test_symbols_exported_and_in_signatures(of2d_lib):
    from opticalflow2d_amd import _lib
    for n in NAMES:
        assert hasattr(of2d_lib, n), f"libof2d.so does not export {n}"
        assert n in _lib.SIGNATURES and n in _lib.PRODUCT_SIGNATURES


def test_null_and_bad_arrays_are_refused_by_name(of2d_lib, quiet):
    from opticalflow2d_amd import _lib
    L = of2d_lib
    bad = _lib.OF2D_ERR_INVALID_ARGUMENT
    assert L.of2d_set_motion(None, None) == bad
    assert "of2d_set_motion: ctx is NULL" in L.of2d_last_error(None).decode()
    assert L.of2d_set_motion_device(None, None, None) == bad
    assert "of2d_set_motion_device: ctx is NULL" in L.of2d_last_error(None).decode()
    assert L.of2d_reset_motion(None) == bad
    assert "of2d_reset_motion: ctx is NULL" in L.of2d_last_error(None).decode()
    h = _create(L)
    assert L.of2d_set_motion(h, None) == bad
    assert L.of2d_last_error(h).decode() == "of2d_set_motion: motion is NULL"
    assert L.of2d_set_motion_device(h, None, None) == bad
    assert L.of2d_last_error(h).decode() == "of2d_set_motion_device: motion is NULL"
    a = _lib.DArray()
    a.ptr, a.dtype = None, _lib.OF2D_F32
    a.stride[:] = [0, 2 * 12, 2, 1]
    assert L.of2d_set_motion_device(h, C.byref(a), None) == bad
    assert L.of2d_last_error(h).decode() == "of2d_set_motion_device: motion.ptr is NULL"
    a.ptr, a.dtype = 4096, -3
    assert L.of2d_set_motion_device(h, C.byref(a), None) == bad
    assert L.of2d_last_error(h).decode() == \
        "of2d_set_motion_device: motion.dtype is neither OF2D_F32 nor OF2D_F64"
    a.dtype = _lib.OF2D_F32
    a.stride[1] = -24
    assert L.of2d_set_motion_device(h, C.byref(a), None) == bad
    assert L.of2d_last_error(h).decode() == "of2d_set_motion_device: motion has a negative stride"
    # the context is still usable
    assert L.of2d_set_option(h, b"fixed_iters", 1.0) == _lib.OF2D_OK
    assert L.of2d_destroy(h) == _lib.OF2D_OK


@pytest.fixture
def quiet():
    """of2d_create prints the reference's banner: keep it off the test output."""
    from opticalflow2d_amd import set_print_sink
    set_print_sink(lambda s: None)
    yield
    set_print_sink(None)


@pytest.mark.parametrize("reg, params", [(0, [0.1]), (2, [1.0, 1.0]), (5, [1.0, 1.0]),
                                         (3, [1.0, 2.0, 1.0, 1.0, 5, 0])])
def test_python_class_checks_the_shape(of2d_lib, quiet, reg, params):
    from opticalflow2d_amd import ImageRegistration
    with ImageRegistration((16, 12), [4, 4], 1, reg, params) as r:
        want = r"expected \(16, 12, 2\)"
        for shape in [(16, 12), (12, 16, 2), (16, 12, 3), (1, 16, 12, 2)]:
            with pytest.raises(ValueError, match=want):
                r.set_motion(np.zeros(shape))
