"""The batch's warm start and motion input on the CPU (include/of2d.h option
"warm_start", of2d_batch_set_motion, _set_motion_device, _reset_motion): the
names are exported, and everything refused is refused with a named message
before any device work, the handle still usable.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

NAMES = ("of2d_batch_set_motion", "of2d_batch_set_motion_device", "of2d_batch_reset_motion")
DEMONS = (1.0, 2.0, 1.0, 1.0, 5, 0)
REFUSAL = "warm_start: the value must be 0 or 1"


def _create(L, reg=0, params=(0.1,), nscales=0):
    from opticalflow2d_amd import _lib
    h = C.c_void_p()
    nit = np.ascontiguousarray(np.asarray((5,) * (nscales + 1), np.int32))
    p = np.ascontiguousarray(np.asarray(params, np.float32))
    rc = L.of2d_batch_create(C.byref(h), 2, 16, 12, nit, nscales, reg, p, len(params), 1)
    assert rc == _lib.OF2D_OK and h.value, L.of2d_batch_last_error(None).decode()
    return h


def _set(L, h, value, key=b"warm_start"):
    rc = L.of2d_batch_set_option(h, key, float(value))
    return rc, L.of2d_batch_last_error(h).decode()


def test_symbols_exported_and_in_signatures(of2d_lib):
    from opticalflow2d_amd import _lib
    for n in NAMES:
        assert hasattr(of2d_lib, n), f"libof2d.so does not export {n}"
        assert n in _lib.SIGNATURES and n in _lib.PRODUCT_SIGNATURES


@pytest.mark.parametrize("kw", [dict(), dict(nscales=2), dict(reg=3, params=DEMONS),
                                dict(reg=3, params=DEMONS[:5] + (1,))])
def test_warm_start_is_taken_by_every_method(of2d_lib, kw):
    from opticalflow2d_amd import _lib
    h = _create(of2d_lib, **kw)
    for v in (1, 0, 1, 1, 0):
        rc, msg = _set(of2d_lib, h, v)
        assert rc == _lib.OF2D_OK, msg
    assert of2d_lib.of2d_batch_destroy(h) == _lib.OF2D_OK


@pytest.mark.parametrize("value", [2, -1, 0.5, float("nan")])
def test_a_value_other_than_0_or_1_is_refused(of2d_lib, value):
    from opticalflow2d_amd import _lib
    h = _create(of2d_lib)
    assert _set(of2d_lib, h, 1)[0] == _lib.OF2D_OK
    rc, msg = _set(of2d_lib, h, value)
    assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert msg == REFUSAL
    # usable, and both values are still taken
    assert _set(of2d_lib, h, 0)[0] == _lib.OF2D_OK
    assert _set(of2d_lib, h, 1)[0] == _lib.OF2D_OK
    assert _set(of2d_lib, h, 1, b"fixed_iters")[0] == _lib.OF2D_OK
    assert of2d_lib.of2d_batch_destroy(h) == _lib.OF2D_OK


def test_null_and_bad_arrays_are_refused_by_name(of2d_lib):
    from opticalflow2d_amd import _lib
    L = of2d_lib
    bad = _lib.OF2D_ERR_INVALID_ARGUMENT
    assert L.of2d_batch_set_motion(None, None) == bad
    assert "of2d_batch_set_motion: b is NULL" in L.of2d_batch_last_error(None).decode()
    assert L.of2d_batch_set_motion_device(None, None, None) == bad
    assert "of2d_batch_set_motion_device: b is NULL" in L.of2d_batch_last_error(None).decode()
    assert L.of2d_batch_reset_motion(None) == bad
    assert "of2d_batch_reset_motion: b is NULL" in L.of2d_batch_last_error(None).decode()
    h = _create(L)
    assert L.of2d_batch_set_motion(h, None) == bad
    assert L.of2d_batch_last_error(h).decode() == "of2d_batch_set_motion: motion is NULL"
    assert L.of2d_batch_set_motion_device(h, None, None) == bad
    assert L.of2d_batch_last_error(h).decode() == "of2d_batch_set_motion_device: motion is NULL"
    a = _lib.DArray()
    a.ptr, a.dtype = None, _lib.OF2D_F32
    a.stride[:] = [2 * 16 * 12, 2 * 12, 2, 1]
    assert L.of2d_batch_set_motion_device(h, C.byref(a), None) == bad
    assert L.of2d_batch_last_error(h).decode() == \
        "of2d_batch_set_motion_device: motion.ptr is NULL"
    a.ptr, a.dtype = 4096, 7
    assert L.of2d_batch_set_motion_device(h, C.byref(a), None) == bad
    assert L.of2d_batch_last_error(h).decode() == \
        "of2d_batch_set_motion_device: motion.dtype is neither OF2D_F32 nor OF2D_F64"
    a.dtype = _lib.OF2D_F64
    a.stride[3] = -1
    assert L.of2d_batch_set_motion_device(h, C.byref(a), None) == bad
    assert L.of2d_batch_last_error(h).decode() == \
        "of2d_batch_set_motion_device: motion has a negative stride"
    # the handle is still usable
    assert _set(L, h, 1)[0] == _lib.OF2D_OK
    assert L.of2d_batch_destroy(h) == _lib.OF2D_OK


def test_python_class(of2d_lib):
    from opticalflow2d_amd import BatchRegistration, InvalidArgument
    with BatchRegistration(3, (16, 12), [4, 4], 1, 0.1, nrefine=2, fixed_iters=1,
                           warm_start=1) as b:
        assert (b.nbatch, b.loops) == (3, 4)
        b.set_option("warm_start", 0)
        for v in (2, -1, 0.5):
            with pytest.raises(InvalidArgument, match=REFUSAL):
                b.set_option("warm_start", v)
        b.set_option("warm_start", 1)
        want = r"expected \(3, 16, 12, 2\)"
        for shape in [(3, 16, 12), (3, 12, 16, 2), (2, 16, 12, 2), (3, 16, 12, 3), (16, 12, 2)]:
            with pytest.raises(ValueError, match=want):
                b.set_motion(np.zeros(shape))
        assert b.status().tolist() == [0, 0, 0] and not b.iterations().any()
    with pytest.raises(InvalidArgument, match=REFUSAL):
        BatchRegistration(2, (16, 12), [4], 0, 0.1, warm_start=3)
    with BatchRegistration(2, (16, 12), [4], 0, list(DEMONS), reg=3, diffeomorphic=1,
                           warm_start=1) as b:
        assert b.reg == 3
