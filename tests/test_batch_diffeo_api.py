"""The batch option "diffeomorphic" on the CPU (include/of2d.h
of2d_batch_set_option): accepted on a Thirion's Demons batch with Composition,
refused everywhere else with a message that names the reason, and a refusal
leaves the handle usable.  No device is needed: the checks precede any device
work."""
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


def _set(L, h, value, key=b"diffeomorphic"):
    rc = L.of2d_batch_set_option(h, key, float(value))
    return rc, L.of2d_batch_last_error(h).decode()


def test_accepted_on_a_thirion_composition_batch(of2d_lib):
    from opticalflow2d_amd import _lib
    h = _create(of2d_lib)
    for v in (1, 0, 1, 1, 0):
        rc, msg = _set(of2d_lib, h, v)
        assert rc == _lib.OF2D_OK, msg
    assert of2d_lib.of2d_batch_destroy(h) == _lib.OF2D_OK


@pytest.mark.parametrize("kw, text", [
    (dict(reg=0, params=(0.1,)), "diffeomorphic: the batch is not a Thirion's Demons batch"),
    (dict(params=DEMONS[:5] + (1,)), "diffeomorphic: accumulation must be Composition (0)"),
    (dict(params=DEMONS[:5] + (2,)), "diffeomorphic: accumulation must be Composition (0)"),
])
def test_refused_on_every_other_handle(of2d_lib, kw, text):
    from opticalflow2d_amd import _lib
    h = _create(of2d_lib, **kw)
    for v in (1, 0):  # the handle, not the value, is what is refused
        rc, msg = _set(of2d_lib, h, v)
        assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT
        assert text in msg
    # still usable: another option is taken, and the handle closes
    rc, msg = _set(of2d_lib, h, 1, b"fixed_iters")
    assert rc == _lib.OF2D_OK, msg
    assert of2d_lib.of2d_batch_destroy(h) == _lib.OF2D_OK


@pytest.mark.parametrize("value", [2, -1, float("nan"), 0.5])
def test_a_value_other_than_0_or_1_is_refused(of2d_lib, value):
    from opticalflow2d_amd import _lib
    h = _create(of2d_lib)
    assert _set(of2d_lib, h, 1)[0] == _lib.OF2D_OK
    rc, msg = _set(of2d_lib, h, value)
    assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert "diffeomorphic" in msg and "0 or 1" in msg
    # usable, and both values are still taken
    assert _set(of2d_lib, h, 0)[0] == _lib.OF2D_OK
    assert _set(of2d_lib, h, 1)[0] == _lib.OF2D_OK
    assert of2d_lib.of2d_batch_destroy(h) == _lib.OF2D_OK


def test_python_class_takes_the_keyword(of2d_lib):
    from opticalflow2d_amd import BatchRegistration, InvalidArgument
    with BatchRegistration(3, (16, 12), [4, 4], 1, list(DEMONS), nrefine=2, reg=3,
                           fixed_iters=1, diffeomorphic=1) as b:
        assert (b.nbatch, b.loops, b.reg) == (3, 4, 3)
        assert b.status().tolist() == [0, 0, 0] and b.last_error() == ""
        b.set_option("diffeomorphic", 0)
        b.set_option("diffeomorphic", 1)
        with pytest.raises(InvalidArgument, match="diffeomorphic: the value must be 0 or 1"):
            b.set_option("diffeomorphic", 2)
        b.set_option("diffeomorphic", 1)
        assert not b.iterations().any()
    with pytest.raises(InvalidArgument, match="not a Thirion's Demons batch"):
        BatchRegistration(2, (16, 12), [4], 0, 0.1, diffeomorphic=1)
    with pytest.raises(InvalidArgument, match=r"accumulation must be Composition \(0\)"):
        BatchRegistration(2, (16, 12), [4], 0, list(DEMONS[:5]) + [1], reg=3, diffeomorphic=1)
    # reg 4 itself stays refused at create
    with pytest.raises(InvalidArgument, match="Diffusion regularisation only"):
        BatchRegistration(2, (16, 12), [4], 0, list(DEMONS[:5]), reg=4)
