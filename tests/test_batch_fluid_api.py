"""Fluid on the batched interface, on the CPU (include/of2d.h, option "fluid"):
the option is accepted on an Elastic handle and refused elsewhere with its own
sentences, of2d_batch_create goes on refusing reg 5, the Python class turns
Regularisation.Fluid into the Elastic handle with the option set, the log is
empty before an estimate, and the formatter of the reference's lines is a pure
function of the log.  No device is needed: every check precedes device work."""
import ctypes as C
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
METHODS = "Diffusion regularisation only"
DEMONS = (1.0, 1.0, 1.0, 1.0, 3.0, 0.0)


def _create(L, nbatch=2, dimx=16, dimy=12, niter=None, nscales=0, reg=2, params=(0.5, 0.25, 0.9)):
    h = C.c_void_p()
    nit = np.ascontiguousarray(np.asarray(niter or [4] * (nscales + 1), np.int32))
    p = np.ascontiguousarray(np.asarray(params, np.float32))
    rc = L.of2d_batch_create(C.byref(h), nbatch, dimx, dimy, nit, nscales, reg, p, len(params), 1)
    return rc, h, L.of2d_batch_last_error(None).decode()


def _usable(L, h, nbatch=2):
    from opticalflow2d_amd import _lib
    for ok in ("fixed_iters", "warm_start"):
        assert L.of2d_batch_set_option(h, ok.encode(), 1.0) == _lib.OF2D_OK
    st = np.full(nbatch, -1, np.int32)
    assert L.of2d_batch_status(h, st.ctypes.data_as(C.POINTER(C.c_int))) == _lib.OF2D_OK
    assert st.tolist() == [_lib.OF2D_OK] * nbatch


def test_option_is_accepted_on_an_elastic_handle(of2d_lib):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib)
    assert rc == _lib.OF2D_OK, msg
    try:
        for v in (1.0, 0.0, 1.0):
            assert of2d_lib.of2d_batch_set_option(h, b"fluid", v) == _lib.OF2D_OK
        # it composes with these, and the other methods' options stay refused
        _usable(of2d_lib, h)
        for key in ("resident", "conv_lds", "diffeomorphic"):
            assert of2d_lib.of2d_batch_set_option(h, key.encode(), 1.0) == \
                _lib.OF2D_ERR_INVALID_ARGUMENT
    finally:
        of2d_lib.of2d_batch_destroy(h)


@pytest.mark.parametrize("reg, params", [(0, (0.1,)), (1, (0.1,)), (3, DEMONS)])
def test_option_is_refused_on_another_method(of2d_lib, reg, params):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib, dimx=16, dimy=16, reg=reg, params=params)
    assert rc == _lib.OF2D_OK, msg
    try:
        for v in (1.0, 0.0):
            assert of2d_lib.of2d_batch_set_option(h, b"fluid", v) == _lib.OF2D_ERR_INVALID_ARGUMENT
            assert "fluid: the batch is not an Elastic batch" in \
                of2d_lib.of2d_batch_last_error(h).decode()
        _usable(of2d_lib, h)
        assert of2d_lib.of2d_batch_fluid_log(h, 0, 0, np.zeros(16, np.float32), 4) == 0
    finally:
        of2d_lib.of2d_batch_destroy(h)


@pytest.mark.parametrize("value", [2.0, -1.0, 0.5, float("nan")])
def test_option_takes_0_or_1(of2d_lib, value):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib)
    assert rc == _lib.OF2D_OK, msg
    try:
        assert of2d_lib.of2d_batch_set_option(h, b"fluid", value) == _lib.OF2D_ERR_INVALID_ARGUMENT
        assert "fluid: the value must be 0 or 1" in of2d_lib.of2d_batch_last_error(h).decode()
        _usable(of2d_lib, h)
        assert of2d_lib.of2d_batch_set_option(h, b"fluid", 1.0) == _lib.OF2D_OK
    finally:
        of2d_lib.of2d_batch_destroy(h)


@pytest.mark.parametrize("kw", [
    dict(dimx=16, dimy=1),
    dict(dimx=1, dimy=16),
    dict(dimx=16, dimy=2, nscales=1),   # level 1 is 8 x 1
    dict(dimx=3, dimy=40, nscales=1),   # level 1 is 1 x 20
])
def test_option_needs_sides_of_at_least_2(of2d_lib, kw):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib, **kw)
    assert rc == _lib.OF2D_OK, msg  # the Elastic batch takes the size
    try:
        assert of2d_lib.of2d_batch_set_option(h, b"fluid", 1.0) == _lib.OF2D_ERR_INVALID_ARGUMENT
        assert "fluid: every level needs sides of at least 2" in \
            of2d_lib.of2d_batch_last_error(h).decode()
        # 0 is what the handle has: nothing to refuse
        assert of2d_lib.of2d_batch_set_option(h, b"fluid", 0.0) == _lib.OF2D_OK
        _usable(of2d_lib, h)
    finally:
        of2d_lib.of2d_batch_destroy(h)
    # the smallest level the option takes
    rc, h, msg = _create(of2d_lib, dimx=4, dimy=4, nscales=1)
    assert rc == _lib.OF2D_OK, msg
    assert of2d_lib.of2d_batch_set_option(h, b"fluid", 1.0) == _lib.OF2D_OK
    of2d_lib.of2d_batch_destroy(h)


@pytest.mark.parametrize("params", [(0.5, 0.25), (0.5, 0.25, 0.9)])
def test_create_still_refuses_reg_5(of2d_lib, params):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib, reg=5, params=params)
    assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT and not h.value
    for text in (METHODS, "Elastic", "[mu, lambda, omega]", "Curvature",
                 "powers of two from 8 to 512"):
        assert text in msg, text
    # the sentence points to the option
    assert "Fluid" in msg and '"fluid"' in msg


def test_log_is_empty_before_an_estimate(of2d_lib):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib)
    assert rc == _lib.OF2D_OK, msg
    try:
        buf = np.full(16, 7.0, np.float32)
        assert of2d_lib.of2d_batch_fluid_log(h, 0, 0, buf, 4) == 0   # no option
        assert of2d_lib.of2d_batch_set_option(h, b"fluid", 1.0) == _lib.OF2D_OK
        assert of2d_lib.of2d_batch_fluid_log(h, 0, 0, buf, 4) == 0   # no estimate
        assert of2d_lib.of2d_batch_fluid_log(h, 1, 0, buf, 4) == 0
        assert (buf == 7.0).all()
        # a pair or a loop the batch does not have
        for pair, loop in [(2, 0), (-1, 0), (0, 1), (0, -1)]:
            assert of2d_lib.of2d_batch_fluid_log(h, pair, loop, buf, 4) == -1
    finally:
        of2d_lib.of2d_batch_destroy(h)


def test_python_class_creates_the_elastic_handle(of2d_lib, monkeypatch):
    from opticalflow2d_amd import BatchRegistration, InvalidArgument, Regularisation
    assert Regularisation.Fluid == 5
    seen, opts = [], []
    real, real_opt = of2d_lib.of2d_batch_create, of2d_lib.of2d_batch_set_option

    def spy(h, nbatch, dimx, dimy, nit, nscales, reg, p, nparams, nrefine):
        seen.append((reg, np.array(p[:nparams], np.float32)))
        return real(h, nbatch, dimx, dimy, nit, nscales, reg, p, nparams, nrefine)

    def spy_opt(h, key, value):
        opts.append((key, value))
        return real_opt(h, key, value)

    monkeypatch.setattr(of2d_lib, "of2d_batch_create", spy)
    monkeypatch.setattr(of2d_lib, "of2d_batch_set_option", spy_opt)
    with BatchRegistration(3, (64, 36), [4, 4, 4], 2, [0.3, 0.1], nrefine=2,
                           reg=Regularisation.Fluid, fixed_iters=1) as b:
        assert (b.nbatch, b.dimx, b.dimy, b.loops, b.reg) == (3, 64, 36, 6, 5)
        assert b.iterations().shape == (3, 6) and not b.iterations().any()
        assert b.status().shape == (3,) and not b.status().any()
        with pytest.raises(InvalidArgument, match="resident"):
            b.set_option("resident", 1)
        b.set_option("warm_start", 1)
        log = b.fluid_log(1)
        assert len(log) == 6 and all(a.shape == (0, 4) and a.dtype == np.float32 for a in log)
        assert b.fluid_lines(1) == []
        with pytest.raises(ValueError):
            b.fluid_log(3)
    reg, p = seen[-1]
    assert reg == 2
    assert p.tobytes() == np.array([0.3, 0.1, 0.66], np.float32).tobytes()
    assert (b"fluid", 1.0) in opts
    # three parameters pass as they are; reg=2 with fluid=1 is the same handle
    opts.clear()
    with BatchRegistration(1, (3, 3), [4], 0, [0.5, 0.25, 0.9], reg=5) as b:
        assert b.reg == 5
    assert seen[-1][0] == 2
    assert seen[-1][1].tobytes() == np.array([0.5, 0.25, 0.9], np.float32).tobytes()
    assert (b"fluid", 1.0) in opts
    opts.clear()
    with BatchRegistration(1, (3, 3), [4], 0, [0.5, 0.25, 0.9], reg=2, fluid=1) as b:
        assert b.reg == 2 and len(b.fluid_log(0)) == 1
    assert seen[-1][0] == 2 and (b"fluid", 1.0) in opts
    # a level with a side of 1 is the option's refusal, through the class too
    with pytest.raises(InvalidArgument, match="sides of at least 2"):
        BatchRegistration(1, (16, 2), [4, 4], 1, [0.5, 0.25], reg=Regularisation.Fluid)
    for alpha in ([0.5], [0.5, 0.25, 0.9, 0.1]):
        with pytest.raises(InvalidArgument, match=METHODS):
            BatchRegistration(1, (16, 12), [4], 0, alpha, reg=Regularisation.Fluid)


def test_line_formatter_on_a_hand_made_log():
    from opticalflow2d_amd.batch import fluid_lines
    inf = np.float32(np.inf)
    log = [
        np.array([[1.23449, 0.5265, 0.9, 0.0],
                  [0.5, 1.3, 0.49951, 1.0],     # regridded at iteration 1
                  [0.0, inf, 1.0, 0.0]], np.float32),
        np.zeros((0, 4), np.float32),           # a loop that ran nothing
        np.array([[0.001, 650.0, 0.25, 1.0]], np.float32),
    ]
    assert fluid_lines(log) == [
        "Dumax: 0.650\tMaxabs increment: 1.234\t Timestep: 0.526",
        "Dumax: 0.650\tMaxabs increment: 0.500\t Timestep: 1.300",
        "Regridding on iteration: 1\tMin Jacobian: 0.500",
        "Dumax: 0.650\tMaxabs increment: 0.000\t Timestep: inf",
        "Dumax: 0.650\tMaxabs increment: 0.001\t Timestep: 650.000",
        "Regridding on iteration: 0\tMin Jacobian: 0.250",
    ]
    assert fluid_lines([]) == []
    # the values are the float32 records widened, as printf's (double) casts
    one = fluid_lines([np.array([[np.float32(0.1), np.float32(6.5), 1.0, 0.0]])])
    assert one == ["Dumax: 0.650\tMaxabs increment: 0.100\t Timestep: 6.500"]


def test_header_and_docs_name_the_option():
    with open(os.path.join(HERE, "..", "include", "of2d.h")) as f:
        h = f.read()
    assert '"fluid"' in h and "of2d_batch_fluid_log" in h
    flat = " ".join(h.replace("\n *", " ").split())  # the comment's line breaks taken out
    assert "fluid: the batch is not an Elastic batch" in flat
    assert "fluid: every level needs sides of at least 2" in flat
    assert "of2d_batch_set_motion leaves it as it is" in flat
    assert "max(niter) records of 16 bytes" in flat
    assert "are not batched" not in flat
    from opticalflow2d_amd import batch
    assert "Fluid" in batch.__doc__ and "Regularisation.Fluid" in batch.BatchRegistration.__doc__
    assert "fluid" in batch.BatchRegistration.fluid_log.__doc__
    assert "Dumax" in batch.fluid_lines.__doc__
