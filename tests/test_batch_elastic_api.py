"""Elastic on the batched interface, on the CPU (include/of2d.h of2d_batch_*):
reg 2 with its three parameters [mu, lambda, omega] creates a handle at any
size the batch takes, reg 2 with any other parameter count is refused with the
sentence the other methods' refusals use (the reference's two-parameter form
included: the Python class appends the default omega itself), and reg 4 and 5
stay refused.  No device is needed: the checks precede any device work.  The
step arithmetic of the loop's sweep (csrc/batch_plan.h) runs in the stand-alone
program tests/host/batch_elastic_plan_test.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
METHODS = "Diffusion regularisation only"


def _create(L, nbatch=2, dimx=16, dimy=12, niter=None, nscales=0, reg=2, params=(0.5, 0.25, 0.9)):
    h = C.c_void_p()
    nit = np.ascontiguousarray(np.asarray(niter or [4] * (nscales + 1), np.int32))
    p = np.ascontiguousarray(np.asarray(params, np.float32))
    rc = L.of2d_batch_create(C.byref(h), nbatch, dimx, dimy, nit, nscales, reg, p, len(params), 1)
    return rc, h, L.of2d_batch_last_error(None).decode()


@pytest.mark.parametrize("kw", [
    dict(),                                # 16 x 12
    dict(dimx=3, dimy=3),                  # one interior pixel
    dict(dimx=2, dimy=7),                  # no interior
    dict(dimx=512, dimy=512),              # OF2D_BATCH_MAXPX
    dict(dimx=1024, dimy=256),             # more columns than a workgroup has threads
    dict(dimx=64, dimy=36, nscales=2),
])
def test_reg2_with_three_parameters_creates_a_handle(of2d_lib, kw):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib, **kw)
    assert rc == _lib.OF2D_OK and h.value, msg
    assert of2d_lib.of2d_batch_destroy(h) == _lib.OF2D_OK


@pytest.mark.parametrize("params", [(0.5,), (0.5, 0.25), (0.5, 0.25, 0.9, 0.1)])
def test_reg2_with_another_parameter_count_is_refused(of2d_lib, params):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib, params=params)
    assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert not h.value
    assert METHODS in msg
    assert "Elastic" in msg and "[mu, lambda, omega]" in msg
    # what the refusals of the other methods look for
    assert "Curvature" in msg and "powers of two from 8 to 512" in msg


@pytest.mark.parametrize("reg, params", [
    (4, (1.0, 1.0, 1.0, 1.0, 3.0)),
    (5, (0.5, 0.25)),
    (5, (0.5, 0.25, 0.9)),
])
def test_the_unbatched_methods_stay_refused(of2d_lib, reg, params):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib, reg=reg, params=params)
    assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert not h.value
    assert METHODS in msg and "Elastic" in msg


def test_size_rules_are_the_batchs_own(of2d_lib):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib, dimx=513, dimy=512)
    assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT and "OF2D_BATCH_MAXPX" in msg
    rc, h, msg = _create(of2d_lib, dimx=16, dimy=12, nscales=4)
    assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT and "pyramid level with zero size" in msg


@pytest.mark.parametrize("key, text", [
    ("resident", "resident: the batch is not a Diffusion batch"),
    ("conv_lds", "conv_lds: the batch is not a Thirion's Demons batch"),
    ("diffeomorphic", "diffeomorphic: the batch is not a Thirion's Demons batch"),
])
def test_options_of_the_other_methods_are_refused(of2d_lib, key, text):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib)
    assert rc == _lib.OF2D_OK, msg
    try:
        assert of2d_lib.of2d_batch_set_option(h, key.encode(), 1.0) == \
            _lib.OF2D_ERR_INVALID_ARGUMENT
        assert text in of2d_lib.of2d_batch_last_error(h).decode()
        # the handle is usable afterwards
        for ok in ("fixed_iters", "warm_start"):
            assert of2d_lib.of2d_batch_set_option(h, ok.encode(), 1.0) == _lib.OF2D_OK
        st = np.full(2, -1, np.int32)
        assert of2d_lib.of2d_batch_status(h, st.ctypes.data_as(C.POINTER(C.c_int))) == _lib.OF2D_OK
        assert st.tolist() == [_lib.OF2D_OK] * 2
    finally:
        of2d_lib.of2d_batch_destroy(h)


def test_python_class_takes_two_or_three_parameters(of2d_lib, monkeypatch):
    from opticalflow2d_amd import BatchRegistration, InvalidArgument, Regularisation
    assert Regularisation.Elastic == 2
    seen = []
    real = of2d_lib.of2d_batch_create

    def spy(h, nbatch, dimx, dimy, nit, nscales, reg, p, nparams, nrefine):
        seen.append(np.array(p[:nparams], np.float32))
        return real(h, nbatch, dimx, dimy, nit, nscales, reg, p, nparams, nrefine)

    monkeypatch.setattr(of2d_lib, "of2d_batch_create", spy)
    with BatchRegistration(3, (64, 36), [4, 4, 4], 2, [0.3, 0.1], nrefine=2,
                           reg=Regularisation.Elastic, fixed_iters=1) as b:
        assert (b.nbatch, b.dimx, b.dimy, b.loops, b.reg) == (3, 64, 36, 6, 2)
        assert b.iterations().shape == (3, 6) and not b.iterations().any()
        assert b.status().shape == (3,) and not b.status().any()
        with pytest.raises(InvalidArgument, match="resident"):
            b.set_option("resident", 1)
        b.set_option("warm_start", 1)
    # the class appended the reference's default omega, bit for bit
    assert seen[-1].tobytes() == np.array([0.3, 0.1, 0.66], np.float32).tobytes()
    with BatchRegistration(1, (3, 3), [4], 0, [0.5, 0.25, 0.9], reg=2) as b:
        assert b.reg == 2
    assert seen[-1].tobytes() == np.array([0.5, 0.25, 0.9], np.float32).tobytes()
    for alpha in ([0.5], [0.5, 0.25, 0.9, 0.1]):
        with pytest.raises(InvalidArgument, match=METHODS):
            BatchRegistration(1, (16, 12), [4], 0, alpha, reg=Regularisation.Elastic)
    # the other methods' parameters are passed on as they are
    with BatchRegistration(1, (16, 12), [4], 0, [0.5]) as b:
        assert b.reg == 0
    assert seen[-1].tobytes() == np.array([0.5], np.float32).tobytes()


def test_header_and_docs_name_the_method():
    with open(os.path.join(HERE, "..", "include", "of2d.h")) as f:
        h = f.read()
    assert "OF2D_REG_ELASTIC" in h and "{mu, lambda, omega}" in h
    from opticalflow2d_amd import batch
    assert "Elastic" in batch.__doc__ and "Elastic" in batch.BatchRegistration.__doc__
    assert "0.66" in batch.BatchRegistration.__doc__


def test_elastic_plan_host_program(tmp_path):
    """The Elastic loop's step arithmetic (csrc/batch_plan.h) on the CPU,
    without HIP and without libof2d.so."""
    exe = str(tmp_path / "batch_elastic_plan_test")
    csrc = os.path.join(HERE, "..", "opticalflow2d_amd", "csrc")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall",
                           "-Wextra", "-I" + csrc, "-o", exe,
                           os.path.join(HERE, "host", "batch_elastic_plan_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout, r.stdout
