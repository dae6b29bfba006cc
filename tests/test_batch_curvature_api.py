"""Curvature on the batched interface, on the CPU (include/of2d.h
of2d_batch_*): reg 1 creates a handle when every pyramid level's sides are
powers of two from 8 to 512, every other reg 1 request is refused with the
sentence the other methods' refusals use, and BatchRegistration takes
``reg=Regularisation.Curvature``.  No device is needed: the checks precede any
device work.  The chunk and scratch arithmetic of the loop (csrc/batch_plan.h)
runs in the stand-alone program tests/host/batch_curvature_plan_test.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PARAM_COUNT = "Invalid number of regularisation parameters for given regularisation method."
METHODS = "Diffusion regularisation only"


def _create(L, nbatch=2, dimx=16, dimy=8, niter=None, nscales=0, params=(0.5, 0.2)):
    h = C.c_void_p()
    nit = np.ascontiguousarray(np.asarray(niter or [4] * (nscales + 1), np.int32))
    p = np.ascontiguousarray(np.asarray(params, np.float32))
    rc = L.of2d_batch_create(C.byref(h), nbatch, dimx, dimy, nit, nscales, 1, p, len(params), 1)
    return rc, h, L.of2d_batch_last_error(None).decode()


@pytest.mark.parametrize("kw", [
    dict(params=(0.5,)),                  # tau = 1
    dict(params=(0.5, 0.2)),
    dict(dimx=64, dimy=64, nscales=3),    # the coarsest level is 8 x 8
    dict(dimx=512, dimy=512),
])
def test_reg1_creates_a_handle(of2d_lib, kw):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib, **kw)
    assert rc == _lib.OF2D_OK and h.value, msg
    assert of2d_lib.of2d_batch_destroy(h) == _lib.OF2D_OK


@pytest.mark.parametrize("kw, text", [
    (dict(dimx=16, dimy=12), METHODS),              # a side that is no power of two
    (dict(dimx=4, dimy=8), METHODS),                # a side below 8
    (dict(dimx=64, dimy=64, nscales=4), METHODS),   # a 4 x 4 level
    (dict(dimx=1024, dimy=256), METHODS),           # within OF2D_BATCH_MAXPX, a side above 512
    (dict(params=(0.5, 0.2, 0.1)), PARAM_COUNT),
])
def test_create_refusals(of2d_lib, kw, text):
    from opticalflow2d_amd import _lib
    rc, h, msg = _create(of2d_lib, **kw)
    assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert not h.value
    assert text in msg


def test_refusal_names_the_third_method(of2d_lib):
    _, _, msg = _create(of2d_lib, dimx=16, dimy=12)
    assert "Curvature" in msg and "powers of two from 8 to 512" in msg


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


def test_python_class_takes_reg(of2d_lib):
    from opticalflow2d_amd import BatchRegistration, InvalidArgument, Regularisation
    assert Regularisation.Curvature == 1
    with BatchRegistration(3, (64, 32), [4, 4, 4], 2, [0.5, 0.2], nrefine=2,
                           reg=Regularisation.Curvature, fixed_iters=1) as b:
        assert (b.nbatch, b.dimx, b.dimy, b.loops, b.reg) == (3, 64, 32, 6, 1)
        assert b.iterations().shape == (3, 6) and not b.iterations().any()
        assert b.status().shape == (3,) and not b.status().any()
        with pytest.raises(InvalidArgument, match="resident"):
            b.set_option("resident", 1)
        b.set_option("warm_start", 1)
    with pytest.raises(InvalidArgument, match=METHODS):
        BatchRegistration(3, (64, 32), [4] * 4, 3, [0.5], reg=Regularisation.Curvature)  # 8 x 4
    with pytest.raises(InvalidArgument, match="Invalid number of regularisation parameters"):
        BatchRegistration(3, (64, 32), [4], 0, [0.5, 0.2, 0.1], reg=1)


def test_header_and_docs_name_the_method():
    with open(os.path.join(HERE, "..", "include", "of2d.h")) as f:
        h = f.read()
    assert "#define OF2D_BATCH_CURV_NMAX 512" in h
    from opticalflow2d_amd import batch
    assert "Curvature" in batch.__doc__ and "Curvature" in batch.BatchRegistration.__doc__


def test_curvature_plan_host_program(tmp_path):
    """The Curvature loop's chunk and scratch arithmetic (csrc/batch_plan.h) on
    the CPU, without HIP and without libof2d.so."""
    exe = str(tmp_path / "batch_curvature_plan_test")
    csrc = os.path.join(HERE, "..", "opticalflow2d_amd", "csrc")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall",
                           "-Wextra", "-I" + csrc, "-o", exe,
                           os.path.join(HERE, "host", "batch_curvature_plan_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout, r.stdout
