"""The batched deformation analysis at the C-ABI and in Python, on the CPU
(include/of2d.h of2d_batch_jacobian / _invert_motion / _quality and their
_device forms; csrc/of2d_prims.h of2d_prim_batch_*): the symbols exist and the
tables are in step, and every refusal returns OF2D_ERR_INVALID_ARGUMENT with
its message.  No device is needed: on a machine without one any device work
would answer OF2D_ERR_DEVICE instead, so the status itself shows that a
refusal launched nothing.  The host arithmetic of the calls (staging rounds,
offsets, argument checks: csrc/batch_plan.h) runs in the stand-alone program
tests/host/batch_plan_test.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT = ["of2d_batch_jacobian", "of2d_batch_invert_motion", "of2d_batch_quality",
           "of2d_batch_jacobian_device", "of2d_batch_invert_motion_device",
           "of2d_batch_quality_device"]
PRIMS = ["of2d_prim_batch_jacobian", "of2d_prim_batch_invert", "of2d_prim_batch_similarity"]
SMALL = "needs dimx >= 2 and dimy >= 2"


def test_symbols_and_tables(of2d_lib):
    from opticalflow2d_amd import _lib
    for n in PRODUCT:
        assert n in _lib.PRODUCT_SIGNATURES and n not in _lib.PRIM_SIGNATURES
        assert hasattr(of2d_lib, n), f"libof2d.so does not export {n}"
    for n in PRIMS:
        assert n in _lib.PRIM_SIGNATURES and n not in _lib.PRODUCT_SIGNATURES
        assert hasattr(of2d_lib, n), f"libof2d.so does not export {n}"
    with open(os.path.join(HERE, "..", "include", "of2d.h")) as f:
        product_h = f.read()
    with open(os.path.join(HERE, "..", "opticalflow2d_amd", "csrc", "of2d_prims.h")) as f:
        prims_h = f.read()
    for n in PRODUCT:
        assert f"int {n}(" in product_h
    for n in PRIMS:
        assert f"int {n}(" in prims_h and f"{n}(" not in product_h


@pytest.fixture
def batch(of2d_lib):
    """(library, handle factory): HS batches, destroyed after the test."""
    made = []

    def make(nbatch=3, dimx=16, dimy=12):
        h = C.c_void_p()
        rc = of2d_lib.of2d_batch_create(C.byref(h), nbatch, dimx, dimy, np.array([3], np.int32),
                                        0, 0, np.array([0.1], np.float32), 1, 1)
        assert rc == 0 and h.value
        made.append(h)
        return h

    yield of2d_lib, make
    for h in made:
        of2d_lib.of2d_batch_destroy(h)


def refused(L, h, rc, text):
    from opticalflow2d_amd import _lib
    assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT
    msg = L.of2d_batch_last_error(h).decode()
    assert text in msg, msg


def darr(ptr=0x1000, dtype=0, stride=(192, 1, 16, 0)):
    from opticalflow2d_amd import _lib
    a = _lib.DArray()
    a.ptr, a.dtype = ptr, dtype
    for k, s in enumerate(stride):
        a.stride[k] = s
    return a


def test_null_handle(of2d_lib):
    from opticalflow2d_amd import _lib
    d = np.zeros(64)
    p = d.ctypes.data
    a = darr()
    for rc in (of2d_lib.of2d_batch_jacobian(None, None, p),
               of2d_lib.of2d_batch_invert_motion(None, 5, 1e-3, None, p),
               of2d_lib.of2d_batch_quality(None, p, 0, p, p),
               of2d_lib.of2d_batch_jacobian_device(None, None, p, None),
               of2d_lib.of2d_batch_invert_motion_device(None, 5, 1e-3, C.byref(a), p, None),
               of2d_lib.of2d_batch_quality_device(None, C.byref(a), 0, C.byref(a), p, None)):
        assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT
        assert "b is NULL" in of2d_lib.of2d_gateway_last_error().decode()


def test_null_results(batch):
    L, make = batch
    h = make()
    buf = np.zeros(3 * 16 * 12 * 2)
    p = buf.ctypes.data
    a = darr()
    refused(L, h, L.of2d_batch_jacobian(h, p, None), "of2d_batch_jacobian: stats is NULL")
    refused(L, h, L.of2d_batch_jacobian_device(h, None, None, None),
            "of2d_batch_jacobian_device: stats is NULL")
    refused(L, h, L.of2d_batch_invert_motion(h, 5, 1e-3, p, None),
            "of2d_batch_invert_motion: info is NULL")
    refused(L, h, L.of2d_batch_invert_motion_device(h, 5, 1e-3, C.byref(a), None, None),
            "of2d_batch_invert_motion_device: info is NULL")
    for args in ((None, 0, p, p), (p, 0, None, p), (p, 1, p, None)):
        refused(L, h, L.of2d_batch_quality(h, *args),
                "of2d_batch_quality: Iref, Imov or out is NULL")
    refused(L, h, L.of2d_batch_quality_device(h, C.byref(a), 0, C.byref(a), None, None),
            "of2d_batch_quality_device: out is NULL")


@pytest.mark.parametrize("max_iter, tol, text", [
    (0, 1e-3, "invert: max_iter < 1"),
    (-4, 1e-3, "invert: max_iter < 1"),
    (5, 0.0, "invert: tol must be finite and > 0"),
    (5, -1e-3, "invert: tol must be finite and > 0"),
    (5, float("nan"), "invert: tol must be finite and > 0"),
    (5, float("inf"), "invert: tol must be finite and > 0"),
])
def test_invert_arguments(batch, max_iter, tol, text):
    L, make = batch
    h = make()
    out, info = np.zeros(3 * 16 * 12 * 2), np.zeros(3 * 4)
    refused(L, h, L.of2d_batch_invert_motion(h, max_iter, tol, out.ctypes.data, info.ctypes.data),
            text)
    a = darr(stride=(384, 1, 16, 192))
    refused(L, h, L.of2d_batch_invert_motion_device(h, max_iter, tol, C.byref(a),
                                                    info.ctypes.data, None), text)
    assert not info.any()


@pytest.mark.parametrize("dims", [(1, 12), (16, 1), (1, 1)])
def test_one_pixel_wide_fields(batch, dims):
    L, make = batch
    h = make(2, *dims)
    st, out = np.zeros(2 * 5), np.zeros(2 * 2 * 16 * 12)
    refused(L, h, L.of2d_batch_jacobian(h, None, st.ctypes.data), "jacobian: the field " + SMALL)
    refused(L, h, L.of2d_batch_jacobian(h, out.ctypes.data, st.ctypes.data),
            "jacobian: the field " + SMALL)
    refused(L, h, L.of2d_batch_jacobian_device(h, None, st.ctypes.data, None),
            "jacobian: the field " + SMALL)
    refused(L, h, L.of2d_batch_invert_motion(h, 5, 1e-3, out.ctypes.data, st.ctypes.data),
            "invert: the field " + SMALL)
    assert not st.any() and not out.any()


def test_darray_refusals(batch):
    L, make = batch
    h = make()
    w = np.zeros(3 * 5)
    p = w.ctypes.data
    good = darr()
    cases = [(None, " is NULL"), (darr(ptr=None), ".ptr is NULL"),
             (darr(dtype=7), ".dtype is neither OF2D_F32 nor OF2D_F64"),
             (darr(stride=(192, -1, 16, 0)), " has a negative stride")]
    for bad, text in cases:
        ref = None if bad is None else C.byref(bad)
        if bad is not None:  # a NULL map is "statistics only", not a refusal
            refused(L, h, L.of2d_batch_jacobian_device(h, ref, p, None),
                    "of2d_batch_jacobian_device: jac" + text)
        refused(L, h, L.of2d_batch_invert_motion_device(h, 5, 1e-3, ref, p, None),
                "of2d_batch_invert_motion_device: out" + text)
        refused(L, h, L.of2d_batch_quality_device(h, ref, 0, C.byref(good), p, None),
                "of2d_batch_quality_device: Iref" + text)
        refused(L, h, L.of2d_batch_quality_device(h, C.byref(good), 1, ref, p, None),
                "of2d_batch_quality_device: Imov" + text)
    # an output's elements must be distinct; an input may repeat them
    zero = darr(stride=(0, 1, 16, 0))
    refused(L, h, L.of2d_batch_jacobian_device(h, C.byref(zero), p, None),
            "jac has a zero stride on an axis of extent > 1")
    zero = darr(stride=(384, 1, 16, 0))
    refused(L, h, L.of2d_batch_invert_motion_device(h, 5, 1e-3, C.byref(zero), p, None),
            "out has a zero stride on an axis of extent > 1")
    assert not w.any()


def test_prim_refusals(of2d_lib):
    from opticalflow2d_amd import _lib
    L = of2d_lib
    u, v = np.zeros((2, 3, 4, 2), np.float32), np.zeros((2, 3, 4, 2), np.float32)
    img = np.zeros((2, 3, 4), np.float32)
    st, info, sim = np.zeros((2, 5)), np.zeros((2, 4)), np.zeros((2, 2))

    def msg():
        return L.of2d_gateway_last_error().decode()

    bad = _lib.OF2D_ERR_INVALID_ARGUMENT
    assert L.of2d_prim_batch_jacobian(u, 0, 4, 3, None, st) == bad and "B outside" in msg()
    assert L.of2d_prim_batch_jacobian(u, 65536, 4, 3, None, st) == bad and "B outside" in msg()
    assert L.of2d_prim_batch_jacobian(u, 2, 1, 3, None, st) == bad and SMALL in msg()
    assert L.of2d_prim_batch_invert(u, 2, 4, 1, 5, 1e-3, v, info, None) == bad and SMALL in msg()
    assert L.of2d_prim_batch_invert(u, 2, 4, 3, 0, 1e-3, v, info, None) == bad
    assert "max_iter < 1" in msg()
    assert L.of2d_prim_batch_invert(u, 2, 4, 3, 5, float("nan"), v, info, None) == bad
    assert "tol must be finite" in msg()
    assert L.of2d_prim_batch_invert(u, 0, 4, 3, 5, 1e-3, v, info, None) == bad
    assert L.of2d_prim_batch_similarity(img, 0, img, 2, 0, 3, sim) == bad and "empty image" in msg()
    assert L.of2d_prim_batch_similarity(img, 0, img, 0, 4, 3, sim) == bad and "B outside" in msg()
    assert not st.any() and not info.any() and not sim.any()


def test_python_shapes(of2d_lib):
    from opticalflow2d_amd import BatchRegistration, InvalidArgument
    from opticalflow2d_amd.prims import prim
    with BatchRegistration(3, (16, 12), [3], 0, 0.1) as b:
        good = np.zeros((3, 16, 12))
        for ref, mov in ((np.zeros((12, 16)), good), (np.zeros((2, 16, 12)), good),
                         (good, np.zeros((3, 12, 16))), (good, np.zeros((16, 12)))):
            with pytest.raises(ValueError, match="expected"):
                b.quality(ref, mov)
        with pytest.raises(ValueError, match="max_iter"):
            b.inverse_motion(max_iter=0)
        with pytest.raises(ValueError, match="tol"):
            b.inverse_motion(tol=0.0)
        with pytest.raises(ValueError, match="not a CUDA tensor"):
            b.jacobian(out=np.zeros((3, 16, 12)))
        with pytest.raises(ValueError, match="not a CUDA tensor"):
            b.inverse_motion(out=np.zeros((3, 16, 12, 2)))
    with BatchRegistration(2, (1, 12), [3], 0, 0.1) as b:
        with pytest.raises(InvalidArgument, match=SMALL):
            b.jacobian()
        with pytest.raises(InvalidArgument, match=SMALL):
            b.inverse_motion()
    with pytest.raises(ValueError, match="stack of motion fields"):
        prim.batch_jacobian(np.zeros((3, 4, 2), np.float32))
    with pytest.raises(ValueError, match="stack of motion fields"):
        prim.batch_invert(np.zeros((2, 3, 4, 3), np.float32))
    with pytest.raises(ValueError, match="stack of images"):
        prim.batch_similarity(np.zeros((3, 4), np.float32), np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="expected"):
        prim.batch_similarity(np.zeros((4, 3), np.float32), np.zeros((2, 3, 4), np.float32))


def test_batch_plan_host_program(tmp_path):
    """csrc/batch_plan.h on the CPU, without HIP and without libof2d.so."""
    exe = str(tmp_path / "batch_plan_test")
    csrc = os.path.join(HERE, "..", "opticalflow2d_amd", "csrc")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall",
                           "-Wextra", "-I" + csrc, "-o", exe,
                           os.path.join(HERE, "host", "batch_plan_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout, r.stdout
