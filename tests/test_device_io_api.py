"""The device-resident I/O interface on the CPU (include/of2d.h of2d_*_device,
of2d_darray): the symbols, every refusal that precedes device work with its
message, the Python classes' ValueErrors, and the dispatch rule (only torch
CUDA tensors leave the host path).  No device is needed.

Not covered anywhere: a pointer on another device than the context's is
refused once the device is known (hipPointerGetAttributes); that needs two
GPUs and cannot be tested on a one-GPU box.
"""
import ctypes as C

import numpy as np
import pytest

DEVICE_SYMBOLS = ["of2d_set_images_device", "of2d_get_motion_device", "of2d_warp_device",
                  "of2d_batch_set_images_device", "of2d_batch_get_motion_device",
                  "of2d_batch_warp_device", "of2d_prim_pack_image", "of2d_prim_unpack_image",
                  "of2d_prim_unpack_motion", "of2d_prim_pack_motion", "of2d_prim_planar_to_motion",
                  "of2d_prim_pack_layout"]

DIMX, DIMY, NB = 16, 12, 3
FAKE = 0x1000  # never dereferenced: every call below is refused on the host


def test_symbols_exported_and_in_signatures(of2d_lib):
    from opticalflow2d_amd import _lib
    for n in DEVICE_SYMBOLS:
        assert hasattr(of2d_lib, n), f"libof2d.so does not export {n}"
        assert n in _lib.SIGNATURES
    assert (_lib.OF2D_F32, _lib.OF2D_F64) == (0, 1)
    # void *, int, long long[4] with the C compiler's padding
    assert C.sizeof(_lib.DArray) == 48 and _lib.DArray.stride.offset == 16


def darr(ptr=FAKE, dtype=0, stride=(DIMX * DIMY, 1, DIMX, DIMX * DIMY)):
    from opticalflow2d_amd import _lib
    a = _lib.DArray()
    a.ptr, a.dtype = ptr, dtype
    for k, s in enumerate(stride):
        a.stride[k] = s
    return a


def ref(a):
    return None if a is None else C.byref(a)


@pytest.fixture()
def ctx(of2d_lib):
    h = C.c_void_p()
    rc = of2d_lib.of2d_create(C.byref(h), DIMX, DIMY, np.array([3], np.int32), 0, 0,
                              np.array([0.1], np.float32), 1, 1, 0)
    assert rc == 0
    yield h
    of2d_lib.of2d_destroy(h)


@pytest.fixture()
def batch(of2d_lib):
    h = C.c_void_p()
    rc = of2d_lib.of2d_batch_create(C.byref(h), NB, DIMX, DIMY, np.array([3], np.int32), 0, 0,
                                    np.array([0.1], np.float32), 1, 1)
    assert rc == 0
    yield h
    of2d_lib.of2d_batch_destroy(h)


# (bad array, message): refused whether the array is read or written
BAD_ANY = [
    (None, "is NULL"),
    (darr(ptr=None), ".ptr is NULL"),
    (darr(dtype=2), ".dtype is neither OF2D_F32 nor OF2D_F64"),
    (darr(dtype=-1), ".dtype is neither OF2D_F32 nor OF2D_F64"),
    (darr(stride=(DIMX * DIMY, -1, DIMX, 1)), "has a negative stride"),
    (darr(stride=(DIMX * DIMY, 1, -DIMX, 1)), "has a negative stride"),
]
# refused for an output only: a zero stride on x or y (extent > 1)
BAD_OUT = [
    (darr(stride=(DIMX * DIMY, 0, DIMX, DIMX * DIMY)), "zero stride on an axis of extent > 1"),
    (darr(stride=(DIMX * DIMY, 1, 0, DIMX * DIMY)), "zero stride on an axis of extent > 1"),
]
# batch outputs: the pair axis; motion outputs: the component axis
BAD_PAIR = (darr(stride=(0, 1, DIMX, DIMX * DIMY)), "zero stride on an axis of extent > 1")
BAD_COMP = (darr(stride=(2 * DIMX * DIMY, 1, DIMX, 0)), "zero stride on an axis of extent > 1")
NEG_PAIR = (darr(stride=(-1, 1, DIMX, DIMX * DIMY)), "has a negative stride")
NEG_COMP = (darr(stride=(2 * DIMX * DIMY, 1, DIMX, -1)), "has a negative stride")


def refused(L, rc, msg, fn, name, text):
    from opticalflow2d_amd import _lib
    assert rc == _lib.OF2D_ERR_INVALID_ARGUMENT, (fn, name, text)
    assert msg.startswith(f"{fn}: {name}") and text in msg, msg


def test_context_refusals(of2d_lib, ctx):
    L = of2d_lib
    ok = darr()

    def err():
        return L.of2d_last_error(ctx).decode()

    for bad, text in BAD_ANY:
        fn = "of2d_set_images_device"
        refused(L, L.of2d_set_images_device(ctx, ref(bad), ref(ok), None), err(), fn, "Iref", text)
        refused(L, L.of2d_set_images_device(ctx, ref(ok), ref(bad), None), err(), fn, "Imov", text)
        fn = "of2d_warp_device"
        refused(L, L.of2d_warp_device(ctx, ref(bad), ref(ok), None), err(), fn, "Imov", text)
    for bad, text in BAD_ANY + BAD_OUT:
        refused(L, L.of2d_warp_device(ctx, ref(ok), ref(bad), None), err(), "of2d_warp_device",
                "out", text)
    for bad, text in BAD_ANY + BAD_OUT + [BAD_COMP, NEG_COMP]:
        refused(L, L.of2d_get_motion_device(ctx, ref(bad), None), err(),
                "of2d_get_motion_device", "out", text)
    # a NULL context
    from opticalflow2d_amd import _lib
    assert L.of2d_get_motion_device(None, ref(ok), None) == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert "ctx is NULL" in L.of2d_gateway_last_error().decode()


def test_batch_refusals(of2d_lib, batch):
    L = of2d_lib
    ok = darr()

    def err():
        return L.of2d_batch_last_error(batch).decode()

    fn = "of2d_batch_set_images_device"
    for bad, text in BAD_ANY + [NEG_PAIR]:
        refused(L, L.of2d_batch_set_images_device(batch, ref(bad), 0, ref(ok), None), err(), fn,
                "Iref", text)
        refused(L, L.of2d_batch_set_images_device(batch, ref(ok), 0, ref(bad), None), err(), fn,
                "Imov", text)
        refused(L, L.of2d_batch_warp_device(batch, ref(bad), ref(ok), None), err(),
                "of2d_batch_warp_device", "Imov", text)
    # a shared reference has no pair axis: its pair stride is not looked at, so
    # the refusal is Imov's
    refused(L, L.of2d_batch_set_images_device(batch, ref(NEG_PAIR[0]), 1, ref(darr(dtype=5)), None),
            err(), fn, "Imov", ".dtype")
    for bad, text in BAD_ANY + BAD_OUT + [BAD_PAIR, NEG_PAIR]:
        refused(L, L.of2d_batch_warp_device(batch, ref(ok), ref(bad), None), err(),
                "of2d_batch_warp_device", "out", text)
    for bad, text in BAD_ANY + BAD_OUT + [BAD_PAIR, NEG_PAIR, BAD_COMP, NEG_COMP]:
        refused(L, L.of2d_batch_get_motion_device(batch, ref(bad), None), err(),
                "of2d_batch_get_motion_device", "out", text)
    from opticalflow2d_amd import _lib
    assert L.of2d_batch_warp_device(None, ref(ok), ref(ok), None) == _lib.OF2D_ERR_INVALID_ARGUMENT
    assert "b is NULL" in L.of2d_gateway_last_error().decode()


def test_primitive_refusals(of2d_lib):
    from opticalflow2d_amd import _lib
    L = of2d_lib
    host = np.zeros(NB * DIMX * DIMY * 2, np.float32)

    def err():
        return L.of2d_gateway_last_error().decode()

    for bad, text in BAD_ANY + [NEG_PAIR]:
        refused(L, L.of2d_prim_pack_image(ref(bad), NB, DIMX, DIMY, host, None), err(),
                "of2d_prim_pack_image", "in", text)
    for bad, text in BAD_ANY + BAD_OUT + [BAD_PAIR, NEG_PAIR]:
        refused(L, L.of2d_prim_unpack_image(host, NB, DIMX, DIMY, ref(bad)), err(),
                "of2d_prim_unpack_image", "out", text)
    for bad, text in BAD_ANY + BAD_OUT + [BAD_PAIR, BAD_COMP, NEG_COMP]:
        refused(L, L.of2d_prim_unpack_motion(host, NB, DIMX, DIMY, ref(bad)), err(),
                "of2d_prim_unpack_motion", "out", text)
    for args in [(0, DIMX, DIMY), (NB, 0, DIMY), (NB, DIMX, -1), (65536, DIMX, DIMY)]:
        assert L.of2d_prim_pack_image(ref(darr()), *args, host, None) == \
            _lib.OF2D_ERR_INVALID_ARGUMENT
        assert "size is out of range" in err()


def test_pack_motion_refusals(of2d_lib):
    """of2d_prim_pack_motion reads its array: unpack motion's refusals less
    those of an output (a zero stride is a broadcast), and a host pointer;
    of2d_prim_planar_to_motion and of2d_prim_pack_layout take host arguments."""
    from opticalflow2d_amd import _lib
    L = of2d_lib
    bad_rc = _lib.OF2D_ERR_INVALID_ARGUMENT
    host = np.zeros(NB * DIMX * DIMY * 2, np.float32)
    planar = np.zeros(NB * DIMX * DIMY * 2, np.float64)
    sizes = [(0, DIMX, DIMY), (NB, 0, DIMY), (NB, DIMX, -1), (65536, DIMX, DIMY)]

    def err():
        return L.of2d_gateway_last_error().decode()

    for bad, text in BAD_ANY + [NEG_PAIR, NEG_COMP]:
        refused(L, L.of2d_prim_pack_motion(ref(bad), NB, DIMX, DIMY, host, None), err(),
                "of2d_prim_pack_motion", "in", text)
    for args in sizes:
        assert L.of2d_prim_pack_motion(ref(darr()), *args, host, None) == bad_rc
        assert err() == "of2d_prim_pack_motion: out_host is NULL or a size is out of range"
    # a host pointer as the device array: refused before anything is allocated
    on_host = np.zeros(NB * DIMX * DIMY * 2, np.float32)
    a = darr(ptr=on_host.ctypes.data, stride=(2 * DIMX * DIMY, 2, 2 * DIMX, 1))
    assert L.of2d_prim_pack_motion(ref(a), NB, DIMX, DIMY, host, None) == bad_rc
    assert err() == "of2d_prim_pack_motion: in.ptr is not a device pointer"
    assert not host.any()

    text = "of2d_prim_planar_to_motion: planar_host or out_host is NULL or a size is out of range"
    for args in sizes:
        assert L.of2d_prim_planar_to_motion(planar, *args, host, None) == bad_rc and err() == text
    # NULL arrays: the table's ndpointer admits no None
    fn = L.of2d_prim_planar_to_motion
    saved, fn.argtypes = fn.argtypes, [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 2
    try:
        for p, o in ((None, host.ctypes.data), (planar.ctypes.data, None)):
            assert fn(p, NB, DIMX, DIMY, o, None) == bad_rc and err() == text
    finally:
        fn.argtypes = saved

    stride, P = C.c_longlong(-1), C.c_int(-1)
    for args in [(0, DIMY, C.byref(stride), C.byref(P)), (DIMX, 0, C.byref(stride), C.byref(P)),
                 (DIMX, DIMY, None, C.byref(P)), (DIMX, DIMY, C.byref(stride), None)]:
        assert L.of2d_prim_pack_layout(*args) == bad_rc
        assert err().startswith("of2d_prim_pack_layout:")
    assert (stride.value, P.value) == (-1, -1)
    # of2d_batch.h: a ghost j-line either side of the rows, one pitch unit of slack
    assert L.of2d_prim_pack_layout(DIMX, DIMY, C.byref(stride), C.byref(P)) == _lib.OF2D_OK
    assert (stride.value, P.value) == ((DIMY + 2) * 128 + 128, 128)
    assert L.of2d_prim_pack_layout(129, 1, C.byref(stride), C.byref(P)) == _lib.OF2D_OK
    assert (stride.value, P.value) == (3 * 256 + 128, 256)


# ------------------------------------------------------------ the Python classes
@pytest.fixture()
def fake_cuda(monkeypatch, of2d_lib):
    """Every torch tensor counts as a CUDA tensor, and every device entry
    fails the test: what is checked must be raised before the library."""
    import torch
    from opticalflow2d_amd import _device

    def entered(*a):
        raise AssertionError("the library was entered")

    monkeypatch.setattr(_device, "is_cuda", lambda a: isinstance(a, torch.Tensor))
    for n in DEVICE_SYMBOLS:
        monkeypatch.setattr(of2d_lib, n, entered)
    return torch


def test_image_registration_value_errors(fake_cuda):
    torch = fake_cuda
    from opticalflow2d_amd import ImageRegistration, set_print_sink
    set_print_sink(lambda s: None)
    good = torch.zeros(DIMX, DIMY)
    with ImageRegistration((DIMX, DIMY), [3], 0, 0, [0.1]) as r:
        for bad, text in [(torch.zeros(DIMY, DIMX), "expected"), (torch.zeros(DIMX, DIMY, 1), "expected"),
                          (torch.zeros(DIMX, DIMY, dtype=torch.float16), "float32 or torch.float64"),
                          (torch.zeros(DIMX, DIMY, dtype=torch.int32), "float32 or torch.float64")]:
            for call in (lambda: r.register(bad, good), lambda: r.set_images(good, bad),
                         lambda: r.warp(bad), lambda: r.warp(good, out=bad)):
                with pytest.raises(ValueError, match=text):
                    call()
        # CUDA and host arrays in one call
        host = np.zeros((DIMX, DIMY))
        for call in (lambda: r.register(good, host), lambda: r.register(host, good),
                     lambda: r.warp(good, out=host), lambda: r.warp(host, out=good)):
            with pytest.raises(ValueError, match="CUDA tensors and host arrays in one call"):
                call()
        with pytest.raises(ValueError, match="out= is for CUDA tensors"):
            r.warp(host, out=np.zeros((DIMX, DIMY)))
        with pytest.raises(ValueError, match="expected"):
            r.motion_device(out=torch.zeros(DIMX, DIMY))
        with pytest.raises(ValueError, match="float32 or torch.float64"):
            r.motion_device(out=torch.zeros(DIMX, DIMY, 2, dtype=torch.float16))
    set_print_sink(None)


def test_batch_registration_value_errors(fake_cuda):
    torch = fake_cuda
    from opticalflow2d_amd import BatchRegistration
    stack = torch.zeros(NB, DIMX, DIMY)
    with BatchRegistration(NB, (DIMX, DIMY), [3], 0, 0.1) as b:
        for bad in (torch.zeros(DIMX), torch.zeros(NB - 1, DIMX, DIMY), torch.zeros(DIMY, DIMX),
                    torch.zeros(1, NB, DIMX, DIMY)):
            with pytest.raises(ValueError, match="Iref is .* expected"):
                b.register(bad, stack)
        for bad in (torch.zeros(DIMX, DIMY), torch.zeros(NB, DIMY, DIMX)):
            with pytest.raises(ValueError, match="Imov is .* expected"):
                b.register(stack, bad)
            with pytest.raises(ValueError, match="expected"):
                b.warp(bad)
        with pytest.raises(ValueError, match="float32 or torch.float64"):
            b.register(stack, stack.to(torch.float16))
        with pytest.raises(ValueError, match="CUDA tensors and host arrays in one call"):
            b.register(np.zeros((DIMX, DIMY)), stack)
        with pytest.raises(ValueError, match="expected"):
            b.motion_device(out=torch.zeros(NB, DIMX, DIMY))


def test_out_must_be_cuda_and_dtype_checked(of2d_lib):
    """Without the fixture: a CPU tensor or a numpy array is no CUDA tensor."""
    import torch
    from opticalflow2d_amd import BatchRegistration, ImageRegistration, set_print_sink
    set_print_sink(lambda s: None)
    with ImageRegistration((DIMX, DIMY), [3], 0, 0, [0.1]) as r:
        for out in (torch.zeros(DIMX, DIMY, 2), np.zeros((DIMX, DIMY, 2), np.float32)):
            with pytest.raises(ValueError, match="out is not a CUDA tensor"):
                r.motion_device(out=out)
        with pytest.raises(ValueError, match="dtype is .* expected"):
            r.motion_device(dtype=torch.float16)
    with BatchRegistration(NB, (DIMX, DIMY), [3], 0, 0.1) as b:
        with pytest.raises(ValueError, match="out is not a CUDA tensor"):
            b.motion_device(out=torch.zeros(NB, DIMX, DIMY, 2))
        with pytest.raises(ValueError, match="dtype is .* expected"):
            b.motion_device(dtype=torch.int64)
    set_print_sink(None)


def test_cpu_tensors_take_the_host_path(of2d_lib, monkeypatch):
    import torch
    from opticalflow2d_amd import BatchRegistration, ImageRegistration, set_print_sink
    set_print_sink(lambda s: None)
    calls = []

    def entered(*a):
        raise AssertionError("a CPU tensor took the device path")

    def host(name):
        def f(*a):
            calls.append((name,) + tuple(x.copy() for x in a if isinstance(x, np.ndarray)))
            return 0
        return f

    for n in DEVICE_SYMBOLS:
        monkeypatch.setattr(of2d_lib, n, entered)
    for n in ("of2d_set_images", "of2d_estimate", "of2d_batch_set_images", "of2d_batch_estimate"):
        monkeypatch.setattr(of2d_lib, n, host(n))
    rng = np.random.default_rng(5)
    a, b2 = rng.random((DIMX, DIMY)), rng.random((DIMX, DIMY))
    with ImageRegistration((DIMX, DIMY), [3], 0, 0, [0.1]) as r:
        r.register(torch.from_numpy(a), torch.from_numpy(b2))
    assert [c[0] for c in calls] == ["of2d_set_images", "of2d_estimate"]
    # the boundary layout of the same doubles: x fastest
    assert np.array_equal(calls[0][1], a.reshape(-1, order="F"))
    assert np.array_equal(calls[0][2], b2.reshape(-1, order="F"))
    calls.clear()
    s = rng.random((NB, DIMX, DIMY)).astype(np.float32)
    with BatchRegistration(NB, (DIMX, DIMY), [3], 0, 0.1) as b:
        b.register(torch.from_numpy(s[0]), torch.from_numpy(s))
    assert [c[0] for c in calls] == ["of2d_batch_set_images", "of2d_batch_estimate"]
    assert np.array_equal(calls[0][2], s.astype(np.float64).transpose(0, 2, 1).reshape(-1))
    set_print_sink(None)
