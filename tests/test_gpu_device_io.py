"""Device-resident I/O on the GPU (include/of2d.h of2d_*_device, io_kernels.hip,
DESIGN.md §4.7): torch CUDA tensors in, CUDA tensors out, against the same
objects fed host arrays.  Every comparison is bit for bit: a float64 tensor
gives what the host path gives for the same doubles, a float32 tensor what it
gives for the widened floats; a float64 output equals the host result, a
float32 output equals it once widened.

Tensors are built and read with copies (``torch.from_numpy(..).to("cuda")``,
``.cpu()``), ``torch.empty`` and views only.  Every unpack writes into a view
of a larger tensor filled with a sentinel, and the whole larger tensor is
compared: a store outside the view is a failed assertion.

Not covered: a pointer on another device than the context's is refused once
the device is known; that cannot be tested on a one-GPU box.
"""
import numpy as np
import pytest

from opticalflow2d_amd import synthetic as S

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
# cross the 64 x 64 tile's edge on each axis, sit on it, collapse an axis to 1;
# (70, 67): two tiles on both axes, both ragged (64 | 6 and 64 | 3)
SHAPES = [(64, 64), (65, 63), (1, 70), (70, 1), (130, 17), (70, 67)]
NPAIRS = [1, 3]
DTYPES = [np.float32, np.float64]
LAYOUTS = ["contiguous", "xfast", "sliced"]


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def big_shape(layout, n, dimx, dimy, tail=()):
    if layout == "contiguous":
        return (n + 2, dimx, dimy) + tail
    if layout == "xfast":
        return (n + 2, dimy, dimx) + tail
    return (n, 3 + 2 * dimx + 1, 5 + 3 * dimy + 2) + tail


def view(big, layout, dimx, dimy):
    """The ``[n, dimx, dimy(, 2)]`` view of the larger array (numpy or torch)."""
    if layout == "contiguous":
        return big[1:-1]
    if layout == "xfast":
        return big[1:-1].swapaxes(1, 2)
    return big[:, 3:3 + 2 * dimx:2, 5:5 + 3 * dimy:3]


def rand(shape, dtype, seed):
    # doubles that are no floats: the pack's rounding is exercised
    return np.random.default_rng(seed).standard_normal(shape).astype(dtype)


# ------------------------------------------------------------ primitives
@pytest.mark.parametrize("npairs", NPAIRS)
@pytest.mark.parametrize("dimx, dimy", SHAPES)
def test_pack_image(gpu, dimx, dimy, npairs):
    from opticalflow2d_amd import prim
    for dtype in DTYPES:
        img = rand((npairs, dimx, dimy), dtype, 1)
        want = np.ascontiguousarray(img.astype(np.float32).transpose(0, 2, 1))
        if dtype is np.float64:  # the host boundary's conversion of the same doubles
            for k in range(npairs):
                assert np.array_equal(prim.d2f(np.ascontiguousarray(img[k].T)), want[k])
        for layout in LAYOUTS:
            big = np.full(big_shape(layout, npairs, dimx, dimy), SENTINEL, dtype)
            view(big, layout, dimx, dimy)[...] = img
            got = prim.pack_image(view(cuda(big), layout, dimx, dimy))
            assert np.array_equal(got, want), (dtype, layout)
        # a pair stride of 0: one image read for every pair
        one = cuda(img[0])
        got = prim.pack_image(one.expand(npairs, dimx, dimy))
        assert np.array_equal(got, np.broadcast_to(want[0], want.shape)), (dtype, "expand")


@pytest.mark.parametrize("npairs", NPAIRS)
@pytest.mark.parametrize("dimx, dimy", SHAPES)
def test_unpack_image(gpu, dimx, dimy, npairs):
    from opticalflow2d_amd import prim
    field = rand((npairs, dimy, dimx), np.float32, 2)
    for dtype in DTYPES:
        for k in range(npairs) if dtype is np.float64 else ():
            assert np.array_equal(prim.f2d(field[k]), field[k].astype(np.float64))
        for layout in LAYOUTS:
            want = np.full(big_shape(layout, npairs, dimx, dimy), SENTINEL, dtype)
            big = cuda(want)
            view(want, layout, dimx, dimy)[...] = field.transpose(0, 2, 1).astype(dtype)
            prim.unpack_image(field, view(big, layout, dimx, dimy))
            assert np.array_equal(big.cpu().numpy(), want), (dtype, layout)


@pytest.mark.parametrize("npairs", NPAIRS)
@pytest.mark.parametrize("dimx, dimy", SHAPES)
def test_unpack_motion(gpu, dimx, dimy, npairs):
    from opticalflow2d_amd import prim
    m = rand((npairs, dimy, dimx, 2), np.float32, 3)
    for dtype in DTYPES:
        if dtype is np.float64:  # the host boundary's planar doubles
            for k in range(npairs):
                assert np.array_equal(prim.motion_to_planar(m[k]),
                                      m[k].transpose(2, 0, 1).astype(np.float64))
        # interleaved [.., dimx, dimy, 2]
        for layout in LAYOUTS:
            want = np.full(big_shape(layout, npairs, dimx, dimy, (2,)), SENTINEL, dtype)
            big = cuda(want)
            view(want, layout, dimx, dimy)[...] = m.transpose(0, 2, 1, 3).astype(dtype)
            prim.unpack_motion(m, view(big, layout, dimx, dimy))
            assert np.array_equal(big.cpu().numpy(), want), (dtype, layout)
        # interleaved at an odd element offset: the components' pair store is
        # not aligned and each goes alone
        want = np.full((npairs * dimx * dimy * 2 + 3,), SENTINEL, dtype)
        big = cuda(want)
        want[1:-2] = m.transpose(0, 2, 1, 3).astype(dtype).reshape(-1)
        prim.unpack_motion(m, big[1:-2].view(npairs, dimx, dimy, 2))
        assert np.array_equal(big.cpu().numpy(), want), (dtype, "odd offset")
        # planar [.., 2, dimy, dimx] (the boundary's layout) through the strides
        want = np.full((npairs + 2, 2, dimy, dimx), SENTINEL, dtype)
        big = cuda(want)
        want[1:-1] = m.transpose(0, 3, 1, 2).astype(dtype)
        prim.unpack_motion(m, big[1:-1], axes=(0, 3, 2, 1))
        assert np.array_equal(big.cpu().numpy(), want), (dtype, "planar")


# ------------------------------------------------------------ one pair
ONE = dict(dims=(67, 50), niter=[5, 6, 7], nscales=2, nrefine=2)
SOLVERS = {"diffusion": (0, [0.1], {}),
           "demons": (3, [1.0, 0.25, 2.0, 2.0, 5, 0], {}),
           "diffusion_2ranks": (0, [0.1], dict(ngpus=2, ngpus_share=1))}
_one = {}


def one_pair_inputs():
    if "in" not in _one:
        _one["in"] = S.texture_pair(67, seed=21, sigma=2.0, shift=(0.8, -0.6), ny=50)
    return _one["in"]


def registration(solver):
    from opticalflow2d_amd import ImageRegistration
    reg, params, opt = SOLVERS[solver]
    return ImageRegistration(ONE["dims"], ONE["niter"], ONE["nscales"], reg, params, ONE["nrefine"],
                             fixed_iters=1, device=0, **opt)


def host_result(solver, dtype):
    """The host path fed the doubles, or the widened floats."""
    key = (solver, dtype)
    if key not in _one:
        ref, mov = (a.astype(dtype).astype(np.float64) for a in one_pair_inputs())
        with registration(solver) as r:
            r.register(ref, mov)
            _one[key] = (r.iterations(), r.motion(), r.warp(mov))
    return _one[key]


@pytest.mark.parametrize("layout", ["contiguous", "sliced"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("solver", list(SOLVERS))
def test_one_pair(gpu, solver, dtype, layout):
    import torch
    dimx, dimy = ONE["dims"]
    iters, motion, warped = host_result(solver, dtype)
    assert iters == [7, 7, 6, 6, 5, 5]
    both = np.stack(one_pair_inputs()).astype(dtype)
    big = np.full(big_shape(layout, 2, dimx, dimy), SENTINEL, dtype)
    view(big, layout, dimx, dimy)[...] = both
    ref, mov = view(cuda(big), layout, dimx, dimy)
    with registration(solver) as r:
        r.register(ref, mov)
        assert r.iterations() == iters
        assert np.array_equal(r.motion(), motion)
        for out_dtype in (torch.float32, torch.float64):
            m = r.motion_device(dtype=out_dtype)
            assert m.dtype == out_dtype and m.is_cuda and tuple(m.shape) == (dimx, dimy, 2)
            assert np.array_equal(m.cpu().numpy().astype(np.float64), motion)
        # into a strided out=, the rest of its tensor untouched
        tdt = torch.float32 if dtype is np.float32 else torch.float64
        want = np.full(big_shape("sliced", 1, dimx, dimy, (2,)), SENTINEL, dtype)
        outbig = cuda(want)
        view(want, "sliced", dimx, dimy)[0] = motion.astype(dtype)
        assert r.motion_device(out=view(outbig, "sliced", dimx, dimy)[0]).dtype == tdt
        assert np.array_equal(outbig.cpu().numpy(), want)
        w = r.warp(mov)
        assert w.dtype == tdt and w.is_cuda and tuple(w.shape) == (dimx, dimy)
        assert np.array_equal(w.cpu().numpy().astype(np.float64), warped)
        want = np.full(big_shape(layout, 2, dimx, dimy), SENTINEL, dtype)
        outbig = cuda(want)
        view(want, layout, dimx, dimy)[1] = warped.astype(dtype)
        r.warp(mov, out=view(outbig, layout, dimx, dimy)[1])
        assert np.array_equal(outbig.cpu().numpy(), want)


# ------------------------------------------------------------ batch
from test_gpu_batch import ALPHA, make_pairs, run_batch  # noqa: E402

BATCH_CASES = [
    # dims, B, niter, nscales, nrefine, shared: test_gpu_batch.FIXED_CASES' shapes
    ((40, 33), 3, [7], 0, 1, False),
    ((130, 17), 5, [6, 9], 1, 1, True),
    ((9, 300), 2, [5, 6], 1, 1, False),
]


def run_batch_device(dims, niter, nscales, alpha, nrefine, refs, movs, out_dtype, **opt):
    from opticalflow2d_amd import BatchRegistration
    with BatchRegistration(len(movs), dims, niter, nscales, alpha, nrefine, device=0, **opt) as b:
        b.register(refs, movs)
        return {"motion": b.motion_device(dtype=out_dtype).cpu().numpy().astype(np.float64),
                "motion_host": b.motion(),
                "warp": b.warp(movs).cpu().numpy().astype(np.float64), "iters": b.iterations(),
                "status": b.status(), "info": b.info(), "error": b.last_error()}


def same(got, want):
    assert np.array_equal(got["motion"], want["motion"])
    assert np.array_equal(got["motion_host"], want["motion"])
    assert np.array_equal(got["warp"], want["warp"])
    assert np.array_equal(got["iters"], want["iters"])
    assert np.array_equal(got["status"], want["status"])
    assert got["error"] == want["error"]
    assert got["info"]["launches"] == want["info"]["launches"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims, B, niter, nscales, nrefine, shared", BATCH_CASES)
def test_batch(gpu, dims, B, niter, nscales, nrefine, shared, dtype):
    import torch
    dimx, dimy = dims
    refs, movs = (a.astype(dtype) for a in make_pairs(dims, B, shared))
    want = run_batch(dims, niter, nscales, ALPHA, nrefine, refs.astype(np.float64),
                     movs.astype(np.float64), fixed_iters=1)
    out_dtype = torch.float64 if dtype is np.float32 else torch.float32
    # the moving stack as a sliced view, the reference contiguous
    big = np.full(big_shape("sliced", B, dimx, dimy), SENTINEL, dtype)
    view(big, "sliced", dimx, dimy)[...] = movs
    tmov = view(cuda(big), "sliced", dimx, dimy)
    tref = cuda(refs)
    same(run_batch_device(dims, niter, nscales, ALPHA, nrefine, tref, tmov, out_dtype,
                          fixed_iters=1), want)
    if shared:
        # the one reference as B references through a pair stride of 0, x fast
        tref = cuda(refs.T).t().expand(B, dimx, dimy)
        assert tref.stride() == (0, 1, dimx)
        same(run_batch_device(dims, niter, nscales, ALPHA, nrefine, tref, cuda(movs), out_dtype,
                              fixed_iters=1), want)


def test_batch_divide_by_zero_is_per_pair(gpu):
    import torch
    from opticalflow2d_amd import _lib
    dims, niter, bad = (40, 33), [5], 2
    refs, movs = make_pairs(dims, 4)
    refs[bad] = 0.5
    movs[bad] = 0.5
    want = run_batch(dims, niter, 0, 0.0, 1, refs, movs, fixed_iters=1)
    got = run_batch_device(dims, niter, 0, 0.0, 1, cuda(refs), cuda(movs), torch.float64,
                           fixed_iters=1)
    same(got, want)
    assert got["status"].tolist() == [_lib.OF2D_OK, _lib.OF2D_OK, _lib.OF2D_ERR_RUNTIME,
                                      _lib.OF2D_OK]
    assert f"pair {bad}" in got["error"] and not got["motion"][bad].any()


def test_batch_launches_do_not_depend_on_batch_size(gpu):
    import torch
    dims, niter = (67, 50), [5, 6, 7]
    refs, movs = make_pairs(dims, 7)
    one = run_batch_device(dims, niter, 2, ALPHA, 2, cuda(refs[:1]), cuda(movs[:1]),
                           torch.float32, fixed_iters=1)
    all7 = run_batch_device(dims, niter, 2, ALPHA, 2, cuda(refs), cuda(movs), torch.float32,
                            fixed_iters=1)
    assert one["info"]["launches"] == all7["info"]["launches"] > 0
    assert np.array_equal(one["motion"][0], all7["motion"][0])


# ------------------------------------------------------------ stream order
@pytest.mark.parametrize("default_stream", [False, True])
@pytest.mark.parametrize("batched", [False, True])
def test_stream_order(gpu, batched, default_stream):
    """The input is filled by an asynchronous copy and the result read by
    one, both on the caller's stream; only that stream is synchronised."""
    import torch
    from opticalflow2d_amd import BatchRegistration, ImageRegistration
    dims, B, niter = (40, 33), 3, [7]
    refs, movs = (a.astype(np.float32) for a in make_pairs(dims, B))
    if batched:
        want = run_batch(dims, niter, 0, ALPHA, 1, refs.astype(np.float64),
                         movs.astype(np.float64), fixed_iters=1)["motion"]
        obj = BatchRegistration(B, dims, niter, 0, ALPHA, 1, device=0, fixed_iters=1)
    else:
        refs, movs = refs[0], movs[0]
        with ImageRegistration(dims, niter, 0, 0, [ALPHA], 1, device=0, fixed_iters=1) as r:
            r.register(refs.astype(np.float64), movs.astype(np.float64))
            want = r.motion()
        obj = ImageRegistration(dims, niter, 0, 0, [ALPHA], 1, device=0, fixed_iters=1)
    pin_in = torch.from_numpy(np.stack([refs, movs])).pin_memory()
    pin_out = torch.empty(want.shape, dtype=torch.float32).pin_memory()
    s = torch.cuda.default_stream() if default_stream else torch.cuda.Stream()
    with obj:
        with torch.cuda.stream(s):
            dev = torch.empty(pin_in.shape, dtype=torch.float32, device="cuda")
            dev.copy_(pin_in, non_blocking=True)
            obj.register(dev[0], dev[1])
            m = obj.motion_device()
            pin_out.copy_(m, non_blocking=True)
        s.synchronize()
        assert np.array_equal(pin_out.numpy().astype(np.float64), want)
