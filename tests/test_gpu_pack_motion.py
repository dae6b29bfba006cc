"""The pack-motion kernels of io_kernels.hip, one launch each (`prim.pack_motion`,
`prim.planar_to_motion`), at tests/test_gpu_device_io.py's shapes: a caller's
strided motion stack, or the host form's planar doubles, into the pitched
float2 fields.  The expected value is numpy's float32 of every component; every
comparison is by bit pattern.

Which of the four kernels of an element type a layout takes is decided by
`launch_pack_motion_t` from the strides and the pointer; `selection` restates
that rule, and every case asserts on the CPU, before its launch, that the
layout takes the kernel it is named for.  At (70, 67) every kernel runs two
blocks along x and two tiles along y, ragged on both (64 | 6 and 64 | 3).

`test_pack_leaves_slack_and_ghost_lines` is the pack's counterpart of the
unpack tests' sentinel on the caller's tensor: the test entries fill the
pitched fields with 0xC5 bytes before the launch and return the whole
allocation, which must hold the converted pixels and the sentinel everywhere
else: in the ghost j-lines, right of dimx in every row, and in the slack.
"""
import numpy as np
import pytest

from test_gpu_device_io import DTYPES, NPAIRS, SHAPES, big_shape, cuda, rand, view

pytestmark = pytest.mark.gpu

MULTI = (70, 67)  # the one shape with more than one tile on both axes
# layout -> (pattern, one load of both components): the kernel it is named for
LAYOUTS = {
    "contiguous": ("tile", True),     # [n, dimx, dimy, 2]: y faster than x
    "xfast": ("rows", True),          # a permuted [n, dimy, dimx, 2]
    "sliced": ("tile", True),         # even strides, none of them the extent's
    "expand": ("tile", True),         # a pair stride of 0
    "odd_rows": ("rows", False),      # [.., :2] of a [n, dimy, dimx, 3]: x stride 3
    "odd_tile": ("tile", False),      # [.., :2] of a [n, dimx, dimy, 3]: y stride 3
    "planar_rows": ("rows", False),   # [n, 2, dimy, dimx] through axes
    "planar_tile": ("tile", False),   # [n, 2, dimx, dimy] through axes
    "offset_rows": ("rows", False),   # the base one element off the pair's alignment
    "offset_tile": ("tile", False),
}
INTERLEAVED = (0, 1, 2, 3)


def build(layout, m):
    """``m`` ([n, dimx, dimy, 2], numpy) on the device in ``layout``: ``(tensor,
    axes, the [n, dimx, dimy, 2] values the launch must read)``."""
    import torch
    n, dimx, dimy, _ = m.shape
    if layout == "contiguous":
        return cuda(m), INTERLEAVED, m
    if layout in ("xfast", "sliced"):  # views of a larger tensor, as the mirror tests'
        big = np.full(big_shape(layout, n, dimx, dimy, (2,)), 7.0, m.dtype)
        view(big, layout, dimx, dimy)[...] = m
        return view(cuda(big), layout, dimx, dimy), INTERLEAVED, m
    if layout == "expand":
        return cuda(m[0]).expand(n, dimx, dimy, 2), INTERLEAVED, np.broadcast_to(m[0], m.shape)
    if layout == "odd_rows":
        big = np.full((n, dimy, dimx, 3), 7.0, m.dtype)
        big[..., :2] = m.transpose(0, 2, 1, 3)
        return cuda(big)[..., :2].permute(0, 2, 1, 3), INTERLEAVED, m
    if layout == "odd_tile":
        big = np.full((n, dimx, dimy, 3), 7.0, m.dtype)
        big[..., :2] = m
        return cuda(big)[..., :2], INTERLEAVED, m
    if layout == "planar_rows":
        return cuda(m.transpose(0, 3, 2, 1)), (0, 3, 2, 1), m
    if layout == "planar_tile":
        return cuda(m.transpose(0, 3, 1, 2)), (0, 3, 1, 2), m
    flat = torch.full((m.size + 1,), 7.0, device="cuda",
                      dtype=torch.float32 if m.dtype == np.float32 else torch.float64)
    if layout == "offset_rows":
        flat[1:] = cuda(m.transpose(0, 2, 1, 3)).reshape(-1)
        return flat[1:].view(n, dimy, dimx, 2).permute(0, 2, 1, 3), INTERLEAVED, m
    assert layout == "offset_tile"
    flat[1:] = cuda(m).reshape(-1)
    return flat[1:].view(n, dimx, dimy, 2), INTERLEAVED, m


def selection(t, axes):
    """launch_pack_motion_t's rule on the tensor's strides and pointer."""
    s = dict(zip(axes, t.stride()))
    rows = s[1] <= s[2]
    vec2 = (s[3] == 1 and t.data_ptr() % (2 * t.element_size()) == 0 and s[0] % 2 == 0 and
            s[1] % 2 == 0 and s[2] % 2 == 0)
    return ("rows" if rows else "tile"), vec2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def fields_of(m):
    """[n, dimx, dimy, 2] of any dtype -> the fields' float32 [n, dimy, dimx, 2]."""
    return np.ascontiguousarray(m.astype(np.float32).transpose(0, 2, 1, 3))


# ------------------------------------------------------------ pack motion
@pytest.mark.parametrize("npairs", NPAIRS)
@pytest.mark.parametrize("dimx, dimy", SHAPES)
def test_pack_motion(gpu, dimx, dimy, npairs):
    from opticalflow2d_amd import prim
    for dtype in DTYPES:
        m = rand((npairs, dimx, dimy, 2), dtype, 4)
        if dtype is np.float64:  # doubles that are no floats
            assert not np.array_equal(m.astype(np.float32).astype(np.float64), m)
        for layout, named in LAYOUTS.items():
            t, axes, read = build(layout, m)
            ext = dict(zip(axes, t.shape))
            assert (ext[0], ext[1], ext[2], ext[3]) == (npairs, dimx, dimy, 2), layout
            if dimx > 1 and dimy > 1:  # an axis of extent 1 has no stride to speak of
                assert selection(t, axes) == named, (dtype, layout, t.stride())
            got = prim.pack_motion(t, axes)
            assert np.array_equal(bits(got), bits(fields_of(read))), (dtype, layout)


def test_every_instantiation_runs_at_the_multi_tile_shape(gpu):
    """On the CPU, from the strides: at (70, 67) the layouts of test_pack_motion
    select all eight instantiations, each with two blocks along x and, for the
    tile kernels, two tiles on each axis."""
    dimx, dimy = MULTI
    assert MULTI in SHAPES
    assert (-(-dimx // 64), -(-dimy // 64)) == (2, 2) and dimx % 64 and dimy % 64
    seen = set()
    for dtype in DTYPES:
        m = rand((3, dimx, dimy, 2), dtype, 4)
        for layout, named in LAYOUTS.items():
            t, axes, _ = build(layout, m)
            assert selection(t, axes) == named, (dtype, layout)
            seen.add((dtype.__name__,) + named)
    assert seen == {(d, p, v) for d in ("float32", "float64") for p in ("rows", "tile")
                    for v in (True, False)}


# ------------------------------------------------------------ the host form
@pytest.mark.parametrize("npairs", NPAIRS)
@pytest.mark.parametrize("dimx, dimy", SHAPES)
def test_planar_to_motion(gpu, dimx, dimy, npairs):
    from opticalflow2d_amd import prim
    planar = rand((npairs, 2, dimy, dimx), np.float64, 5)
    want = np.ascontiguousarray(planar.astype(np.float32).transpose(0, 2, 3, 1))
    assert not np.array_equal(want.transpose(0, 3, 1, 2).astype(np.float64), planar)
    got = prim.planar_to_motion(planar)
    assert np.array_equal(bits(got), bits(want))
    for k in range(npairs):  # and back through the kernel it mirrors
        assert np.array_equal(prim.motion_to_planar(got[k]),
                              planar[k].astype(np.float32).astype(np.float64))


# ------------------------------------------------------------ outside the pixels
def whole_allocation(fields):
    """The pitched fields holding ``fields`` ([n, dimy, dimx(, 2)] float32) in an
    allocation of the sentinel, as words: pixel (i, j) of pair k at element
    k * stride + P + j * P + i."""
    from opticalflow2d_amd import prim
    n, dimy, dimx = fields.shape[:3]
    tail = fields.shape[3:]
    stride, P = prim.pack_layout(dimx, dimy)
    assert P >= dimx and P % 128 == 0 and stride >= (dimy + 2) * P
    whole = np.full((n, stride) + tail, prim.PACK_SENTINEL, np.uint32)
    rows = whole[:, P:P + dimy * P].reshape((n, dimy, P) + tail)
    rows[:, :, :dimx] = bits(fields)
    return whole


@pytest.mark.parametrize("dimx, dimy", SHAPES)
def test_pack_leaves_slack_and_ghost_lines(gpu, dimx, dimy):
    from opticalflow2d_amd import prim
    n = 3
    # finite, and far from the inputs' normal deviates
    assert np.array([prim.PACK_SENTINEL], np.uint32).view(np.float32)[0] == np.float32(-6328.721)

    def check(got, raw, fields, what):
        assert np.array_equal(bits(got), bits(fields)), what
        want = whole_allocation(fields)
        assert raw.dtype == np.float32 and raw.shape == want.shape, what
        bad = np.argwhere(raw.view(np.uint32) != want)
        assert not len(bad), f"{what}: {len(bad)} words differ, first at {tuple(bad[0])}"

    img = rand((n, dimx, dimy), np.float64, 6)
    want = np.ascontiguousarray(img.astype(np.float32).transpose(0, 2, 1))
    for layout in ("contiguous", "xfast"):  # the tile and the rows kernel
        big = np.full(big_shape(layout, n, dimx, dimy), 7.0, np.float64)
        view(big, layout, dimx, dimy)[...] = img
        got, raw = prim.pack_image(view(cuda(big), layout, dimx, dimy), raw=True)
        check(got, raw, want, f"pack_image {layout}")
    for dtype, layouts in ((np.float32, ("xfast", "contiguous")),
                           (np.float64, ("planar_rows", "planar_tile"))):
        m = rand((n, dimx, dimy, 2), dtype, 7)
        for layout in layouts:
            t, axes, read = build(layout, m)
            if dimx > 1 and dimy > 1:
                assert selection(t, axes) == LAYOUTS[layout]
            got, raw = prim.pack_motion(t, axes, raw=True)
            check(got, raw, fields_of(read), f"pack_motion {layout}")
    planar = rand((n, 2, dimy, dimx), np.float64, 8)
    got, raw = prim.planar_to_motion(planar, raw=True)
    check(got, raw, np.ascontiguousarray(planar.astype(np.float32).transpose(0, 2, 3, 1)),
          "planar_to_motion")
