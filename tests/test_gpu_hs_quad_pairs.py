"""What a change of how the quad kernel (hs::jacobi4_kernel, hs_jacobi_impl.h)
pairs the two pixels of a lane can break.  The kernel takes its division-range
decision on the bits of both pixels' sc and selects px 1 out of the Logger
norms only in the strip that ends an odd dimx; a variant that holds every row
by component, X = (x of px 0, x of px 1), Y = (y of px 0, y of px 1), was
written against this file (tools/ab_quad_pairs.patch).
tests/test_gpu_hs_quad.py, test_gpu_hs_division_range.py and test_gpu_hs.py
hold the quad's motion to the oracle on their grids; this file adds inputs on
which an exchanged component or pixel, a range decision taken on the wrong
pixel of a lane, the odd last column's select and the un-unrolled tail of a
short band would show.

Bar: the motion equals the oracle's on the float32 bits (equal NaN masks where
the oracle holds NaN, signs of zero included).  The Logger errors equal, bit for
bit (rtol 0), those of a hs_fixed_quads = 0 run: a quad takes the triple's
strips, bands and march directions and adds each lane's magnitudes in the same
order, px 0 before px 1.  That holds for iterations which a quad or a triple
produces in both runs, so the triples run is made of whole triples: it runs
3 * ceil(n / 3) iterations, of which the first n are compared (the iterate's
history is the same, and a fixed 4-iteration triples run would produce its
fourth iteration with the single-step kernel, which has other blocks and sums in
fp64 per pixel).

The pitch padding of a slab's device arrays cannot be reached from Python
(SlabSolver takes and returns image rows only, and the primitives of prims.py
work on dense arrays of their own), so the padding is not poisoned here; the
odd widths are compared as they are.

Geometry (of2d_device.h): a wave's row step covers 128 px of strip b, x in
[120 b - 4, 120 b + 124), lane l holding x = 120 b - 4 + 2 l (px 0, an even
column) and the odd column after it (px 1).
"""
import functools

import numpy as np
import pytest

from opticalflow2d_amd import SlabSolver
from opticalflow2d_amd import synthetic as S
from test_gpu_hs_division_range import assert_bits, bits, derivatives, precheck_flag

F = np.float32
ALPHA = 0.3
LO_SC, HI_SC = F(2.0 ** -50), F(2.0 ** 30)


def slab_run(dims, iters, ref, mov, quads, alpha=ALPHA):
    s = SlabSolver(dims[0], dims[1], alpha)
    try:
        s.set_images(ref, mov)
        s.set_option("hs_gradients_from_image", 0)
        s.set_option("hs_fixed_quads", quads)
        per_launch = s.info()["iterations_per_launch"]
        assert per_launch == (4 if quads else 3)
        assert s.run(iters, fixed_iters=True) == iters
        return s.motion(), s.errors()
    finally:
        s.close()


def oracle_motion(oracle, dims, iters, ref, mov, alpha=ALPHA):
    r = oracle.Registration(dims, [iters], 0, 0, [alpha], 1, 0, fixed_iters=True)
    try:
        r.register(ref, mov)
        return r.motion()
    finally:
        r.close()


def check(oracle, dims, iters, ref, mov, what):
    """Quads against the oracle (motion) and against whole triples (errors)."""
    m, e = slab_run(dims, iters, ref, mov, 1)
    assert_bits(m, oracle_motion(oracle, dims, iters, ref, mov), f"{what}: motion")
    _, et = slab_run(dims, 3 * ((iters + 2) // 3), ref, mov, 0)
    assert len(e) == iters
    for k in range(iters):
        print(f"{what}: iteration {k} error quads {float(e[k])!r} triples {float(et[k])!r}")
    assert_bits(e, et[:iters], f"{what}: Logger errors")


# ------------------------------------------------- components and pixels
@functools.lru_cache(maxsize=None)
def skewed_pair(dims):
    """A steep ramp in x times a shallow one in y, odd columns 2^-7 of the even
    ones, plus seeded noise: gx is hundreds of times gy, and the two pixels of
    a lane differ by orders of magnitude in value, gradient and It."""
    nx, ny = dims
    rng = np.random.default_rng(7 * nx + ny)
    x = np.arange(nx, dtype=np.float64)[:, None]
    y = np.arange(ny, dtype=np.float64)[None, :]
    col = np.where(np.arange(nx) % 2, 2.0 ** -7, 1.0)[:, None]
    ref = (40.0 * (x + 1.0)) * (1.0 + 2.0 ** -13 * y) * col + 2.0 ** -6 * rng.random(dims)
    mov = ref * 0.75 + col * (3.0 + 2.0 ** -6 * rng.random(dims))
    return ref, mov


def test_skewed_pair_is_skewed(oracle):
    """CPU: the input separates components and pixels as its docstring says."""
    for dims in ((121, 37), (6, 9)):
        gx, gy, It = derivatives(oracle, *skewed_pair(dims))
        assert np.median(np.abs(gx)) > 100 * np.median(np.abs(gy)) > 0
        ev, od = np.abs(It[0::2]).mean(), np.abs(It[1::2]).mean()
        assert ev > 50 * od > 0
        assert precheck_flag(gx, gy, ALPHA) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [4, 12])
@pytest.mark.parametrize("dims", [(121, 37), (6, 9)], ids=lambda d: f"{d[0]}x{d[1]}")
def test_components_and_pixels_not_exchanged(gpu, oracle, dims, iters):
    ref, mov = skewed_pair(dims)
    check(oracle, dims, iters, ref, mov, f"skewed {dims[0]}x{dims[1]}, {iters} iterations")


# ------------------------------------------------------- odd last column
@pytest.mark.gpu
@pytest.mark.parametrize("iters", [4, 12])
@pytest.mark.parametrize("dimx", [5, 121, 241])
def test_odd_last_column(gpu, oracle, dimx, iters):
    """The lane holding column dimx - 1 has its px 1 in the padding: one lane
    of strip 0 (5), the only owned lane of strip 1 (121), of strip 2 (241)."""
    dims = (dimx, 9)
    ref, mov = skewed_pair(dims)
    check(oracle, dims, iters, ref, mov, f"odd width {dimx}x9, {iters} iterations")


# ------------------------------------------------------------ band tails
@pytest.mark.gpu
@pytest.mark.parametrize("iters", [4, 12])
@pytest.mark.parametrize("dimy", [1, 2, 3, 5, 6])
def test_band_tails(gpu, oracle, dimy, iters):
    """Waves with fewer than four j-lines: the un-unrolled tail loop and every
    `sp + k < n` guard.  A wave marches 4 j-lines on these grids (hs3_rows), so
    3 j-lines give a wave n = 3, 5 give 4 and 1, 6 give 4 and 2.  A slab of
    fewer than 3 j-lines does not exist (slab.cpp: "grid too small"; the
    reference's one-sided differences need a neighbour, and with one j-line
    partial_y reads past the image): 1 and 2 are held to that refusal."""
    dims = (8, dimy)
    ref, mov = skewed_pair(dims)
    if dimy < 3:
        from opticalflow2d_amd._lib import InvalidArgument
        with pytest.raises(InvalidArgument):
            slab_run(dims, iters, ref, mov, 1)
        return
    check(oracle, dims, iters, ref, mov, f"8x{dimy}, {iters} iterations")


# ------------------------------------- range decision, one pixel of a lane
RDIMS = (130, 12)
SUB = F(2.0 ** -130)  # a float32 denormal
VALUES = {"lo": LO_SC, "lo-ulp": np.nextafter(LO_SC, F(0)), "hi-ulp": np.nextafter(HI_SC, F(0)),
          "hi": HI_SC, "zero": F(0), "denormal": SUB, "inf": F(np.inf), "nan": F(np.nan)}
IN_RANGE = {"lo", "hi-ulp"}
# (x of px 0 of the lane, j-line): lane 32 of strip 0; lane 63 of strip 0, which
# is lane 3 of strip 1 (x = 122, 123 lie in both strips' row steps)
PLACES = [(60, 3), (122, 8)]


@functools.lru_cache(maxsize=None)
def range_case(name, side):
    """The textured pair with It = VALUES[name] on the even (side 0) or the odd
    (side 1) column of a lane at both PLACES, every other It in range.  It is
    Imov - Iref in float32: with Imov = 0 there and Iref = -v it is v."""
    r, m = S.texture_pair(RDIMS[0], seed=33, ny=RDIMS[1])
    ref, mov = r.astype(F), m.astype(F)
    ref[ref == mov] += F(2.0 ** -10)
    with np.errstate(all="ignore"):
        for x0, j in PLACES:
            mov[x0 + side, j] = 0
            ref[x0 + side, j] = -VALUES[name]
    return ref.astype(np.float64), mov.astype(np.float64)


def range_key_ok(v):
    """The kernel's decision on the bits of v: the sign shifted out, the biased
    exponent 77 <= e < 157 as one unsigned compare."""
    b = np.asarray(v, F).view(np.uint32).astype(np.uint64)
    return (((b << np.uint64(1)) - np.uint64(77 << 24)) & np.uint64(0xFFFFFFFF)) < np.uint64(80 << 24)


def test_range_placements_are_what_they_claim(oracle):
    """CPU, the oracle alone: each placement produces the sc it claims at the
    first iteration (q = 0, so sc = It), on that pixel only; the decision on the
    bits equals 2^-50 <= |sc| < 2^30 for every value; and on each side the
    in-range values leave strip 0's row step on the unscaled sequence while the
    others send it to the IEEE sequence."""
    edge = np.array([2.0 ** -50, 2.0 ** 30, 0.0, 2.0 ** -130, np.inf, np.nan, 1.0, -1.0, 2.0 ** -126,
                     -2.0 ** -50, -2.0 ** 30, 3.4e38], F)
    edge = np.concatenate([edge, np.nextafter(edge, F(0)), np.nextafter(edge, F(np.inf))])
    with np.errstate(invalid="ignore"):
        expect = (np.abs(edge) >= LO_SC) & (np.abs(edge) < HI_SC)
    assert np.array_equal(range_key_ok(edge), expect)
    paths = {0: set(), 1: set()}
    for side in (0, 1):
        for name, v in VALUES.items():
            gx, gy, It = derivatives(oracle, *range_case(name, side))
            assert precheck_flag(gx, gy, ALPHA) == 0, (name, side)
            ok = range_key_ok(It)
            for x0, j in PLACES:
                got = It[x0 + side, j]
                assert (np.isnan(got) and np.isnan(v)) or got.view(np.uint32) == v.view(np.uint32)
                ok[x0 + side, j] = True
            assert ok.all(), (name, side)  # every other pixel is in range
            step = range_key_ok(It)[0:124].all(axis=0)  # strip 0's row steps
            assert step[[j for _, j in PLACES]].all() == (name in IN_RANGE)
            assert step.sum() == (RDIMS[1] if name in IN_RANGE else RDIMS[1] - len(PLACES))
            paths[side].add("unscaled" if step[PLACES[0][1]] else "ieee")
    assert paths == {0: {"unscaled", "ieee"}, 1: {"unscaled", "ieee"}}
    assert float(VALUES["lo-ulp"]) == 2.0 ** -50 - 2.0 ** -74
    assert float(VALUES["hi-ulp"]) == 2.0 ** 30 - 64 and 0 < float(SUB) < 2.0 ** -126


@pytest.mark.gpu
@pytest.mark.parametrize("side", [0, 1], ids=["even", "odd"])
@pytest.mark.parametrize("name", list(VALUES))
def test_range_decision_one_pixel_of_a_lane(gpu, oracle, name, side):
    ref, mov = range_case(name, side)
    m, _ = slab_run(RDIMS, 4, ref, mov, 1)
    want = oracle_motion(oracle, RDIMS, 4, ref, mov)
    assert want.any()
    assert_bits(m, want, f"sc {name} on the {'odd' if side else 'even'} column")
