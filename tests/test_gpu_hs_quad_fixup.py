"""The quad kernel (hs::jacobi4_kernel, hs_jacobi_impl.h) leaves the division's
fix-up (v_div_fixup_f32) out of the row steps of a gradient row none of whose
lanes holds a gradient component +-0, and keeps it in all others; the argument
is in the comment above hs::recip_refined.  This file holds what that decision
can break: rows without any zero gradient (the path without the fix-up), a
single zero (+0 and -0) on an owned lane, on a halo lane and beside the padding of an odd
width, a whole row and a whole field of zeros, the zero row at every march
position of a wave marching down and of one marching up, and numerators at
both ends of the range the unscaled sequence is used in.

Bar: the motion equals, on the float32 bits (signs of zero included, equal NaN
masks), the oracle's and that of the same run with hs_fixed_quads = 0.  The
Logger errors equal bit for bit (rtol 0) those of a hs_fixed_quads = 0 run made
of whole triples, for the iterations both produce (test_gpu_hs_quad_pairs.py's
rule).

The slab takes images, not fields (SlabSolver.set_images; the motion starts at
0), so the inputs are images whose float32 differences are the wanted fields:
gx(x, j) = (mov[x+1, j] - mov[x-1, j]) / 2 is +0 where the two neighbours are
equal, gy likewise along j, and It = mov - ref.  Two things follow.  A gradient
of -0 takes a -0 pixel after the pixel and a +0 before it, (-0 - +0) / 2 = -0,
and the -0 pixel has to survive the slab's warp of the moving image by the
zero motion (pixel * 1 + three taps * 0), which it does while its right, lower
and diagonal neighbours are negative: `minus_zero_px`, `warp_zero` and the CPU
assertion on the bits 0x80000000 of the warped image's gradients.  It is the
one input on which fin()'s zero word depends on the |.| operands of its
minimum, and beside It > 0 it gives the numerator a = g * sc = -0; g = +0
beside sc < 0 gives the same.  And the stencil mean q of a pixel is -0 only if its four neighbours
sum to -0 or to a value that rounds to it: `minus_zero_case` holds the vertical
neighbours of one pixel at u.x = -2^-149 in every iteration (It = 2^-147, gx =
0.25, alpha = 1: their row steps take the IEEE sequence) and everything else
around it at 0, so that q.x = -2^-149 / 4 = -0 there in iterations 2, 3 and 4
while It = -1 < 0 and gx = +0 make a.x = -0: IEEE gives -0 - -0 = +0, the
sequence without the fix-up -0 - +0 = -0.  For the horizontal neighbours to
stay 0 the pixels within 8 columns of it carry a zero gradient too (a pixel
with a gradient and It != 0 moves in the first iteration and reaches its
neighbours one pixel per iteration); every other pixel of that j-line has
gradients, so the j-lines before and after it take the path without the fix-up
and this one must not.  The CPU part asserts on the oracle's iterate that the
case is what it claims.

What this file cannot do: a build of the kernel with the fix-up left out of
every row step, zero rows included, passes it as well (measured, all 45 GPU
cases).  The only thing that build gets wrong is the sign of a zero of the
iterate, and that sign does not reach anything the slab returns: the motion is
the iterate composed onto the zero motion (0 + u, which is +0 for u = -0), a
zero adds nothing to a Logger norm, and in the next iteration a -0 neighbour
changes a stencil sum only where the other three are -0 too.  So the file
holds the results to the oracle's bits on inputs that take each of the three
division paths, but the row flag itself rests on the argument in the kernel's
comment, not on a test that fails without it.

Geometry (of2d_device.h): strip b covers x in [120 b - 4, 120 b + 124), lane l
holds x = 120 b - 4 + 2 l and the column after it; lanes 2..61 own their
pixels.  A wave marches 4 j-lines on these grids, odd waves upward.  A strip
that reaches into the pitch padding (It = 0 there) takes the IEEE sequence in
every row step, so the fast paths run in the strips that lie inside the image:
strip 0 from width 124 on, strip 1 from 244 on.
"""
import functools

import numpy as np
import pytest

from opticalflow2d_amd import SlabSolver
from test_gpu_hs_division_range import assert_bits, bits, derivatives, precheck_flag

F = np.float32
ALPHA = 0.3
NY = 12


def slab_run(dims, iters, ref, mov, quads, alpha):
    s = SlabSolver(dims[0], dims[1], alpha)
    try:
        s.set_images(ref, mov)
        s.set_option("hs_gradients_from_image", 0)
        s.set_option("hs_fixed_quads", quads)
        assert s.info()["iterations_per_launch"] == (4 if quads else 3)
        assert s.run(iters, fixed_iters=True) == iters
        return s.motion(), s.errors()
    finally:
        s.close()


def oracle_motion(oracle, dims, iters, ref, mov, alpha):
    r = oracle.Registration(dims, [iters], 0, 0, [alpha], 1, 0, fixed_iters=True)
    try:
        r.register(ref, mov)
        return r.motion()
    finally:
        r.close()


def check(oracle, ref, mov, what, iters=8, alpha=ALPHA):
    dims = ref.shape
    m, e = slab_run(dims, iters, ref, mov, 1, alpha)
    assert_bits(m, oracle_motion(oracle, dims, iters, ref, mov, alpha), f"{what}: motion, oracle")
    whole = 3 * ((iters + 2) // 3)
    mt, et = slab_run(dims, whole, ref, mov, 0, alpha)
    if whole == iters:
        assert_bits(m, mt, f"{what}: motion, triples")
    else:
        mt, _ = slab_run(dims, iters, ref, mov, 0, alpha)
        assert_bits(m, mt, f"{what}: motion, hs_fixed_quads 0")
    assert len(e) == iters
    for k in range(iters):
        print(f"{what}: iteration {k} error quads {float(e[k])!r} triples {float(et[k])!r}")
    assert_bits(e, et[:iters], f"{what}: Logger errors")


# ------------------------------------------------------------------ inputs
def noise(dims, seed):
    """Seeded noise in [1, 2) (mov) and It = mov - ref in [0.5, 1.5): every
    gradient component and every It non-zero and in range."""
    rng = np.random.default_rng(seed)
    mov = (1.0 + rng.random(dims)).astype(F)
    it = (0.5 + rng.random(dims)).astype(F)
    return mov, it


def finish(mov, it):
    """(ref, mov) as float64 arrays of float32 values with mov - ref ~ it."""
    mov = np.ascontiguousarray(mov, F)
    ref = (mov - np.asarray(it, F)).astype(F)
    return ref.astype(np.float64), mov.astype(np.float64)


def zero_gx(mov, x, j):
    mov[x + 1, j] = mov[x - 1, j]


def zero_gy(mov, x, j):
    mov[x, j + 1] = mov[x, j - 1]


def zeros_of(oracle, ref, mov):
    gx, gy, It = derivatives(oracle, ref, mov)
    return (gx == 0) | (gy == 0), gx, gy, It


# ------------------------------------------------- (a) no zero gradient
@functools.lru_cache(maxsize=None)
def plain_case(dimx):
    return finish(*noise((dimx, NY), 100 + dimx))


def test_plain_cases_hold_no_zero(oracle):
    for dimx in (120, 121, 250):
        ref, mov = plain_case(dimx)
        z, gx, gy, It = zeros_of(oracle, ref, mov)
        assert not z.any() and (np.abs(It) >= 0.25).all()
        assert precheck_flag(gx, gy, ALPHA) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dimx", [120, 121, 250])
def test_no_zero_gradient(gpu, oracle, dimx):
    """The issue's widths.  Only 250 reaches the path without the fix-up, in
    strips 0 and 1 (x in [-4, 124) and [116, 244), inside the image); its
    strip 2, and the single strip of 120 and both strips of 121, reach into
    the pitch padding, where It = 0 sends every row step to the IEEE sequence.
    Those widths hold the odd last column and the padding-side lanes to the
    oracle; they do not run either fast path."""
    ref, mov = plain_case(dimx)
    check(oracle, ref, mov, f"no zero, width {dimx}")


# ---------------------------------- (b) one zero, generic q; and q = -0 / +0
WHICH = ["gx", "gy", "both"]
PX = (60, 5)  # lane 32 of strip 0, the second j-line of wave 1 (marching up)


def warp_zero(mov):
    """Image::warp2d by the zero motion as the slab applies it to the moving
    image before it takes the gradients (warp_zero_rows_kernel, and the
    reference's Image.cpp:119-182 with fx = fy = 0), in float32: the pixel
    times 1 plus its right, lower and diagonal taps times 0."""
    m = np.asarray(mov, F)
    out = (m * F(1)) * F(1)
    out[:-1, :] = out[:-1, :] + (m[1:, :] * F(0)) * F(1)
    out[:, :-1] = out[:, :-1] + (m[:, 1:] * F(1)) * F(0)
    out[:-1, :-1] = out[:-1, :-1] + (m[1:, 1:] * F(0)) * F(0)
    return out


def minus_zero_px(mov, x, j):
    """Pixel (x, j) = -0 in a way that survives warp_zero: -0 * 1 + tap * 0
    is -0 only while every tap is negative (or -0), so its right, lower and
    diagonal neighbours are made negative."""
    mov[x, j] = -0.0
    for dx, dj in ((1, 0), (0, 1), (1, 1)):
        if bits(mov[x + dx, j + dj]) != 0x80000000:
            mov[x + dx, j + dj] = -abs(mov[x + dx, j + dj])


@functools.lru_cache(maxsize=None)
def one_zero_case(which, sign, dimx=250, px=PX, gzero="+0"):
    """One pixel with gx, gy or both +0 (two equal neighbours) or -0 (the
    neighbour after it -0, the one before it +0: (-0 - +0) / 2 = -0); It there
    positive or negative, so the numerator g * sc is a zero of either sign
    either way."""
    mov, it = noise((dimx, NY), 7)
    x, j = px
    if gzero == "+0":
        if which in ("gx", "both"):
            zero_gx(mov, x, j)
        if which in ("gy", "both"):
            zero_gy(mov, x, j)
    else:
        if which in ("gx", "both"):
            mov[x - 1, j] = 0.0
            minus_zero_px(mov, x + 1, j)
        if which in ("gy", "both"):
            mov[x, j - 1] = 0.0
            minus_zero_px(mov, x, j + 1)
    it[x, j] = F(sign) * it[x, j]
    return finish(mov, it)


def test_one_zero_cases(oracle):
    """CPU: one zero component of the claimed sign, on the gradients of the
    moving image as the slab holds it, that is after the warp by the zero
    motion (which must keep the -0 pixels the -0 gradients are made of)."""
    for gzero, want in (("+0", 0), ("-0", 0x80000000)):
        for which in WHICH:
            for sign in (1, -1):
                ref, mov = one_zero_case(which, sign, gzero=gzero)
                warped = warp_zero(mov)
                if gzero == "-0":
                    assert (bits(warped) == 0x80000000).sum() == (2 if which == "both" else 1)
                    assert np.array_equal(warped, mov.astype(F))
                else:
                    assert np.array_equal(bits(warped), bits(mov.astype(F)))
                z, gx, gy, It = zeros_of(oracle, ref, warped.astype(np.float64))
                assert z.sum() == 1 and z[PX] and np.sign(It[PX]) == sign
                assert (gx[PX] == 0) == (which != "gy") and (gy[PX] == 0) == (which != "gx")
                if which != "gy":
                    assert bits(gx[PX]) == want
                if which != "gx":
                    assert bits(gy[PX]) == want
                assert precheck_flag(gx, gy, ALPHA) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1, -1], ids=["It+", "It-"])
@pytest.mark.parametrize("gzero", ["+0", "-0"], ids=["g+0", "g-0"])
@pytest.mark.parametrize("which", WHICH)
def test_one_zero_gradient(gpu, oracle, which, gzero, sign):
    """PX lies in strip 0 of a 250-wide grid, which is inside the image: the
    row steps of j-line 5 take the unscaled sequence with the fix-up, those of
    the other j-lines without it.  A -0 component is the one input on which
    the row's word depends on the |.| operands of fin()'s minimum."""
    ref, mov = one_zero_case(which, sign, gzero=gzero)
    check(oracle, ref, mov, f"one zero {which} = {gzero}, It sign {sign}")


MZ_DIMS = (250, NY)
MZ_HALF = 8  # zero gradients on the columns within 8 of PX


@functools.lru_cache(maxsize=None)
def minus_zero_case(feed):
    """The module docstring's construction around PX; feed = False leaves the
    vertical neighbours at 0, so that q = +0 there."""
    x, j = PX
    mov, it = noise(MZ_DIMS, 11)
    it[:, :] = 0                      # no pixel moves ...
    it[:, j] = -(0.5 + it[:, j])      # ... but those of j-line j; here -0.5
    # j-lines j-1, j, j+1 flat within MZ_HALF + 1 columns of x: gx = gy = +0 on j
    mov[x - MZ_HALF - 1:x + MZ_HALF + 2, j - 1:j + 2] = 1.0
    for dj in (-1, 1):                # the vertical neighbours: gx = 0.25, gy = 0
        mov[x - 1, j + dj], mov[x, j + dj], mov[x + 1, j + dj] = 0.0, 0.0, 0.5
        mov[x, j + 2 * dj] = 1.0
        if feed:
            it[x, j + dj] = F(2.0 ** -147)
    return finish(mov, it)


def test_minus_zero_case_is_what_it_claims(oracle):
    """CPU, the oracle alone: the fields, q.x = -0 at PX in iterations 2..4, the
    result +0 there, and the j-lines around it free of zero gradients."""
    x, j = PX
    for feed in (True, False):
        ref, mov = minus_zero_case(feed)
        z, gx, gy, It = zeros_of(oracle, ref, mov)
        assert precheck_flag(gx, gy, 1.0) == 0
        assert z[x - MZ_HALF:x + MZ_HALF + 1, j].all() and gx[x, j] == 0 and gy[x, j] == 0
        assert bits(gx[x, j]) == 0 and bits(gy[x, j]) == 0        # +0
        assert not z[:116, j].all() and not z[:, j - 2].any() and not z[:, j + 2].any()
        assert not z[x + MZ_HALF + 2:244, j].any() and not z[:x - MZ_HALF - 1, j].any()
        assert (It[:, j] < -0.25).all()
        for dj in (-1, 1):
            assert gx[x, j + dj] == 0.25 and gy[x, j + dj] == 0
            assert It[x, j + dj] == (F(2.0 ** -147) if feed else 0)
        nx, ny = MZ_DIMS
        dI = np.ascontiguousarray(np.stack([gx.T, gy.T], axis=2).reshape(-1))
        Itf = np.ascontiguousarray(It.T.reshape(-1))
        for iters in (1, 2, 3, 4):
            u = np.zeros(2 * nx * ny, F)
            errs = np.zeros(iters, F)
            assert oracle.lib().oracle_hs_loop(u, dI, Itf, nx, ny, 1.0, iters, 1, errs) == iters
            u = u.reshape(ny, nx, 2).transpose(1, 0, 2)
            want = -F(2.0 ** -149) if feed else F(0)
            assert u[x, j - 1, 0] == want and u[x, j + 1, 0] == want
            assert not u[x - 1, j].any() and not u[x + 1, j].any()
            assert bits(u[x, j, 0]) == 0 and bits(u[x, j, 1]) == 0  # +0, not -0
        # the mean of the four neighbours at PX: -2^-148 / 4 rounds to -0
        with np.errstate(under="ignore"):
            q = (((u[x - 1, j, 0] + u[x + 1, j, 0]) + u[x, j - 1, 0]) + u[x, j + 1, 0]) / F(4)
        assert bits(q) == (0x80000000 if feed else 0)
        # and -0 - +0, what the sequence without its fix-up would leave, is -0
        assert bits(F(q) - F(0.0)) == (0x80000000 if feed else 0)
        m = oracle_motion(oracle, MZ_DIMS, 4, ref, mov, 1.0)
        assert bits(m[x, j, 0]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("feed", [True, False], ids=["q-0", "q+0"])
def test_minus_zero_numerator(gpu, oracle, feed):
    ref, mov = minus_zero_case(feed)
    check(oracle, ref, mov, f"a = -0 beside q = {'-0' if feed else '+0'}", iters=4, alpha=1.0)
    check(oracle, ref, mov, f"a = -0 beside q = {'-0' if feed else '+0'}", iters=8, alpha=1.0)


# --------------------------------- (c) the zero on a halo lane, odd widths
# x = 117: lane 0 of strip 1 (px 1), lane 60 of strip 0; x = 243: lane 63 of
# strip 1 (px 1), lane 3 of strip 2; x = 1: lane 2 of strip 0 and, clamped,
# the halo lanes 0-1 left of the image; 248: the last but one column of 250
HALO = [(250, 117), (250, 243), (250, 1), (250, 248), (251, 117), (251, 249), (121, 117),
        (121, 119)]


@functools.lru_cache(maxsize=None)
def halo_case(dimx, x):
    return one_zero_case("both", -1, dimx, (x, 6))


def test_halo_cases(oracle):
    for dimx, x in HALO:
        z, gx, gy, It = zeros_of(oracle, *halo_case(dimx, x))
        assert z.sum() == 1 and z[x, 6] and It[x, 6] < 0


@pytest.mark.gpu
@pytest.mark.parametrize("dimx,x", HALO)
def test_zero_on_halo_lane_and_odd_width(gpu, oracle, dimx, x):
    """Which strips reach the fast paths here: of widths 250 and 251, strips 0
    and 1 (inside the image).  x = 117 is owned by strip 0 and a halo lane of
    strip 1, so both waves must keep the fix-up on that j-line and both are
    on the unscaled sequence; x = 1 is owned by strip 0, whose clamped halo
    lanes left of the image read columns 0 and 1 again.  x = 243 is a halo
    lane of strip 1 (fast path, must fall back) and owned by strip 2; x = 248
    and 249 lie in strip 2 only.  Strip 2 and every strip of width 121 reach
    into the pitch padding (It = 0) and take the IEEE sequence in every row
    step: those cases hold the padding-side lanes and the odd last column to
    the oracle, not the fall-back."""
    check(oracle, *halo_case(dimx, x), f"zero at x {x} of {dimx}")


# ----------------------------------------- (d) a zero j-line, a zero field
@functools.lru_cache(maxsize=None)
def flat_case(kind):
    mov, it = noise((250, NY), 13)
    it[::3] = -it[::3]
    if kind == "line":
        mov[:, 4:7] = 1.5   # j-lines 4..6 equal and flat: gx = gy = 0 on j-line 5
    else:
        mov[:, :] = 1.5
    return finish(mov, it)


def test_flat_cases(oracle):
    z, _, _, _ = zeros_of(oracle, *flat_case("line"))
    assert z[:, 5].all() and not z[:, :3].any() and not z[:, 8:].any()
    z, gx, gy, It = zeros_of(oracle, *flat_case("field"))
    assert not gx.any() and not gy.any() and (It != 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["line", "field"])
def test_flat_image(gpu, oracle, kind):
    check(oracle, *flat_case(kind), f"flat {kind}")


# ------------------------------------ (e) the zero row at each march position
E_NY = 16  # four waves: j-lines 0-3 down, 7-4 up, 8-11 down, 15-12 up


@functools.lru_cache(maxsize=None)
def row_case(j):
    """gx = 0 on every pixel of j-line j (columns pairwise equal there), It of
    both signs."""
    mov, it = noise((250, E_NY), 17)
    it[1::2] = -it[1::2]
    mov[0::2, j], mov[1::2, j] = 1.25, 1.75
    return finish(mov, it)


def test_row_cases(oracle):
    for j in range(E_NY):
        z, gx, gy, It = zeros_of(oracle, *row_case(j))
        assert (gx[1:-1, j] == 0).all() and z[1:-1, j].all()
        assert not np.delete(z, j, axis=1).any()
        assert precheck_flag(gx, gy, ALPHA) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(E_NY))
def test_zero_row_at_each_march_position(gpu, oracle, j):
    """For the wave marching j-lines 8..11 downward the j-lines 5, 6, 7 are the
    prologue's halo rows (gm3, gm2, gm1), 8, 9, 10 its first three rows and 11
    its last; for the wave marching 7..4 upward these are 10, 9, 8, then 7, 6,
    5, and 4.  Every j-line takes every role of its own wave and of the waves
    beside it."""
    check(oracle, *row_case(j), f"zero row {j}")


# ------------------------------------------- (f) a at the range's corners
LO_G, HI_G = F(2.0 ** -30), np.nextafter(F(2.0 ** 20), F(0))
LO_SC, HI_SC = F(2.0 ** -50), np.nextafter(F(2.0 ** 30), F(0))
QX = (60, 5)


@functools.lru_cache(maxsize=None)
def corner_case(end):
    """gx = 2^-30 beside It = 2^-50 (the smallest numerator, 2^-80), or gx =
    2^20 - ulp beside It = 2^30 - ulp (the largest), on one pixel of the noise
    pair; no gradient is 0.  sc = It in the first iteration."""
    mov, it = noise((250, NY), 19)
    x, j = QX
    if end == "low":
        mov[x - 1, j], mov[x + 1, j] = 0.0, F(2) * LO_G
        mov[x, j] = 0.0                                  # so that ref = -It is exact
        it[x, j] = LO_SC
    else:
        mov[x - 1, j], mov[x + 1, j] = 0.0, F(2) * HI_G
        mov[x, j] = 0.0
        it[x, j] = HI_SC
    return finish(mov, it)


def test_corner_cases(oracle):
    for end in ("low", "high"):
        z, gx, gy, It = zeros_of(oracle, *corner_case(end))
        assert not z.any() and precheck_flag(gx, gy, ALPHA) == 0
        if end == "low":
            assert gx[QX] == LO_G and It[QX] == LO_SC
        else:
            assert gx[QX] == HI_G and It[QX] == HI_SC
            assert float(gx[QX]) * float(It[QX]) < 2.0 ** 50


@pytest.mark.gpu
@pytest.mark.parametrize("end", ["low", "high"])
def test_numerator_at_the_corners(gpu, oracle, end):
    check(oracle, *corner_case(end), f"corner {end}", iters=4)
    check(oracle, *corner_case(end), f"corner {end}", iters=8)
