"""The quad kernel's end-of-band exchange (hs::jacobi4_kernel XCH,
hs_jacobi_impl.h; slab option "hs_quad_tail_exchange", default on): the two
waves of a pair hand each other their last u1, u2 and u3 rows through LDS
instead of recomputing them past the end of their bands.

Bar: with the option on, the motion equals the oracle's and that of the option
off on the float32 bits (NaN masks and signs of zero included), and every
iteration's Logger error equals the option-off run's bit for bit (rtol 0): both
runs are whole quads (4, 8, 12 iterations), so every iteration comes from the
same kernel, blocks and march order in both.

Geometry.  A wave marches hs3_rows(dimx, dimy) j-lines (of2d_device.h; the rule
is restated below, and the CPU test holds the restatement to the values the
header documents).  With two strips (dimx 130, 131) the rule gives 4 j-lines per wave until
the grid needs more than 1024 blocks, so the heights that give n = 5, 6, 7 and
36 are tens of thousands of j-lines: 2 * ceil(dimy / (4 n)) <= 1024 blocks at n
and more than 1024 at n - 1.  A block takes the exchange only when all four of
its waves have n >= 6 j-lines; the heights below put a partial second pair, an
idle wave, n = 5 and one-band grids beside the full blocks.
"""
import functools

import numpy as np
import pytest

from opticalflow2d_amd import SlabSolver
from test_gpu_hs_division_range import assert_bits

F = np.float32
ALPHA = 0.3
WAVES, OUT, CAP = 4, 120, 1024


def hs3_rows(dimx, nrows, cap=CAP):
    """of2d_device.h hs3_rows."""
    gx = (dimx + OUT - 1) // OUT
    best, best_t = 4, -1
    for r in range(4, 65):
        bands = (nrows + WAVES * r - 1) // (WAVES * r)
        rounds = (gx * bands + cap - 1) // cap
        t = rounds * (r + 2)
        if best_t < 0 or t < best_t:
            best_t, best = t, r
        if bands == 1:
            break
    return best


def last_band(dimx, dimy):
    """(n, j-lines of each wave of the last band)."""
    n = hs3_rows(dimx, dimy)
    left = dimy - (dimy - 1) // (WAVES * n) * (WAVES * n)
    return n, [max(0, min(n, left - w * n)) for w in range(WAVES)]


# dimy: (n, the last band's waves)
HEIGHTS = {
    12288: (6, [6, 6, 6, 6]),    # every block exchanges
    12279: (6, [6, 6, 3, 0]),    # last band: second pair partial, one wave idle
    12276: (6, [6, 6, 0, 0]),    # last band: second pair idle
    14336: (7, [7, 7, 7, 7]),
    14329: (7, [7, 7, 7, 0]),
    10240: (5, [5, 5, 5, 5]),    # n = 5: no block exchanges
    73728: (36, [36, 36, 36, 36]),
    8: (4, [4, 4, 0, 0]),        # one band; the first pair's boundary is interior,
    16: (4, [4, 4, 4, 4]),       # n = 4
    3: (4, [3, 0, 0, 0]),        # one wave, its end the image's edge
}


def test_heights_give_the_bands_they_claim():
    """CPU: hs3_rows as restated gives each height its n and last band, for
    both widths; the rule's documented values hold for the restatement."""
    assert hs3_rows(4096, 4096) == 36 and hs3_rows(16384, 16384) == 50
    for dimx in (130, 131):
        for dimy, want in HEIGHTS.items():
            assert last_band(dimx, dimy) == (want[0], want[1]), (dimx, dimy)


@functools.lru_cache(maxsize=None)
def pair(dims, special):
    """A smooth texture pair with seeded noise.  special: j-line of a pair's
    shared boundary (the first j-line of the second wave of band 0) around
    which, or 0 for none,
      * the moving image is constant over j-lines jb-3 .. jb+2, so the gradient
        rows jb-2 .. jb+1 are zero (gx and gy; jb-3 and jb+2 have gx = 0), which
        puts the rows that keep the division's fix-up into the exchanged steps;
      * It is NaN at one pixel of j-line jb-1 and 2^31 (sc out of the unscaled
        division's range) at one of j-line jb, in different strips, which puts
        the IEEE sequence there."""
    nx, ny = dims
    rng = np.random.default_rng(1000 * nx + ny + special)
    x = np.arange(nx, dtype=np.float64)[:, None]
    y = np.arange(ny, dtype=np.float64)[None, :]
    tex = lambda a, b: 0.5 + 0.1 * (np.sin(0.11 * a + 0.07 * b) + np.sin(0.05 * a - 0.13 * b + 1.0))
    ref = (tex(x, y) + 2.0 ** -8 * rng.random(dims)).astype(F)
    mov = (tex(x - 1.5, y + 0.75) + 2.0 ** -8 * rng.random(dims)).astype(F)
    if special:
        jb = special
        mov[:, jb - 3:jb + 3] = F(0.625)
        with np.errstate(all="ignore"):
            ref[60, jb - 1] = F(np.nan)       # It = mov - ref = NaN, strip 0
            ref[125, jb] = F(-2.0 ** 31)      # It = 2^31 + 0.625, strips 0 and 1
    return ref.astype(np.float64), mov.astype(np.float64)


def slab_run(dims, iters, ref, mov, exchange):
    s = SlabSolver(dims[0], dims[1], ALPHA)
    try:
        s.set_images(ref, mov)
        s.set_option("hs_gradients_from_image", 0)
        s.set_option("hs_quad_tail_exchange", exchange)
        info = s.info()
        assert info["iterations_per_launch"] == 4 and info["quad_tail_exchange"] == exchange
        assert s.run(iters, fixed_iters=True) == iters
        return s.motion(), s.errors()
    finally:
        s.close()


@functools.lru_cache(maxsize=None)
def oracle_motion(oracle, dims, iters, special):
    ref, mov = pair(dims, special)
    r = oracle.Registration(dims, [iters], 0, 0, [ALPHA], 1, 0, fixed_iters=True)
    try:
        r.register(ref, mov)
        return r.motion()
    finally:
        r.close()


def check(oracle, dims, iters, special):
    what = f"{dims[0]}x{dims[1]}, {iters} iterations, special {special}"
    ref, mov = pair(dims, special)
    m1, e1 = slab_run(dims, iters, ref, mov, 1)
    m0, e0 = slab_run(dims, iters, ref, mov, 0)
    for k in range(iters):
        print(f"{what}: iteration {k} error exchange {float(e1[k])!r} none {float(e0[k])!r}")
    assert len(e1) == iters == len(e0)
    assert_bits(m1, m0, f"{what}: motion, option 1 against 0")
    assert_bits(e1, e0, f"{what}: Logger errors, option 1 against 0")
    assert_bits(m1, oracle_motion(oracle, dims, iters, special), f"{what}: motion against the oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [4, 8, 12])
@pytest.mark.parametrize("dimx", [130, 131])
@pytest.mark.parametrize("dimy", [12288, 12279, 14329, 10240])
def test_exchange_bits(gpu, oracle, dimy, dimx, iters):
    """n = 6 full, n = 6 with a partial pair and an idle wave in the last band,
    n = 7 with an idle wave, n = 5 (no exchange); the zero gradient rows, the
    NaN and the out-of-range sc sit on the first pair's boundary."""
    n, _ = last_band(dimx, dimy)
    check(oracle, (dimx, dimy), iters, n)


@pytest.mark.gpu
@pytest.mark.parametrize("dimx,dimy,special", [(131, 12276, 0), (130, 14336, 0), (130, 14336, 7),
                                               (131, 12288, 18), (130, 8, 4), (131, 16, 0),
                                               (131, 16, 12), (130, 3, 0)])
def test_exchange_bits_more_bands(gpu, oracle, dimx, dimy, special):
    """An idle second pair, n = 7 full, the special rows on the second pair's
    boundary (3 n), one-band grids of 4-line waves and a single wave; 12
    iterations."""
    check(oracle, (dimx, dimy), 12, special)


@pytest.mark.gpu
def test_exchange_bits_bench_rows(gpu, oracle):
    """n = 36, the benchmark's j-lines per wave, every pair full."""
    check(oracle, (130, 73728), 8, 36)
