"""The four-iterations-per-launch Horn-Schunck kernel (hs::jacobi4_kernel,
hs_jacobi_impl.h) that a one-rank slab's fixed-iteration run launches
(slab.cpp, option "hs_fixed_quads", default on), against the oracle.

Bar: the motion bit for bit (the quad applies the triple's row step four
times), whatever the mix of quads with the triple, pair or single step of a
run's tail.  The Logger errors are compared with the triple-only path (option
off).  A quad takes the same strips, bands and march directions as a triple
and adds in the same order, so an iteration that a quad or a triple produces
in both runs must give the same error bit for bit (and so must one that the
same single-step or pair kernel produces in both): those are asserted at rtol
0.  Only where the two schedules cut a run's tail into different kernels
(8 iterations: two quads, or two triples and a pair, whose kernel has other
blocks) may the fp64 sums differ in rounding; there the tolerance is the one
the fixed-iteration HS errors are held to elsewhere (tests/test_gpu_ranks.py:
1e-5 relative).

Grids (dimx x dimy), each for one way the kernel can go wrong:
  8 x 5, 5 x 3           fewer rows than the 8-line halo: every ghost clamp
  119 x 40, 120 x 37,    the strip boundary (120 output columns), its odd last
  121 x 37               column, a second strip of one column; a band boundary
  257 x 151              three strips, a ragged last one, several bands, both
                         march directions
  4096 x 8               the workload's width and pitch, one short band
Iterations 4, 8, 9, 10, 11, 13: quads only, quad + single, + pair, + triple,
and mixed.
"""
import functools

import numpy as np
import pytest

from opticalflow2d_amd import SlabSolver
from opticalflow2d_amd import synthetic as S

pytestmark = pytest.mark.gpu

ALPHA = 0.3
GRIDS = [(8, 5), (5, 3), (119, 40), (120, 37), (121, 37), (257, 151), (4096, 8)]
ITERS = [4, 8, 9, 10, 11, 13]
ERR_RTOL = 1e-5  # tests/test_gpu_ranks.py, fixed-iteration HS errors


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def pair(dims):
    nx, ny = dims
    rng = np.random.default_rng(nx * 1000 + ny)
    ref = rng.random((nx, ny))
    mov = np.roll(ref, 1, axis=0) * 0.9 + 0.05
    return ref, mov


def oracle_motion(oracle, dims, iters, ref, mov):
    r = oracle.Registration(dims, [iters], 0, 0, [ALPHA], 1, 0, fixed_iters=True)
    r.register(ref, mov)
    m = r.motion()
    r.close()
    return m


_ORACLE = {}


def want(oracle, dims, iters):
    """The oracle's motion of the seeded pair, computed once per case."""
    key = (dims, iters)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_motion(oracle, dims, iters, *pair(dims))
        _ORACLE[key].setflags(write=False)
    return _ORACLE[key]


def slab_run(dims, iters, ref, mov, quads=1, gi=0):
    s = SlabSolver(dims[0], dims[1], ALPHA)
    try:
        s.set_images(ref, mov)
        s.set_option("hs_gradients_from_image", gi)
        s.set_option("hs_fixed_quads", quads)
        per_launch = s.info()["iterations_per_launch"]
        assert s.run(iters, fixed_iters=True) == iters
        return s.motion(), s.errors(), per_launch
    finally:
        s.close()


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: f"{d[0]}x{d[1]}")
def test_quad_motion_bitwise(gpu, oracle, dims, iters):
    ref, mov = pair(dims)
    m, errs, per_launch = slab_run(dims, iters, ref, mov)
    assert per_launch == 4
    assert len(errs) == iters
    assert np.array_equal(bits(m), bits(want(oracle, dims, iters)))


def test_gradients_from_image_keeps_the_triple(gpu, oracle):
    """The quad kernel reads dI; a slab told to derive the gradients from the
    image launches triples, with the same bits."""
    dims, iters = (257, 151), 13
    ref, mov = pair(dims)
    m, _, per_launch = slab_run(dims, iters, ref, mov, gi=1)
    assert per_launch == 3
    assert np.array_equal(bits(m), bits(want(oracle, dims, iters)))


@pytest.mark.parametrize("case", ["texture", "blob", "tiny"])
def test_quad_division_paths_bitwise(gpu, oracle, case):
    """As tests/test_gpu_hs.py::test_division_paths_bitwise, through quads (61
    iterations: fifteen quads and a single step):
      texture  gradients and sc in the unscaled division's range;
      blob     It = 0 outside a 20 x 20 blob: motion far below 2^-50 at the
               diffusion front (those wave-steps take the IEEE sequence);
      tiny     intensities ~1e-12: gradients below 2^-30, range_flag set (the
               IEEE sequence everywhere)."""
    n, iters = 200, 61
    ref, mov = S.texture_pair(n, seed=3)
    if case == "blob":
        blob = mov.copy()
        mov = ref.copy()
        mov[90:110, 90:110] = blob[90:110, 90:110]
    elif case == "tiny":
        ref, mov = ref * 1e-12, mov * 1e-12
    m, _, per_launch = slab_run((n, n), iters, ref, mov)
    assert per_launch == 4
    o = oracle_motion(oracle, (n, n), iters, ref, mov)
    assert np.array_equal(bits(m), bits(o))
    if case == "blob":  # the case does reach the scaled-division range
        a = np.abs(m[m != 0])
        assert a.min() < 2.0 ** -60


def kinds(iters, quads):
    """The kernel that produces each iteration of a fixed run of `iters`
    iterations (iter_schedule.h plan_fused): 'fused' for a quad or a triple
    (one geometry, one summation order), 'pair', 'single'."""
    k = []
    while len(k) < iters:
        left = iters - len(k)
        n = 4 if quads and left >= 4 else min(left, 3)
        k += [{1: "single", 2: "pair"}.get(n, "fused")] * n
    return k


@pytest.mark.parametrize("dims,iters,exact",
                         [((257, 151), 13, 13), ((257, 151), 12, 12), ((120, 37), 12, 12),
                          ((121, 37), 8, 6), ((4096, 8), 11, 9)],
                         ids=["257x151-13", "257x151-12", "120x37-12", "121x37-8", "4096x8-11"])
def test_quad_logger_errors_match_triples(gpu, dims, iters, exact):
    """13: three quads and a single step against four triples and the same
    single step; 12: three quads against four triples; every iteration exact.
    8: two quads against two triples and a pair (iterations 6, 7 at the
    tolerance); 11: two quads and a triple against three triples and a pair
    (iterations 9, 10 at the tolerance)."""
    ref, mov = pair(dims)
    mq, eq, kq = slab_run(dims, iters, ref, mov, quads=1)
    mt, et, kt = slab_run(dims, iters, ref, mov, quads=0)
    assert (kq, kt) == (4, 3)
    assert np.array_equal(bits(mq), bits(mt))
    assert len(eq) == len(et) == iters
    same = np.array([a == b for a, b in zip(kinds(iters, True), kinds(iters, False))])
    assert int(same.sum()) == exact and same[:exact].all()
    assert np.array_equal(bits(eq[same]), bits(et[same]))
    np.testing.assert_allclose(eq[~same].astype(np.float64), et[~same].astype(np.float64),
                               rtol=ERR_RTOL, atol=0)
