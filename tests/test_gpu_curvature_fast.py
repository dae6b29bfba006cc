"""Curvature registration with the fast line transforms ("curvature_dct" = 1)
against the oracle, at the bar of tests/test_gpu_curvature.py: max |du| <= 1e-5
px after the double -> float conversion and identical iteration counts.  The
fast path evaluates the oracle's REDFT10 / REDFT01 sums in another order
(through an FFT), all in fp64, so the same tolerance applies.  Every case
asserts what of2d_curvature_paths reports, so a fallback to the GEMMs cannot
pass as the fast path.
"""
import numpy as np
import pytest

from opticalflow2d_amd import ImageRegistration
from opticalflow2d_amd import synthetic as S

pytestmark = pytest.mark.gpu

TOL = 1e-5


def both(oracle, dims, niter, nscales, params, ref, mov, nrefine=1, **opt):
    with ImageRegistration(dims, niter, nscales, 1, params, nrefine, **opt) as r:
        r.register(ref, mov)
        g = dict(motion=r.motion(), warped=r.warp(mov), iters=r.iterations(),
                 paths=r.curvature_paths())
    o = oracle.Registration(dims, niter, nscales, 1, params, nrefine, 0,
                            fixed_iters=bool(opt.get("fixed_iters", 0)))
    o.register(ref, mov)
    w = dict(motion=o.motion(), warped=o.warp(mov), iters=o.iterations())
    o.close()
    return g, w


def pair(dims, seed):
    ref, mov = S.texture_pair(max(dims), seed=seed)
    return ref[: dims[0], : dims[1]], mov[: dims[0], : dims[1]]


@pytest.mark.parametrize("dims,fx,fy", [((64, 64), 1, 1), ((128, 32), 1, 1), ((32, 256), 1, 1),
                                        ((64, 37), 1, 0), ((70, 64), 0, 1)])
def test_fast_curvature_fixed_iterations(gpu, oracle, dims, fx, fy):
    ref, mov = pair(dims, 5)
    g, w = both(oracle, dims, [8], 0, [0.5, 0.2], ref, mov, fixed_iters=1, curvature_dct=1)
    assert g["paths"] == [(dims[0], dims[1], fx, fy)]
    assert g["iters"] == w["iters"] == [8]
    assert np.abs(g["motion"] - w["motion"]).max() <= TOL


def test_fast_curvature_pyramid_convergence(gpu, oracle):
    """Two levels, convergence break on: the coarse level (64 x 64) runs first."""
    ref, mov = S.texture_pair(128, seed=2)
    g, w = both(oracle, (128, 128), [60, 40], 1, [2.0], ref, mov, curvature_dct=1)
    assert g["paths"] == [(64, 64, 1, 1), (128, 128, 1, 1)]
    assert g["iters"] == w["iters"]
    assert np.abs(g["motion"] - w["motion"]).max() <= TOL
    assert np.abs(g["warped"] - w["warped"]).max() <= 1e-4


def test_fast_curvature_chunked_replay(gpu, oracle):
    ref, mov = S.texture_pair(64, seed=9)
    for chunk in (1, 7):
        g, w = both(oracle, (64, 64), [200], 0, [1.0, 0.5], ref, mov, chunk=chunk,
                    curvature_dct=1)
        assert g["paths"] == [(64, 64, 1, 1)]
        assert g["iters"] == w["iters"]
        assert np.abs(g["motion"] - w["motion"]).max() <= TOL


def test_fast_against_gemm(gpu):
    """The same registration by either path: the motions agree within the bar."""
    dims = (128, 64)
    ref, mov = pair(dims, 7)
    out = {}
    for dct in (0, 1):
        with ImageRegistration(dims, [12, 8], 1, 1, [0.5, 0.2], fixed_iters=1,
                               curvature_dct=dct) as r:
            r.register(ref, mov)
            out[dct] = (r.motion(), r.curvature_paths(), r.iterations())
    assert out[0][1] == [(64, 32, 0, 0), (128, 64, 0, 0)]
    assert out[1][1] == [(64, 32, 1, 1), (128, 64, 1, 1)]
    assert out[0][2] == out[1][2] == [8, 12]
    assert np.abs(out[0][0] - out[1][0]).max() <= TOL


def test_option_switches_between_registrations(gpu):
    """One handle: the level's tables follow the option from call to call.  A
    second handle that stays on the GEMMs runs the same calls (a handle's
    motion carries over from one register to the next), and the two agree
    within the bar after every call."""
    dims = (64, 37)
    ref, mov = pair(dims, 3)
    with ImageRegistration(dims, [6], 0, 1, [0.5, 0.2], fixed_iters=1) as r, \
            ImageRegistration(dims, [6], 0, 1, [0.5, 0.2], fixed_iters=1) as g:
        for dct, want in ((0, (64, 37, 0, 0)), (1, (64, 37, 1, 0)), (0, (64, 37, 0, 0)),
                          (1, (64, 37, 1, 0))):
            r.set_option("curvature_dct", dct)
            r.register(ref, mov)
            g.register(ref, mov)
            assert r.curvature_paths() == [want]
            assert g.curvature_paths() == [(64, 37, 0, 0)]
            assert np.abs(r.motion() - g.motion()).max() <= TOL
