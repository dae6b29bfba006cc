"""Deformation analysis on the device (`opticalflow2d_amd.field`, and the
same three calls on an ImageRegistration): the Jacobian determinant map with
its statistics, the inverse field, the similarity of two images.

The Jacobian map and every iterate of the inverse are held to the oracle bit
for bit (uint32 views).  The only tolerances are for fp64 sums taken in another
order than numpy's: the Jacobian mean (2 n 2^-53 relative, the bound for
reordering an fp64 sum of n terms) and MSE / NCC (1e-11 relative: the same
bound with margin for the final divisions, non-negative images, n <= 10^4).

Shapes are small on purpose: the failure modes are tile, pitch and edge
handling.  2x2, 2x65 and 65x2 are the smallest grids; 63x5, 64x64 and 65x33 lie
either side of the 64-pixel blocks; 97x61 and 130x33 are ragged in both axes
(130 also crosses the 128-pixel pitch and Jacobian tile).

Arrays are in the C-ABI's layout: image [dimy, dimx], motion [dimy, dimx, 2].
"""
import functools

import numpy as np
import pytest

from opticalflow2d_amd import ImageRegistration, field
from opticalflow2d_amd import synthetic as S
from opticalflow2d_amd.registration import INVERT_CHUNK

pytestmark = pytest.mark.gpu
F = np.float32

SHAPES = [(2, 2), (2, 65), (65, 2), (63, 5), (64, 64), (65, 33), (97, 61), (130, 33)]
# (dimx, dimy), amplitude: the inverse's converging cases (tol 1e-3)
INVERTIBLE = [((97, 61), 3.0), ((64, 64), 2.0), ((130, 33), 2.5)]
ids = lambda s: "x".join(str(v) for v in s) if isinstance(s, tuple) else str(s)  # noqa: E731


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    if len(bad):
        k = tuple(bad[0])
        pytest.fail(f"{what}: {len(bad)} of {g.size} words differ, first at {k}: "
                    f"got {np.asarray(got, F)[k]!r} want {np.asarray(want, F)[k]!r}")


def frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def sinusoids(dimx, dimy, amp):
    """ux = A sin(2 pi i / dimx + 0.3) cos(2 pi j / dimy),
    uy = 0.7 A cos(4 pi i / dimx) sin(2 pi j / dimy + 0.5)."""
    j, i = np.mgrid[0:dimy, 0:dimx].astype(np.float64)
    u = np.zeros((dimy, dimx, 2))
    u[..., 0] = amp * np.sin(2 * np.pi * i / dimx + 0.3) * np.cos(2 * np.pi * j / dimy)
    u[..., 1] = 0.7 * amp * np.cos(4 * np.pi * i / dimx) * np.sin(2 * np.pi * j / dimy + 0.5)
    return frozen(u.astype(F))


@functools.lru_cache(maxsize=None)
def noisy(dimx, dimy):
    """The smooth base plus seeded noise: mixed-sign derivatives everywhere."""
    rng = np.random.default_rng(dimx * 1000 + dimy)
    return frozen((sinusoids(dimx, dimy, 2.0) +
                   rng.uniform(-0.3, 0.3, (dimy, dimx, 2))).astype(F))


def oracle_jac(O, u):
    dimy, dimx, _ = u.shape
    jac = np.zeros((dimy, dimx), F)
    O.lib().oracle_jacobian(np.ascontiguousarray(u).reshape(-1), dimx, dimy, jac.reshape(-1))
    return jac


def check_jacobian(O, u):
    dimy, dimx, _ = u.shape
    n = dimx * dimy
    want = oracle_jac(O, u)
    jac, st = field.jacobian(u)
    same(jac, want, "jacobian map")
    assert F(st["min"]) == want.min() and F(st["max"]) == want.max()
    same(F(st["min"]), F(O.lib().oracle_image_min(want.reshape(-1), n)), "min vs oracle_image_min")
    assert st["folded"] == int((want <= 0).sum())
    assert st["below_half"] == int((want < F(0.5)).sum())
    w64 = want.astype(np.float64)
    mean = w64.mean()
    bound = 2 * n * 2.0 ** -53 * abs(mean)
    print(f"{dimx}x{dimy}: mean {st['mean']!r} numpy {mean!r} diff {abs(st['mean'] - mean):.3e} "
          f"bound {bound:.3e}")
    assert abs(st["mean"] - mean) <= bound
    none, st2 = field.jacobian(u, jac=False)
    assert none is None and st2 == st
    jac3, st3 = field.jacobian(u)
    assert np.array_equal(bits(jac3), bits(jac)) and st3 == st
    return want, st


# ------------------------------------------------------------------ Jacobian
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_jacobian(gpu, oracle, shape):
    check_jacobian(oracle, noisy(*shape))


def test_jacobian_planted_fold(gpu, oracle):
    """Amplitude 12 on 97 x 61 folds (the oracle's min J is about -0.257)."""
    want, st = check_jacobian(oracle, sinusoids(97, 61, 12.0))
    assert want.min() < -0.2
    assert st["folded"] > 0 and st["folded"] == int((want <= 0).sum())


def test_jacobian_of_zero_motion(gpu):
    jac, st = field.jacobian(np.zeros((5, 63, 2), F))
    assert np.array_equal(bits(jac), bits(np.ones((5, 63), F)))
    assert st == {"min": 1.0, "max": 1.0, "mean": 1.0, "folded": 0, "below_half": 0}


# ------------------------------------------------------------------ inverse
def planted_field(dimx, dimy, amp, planted=()):
    """sinusoids with NaN on the (j, i, component) words of `planted`."""
    u = sinusoids(dimx, dimy, amp).copy()
    for j, i, c in planted:
        u[j, i, c] = np.nan
    return frozen(u)


@functools.lru_cache(maxsize=None)
def invert_ref(dimx, dimy, amp, max_iter, tol, planted=()):
    """The loop of of2d_field_invert restated around oracle_accumulate.  The
    range test is the reference's, with its x86 conversion: a NaN coordinate
    converts to INT_MIN, which is outside the grid (as accumulate_px and
    oracle_accumulate take it)."""
    from oracle import oracle as O
    u = planted_field(dimx, dimy, amp, planted)
    i = np.arange(dimx, dtype=F)[None, :]
    j = np.arange(dimy, dtype=F)[:, None]
    v = np.zeros_like(u)
    res, n_oob, conv = [], 0, False
    for _ in range(max_iter):
        r = u.copy()
        O.lib().oracle_accumulate(r.reshape(-1), v.reshape(-1), dimx, dimy)
        with np.errstate(invalid="ignore"):
            fx, fy = np.floor(i + v[..., 0]), np.floor(j + v[..., 1])
            oob = (fx < 0) | (fx >= dimx) | (fy < 0) | (fy >= dimy) | np.isnan(fx) | np.isnan(fy)
        r[oob] = 0
        v = v - r
        assert v.dtype == F
        with np.errstate(invalid="ignore"):
            res.append(np.abs(r).max())  # NaN if any r is
        n_oob = int(oob.sum())
        if res[-1] < F(tol):
            conv = True
            break
    return frozen(v), frozen(np.array(res, F)), n_oob, conv


def check_invert(dimx, dimy, amp, max_iter, tol=1e-3):
    want_v, want_res, want_oob, want_conv = invert_ref(dimx, dimy, amp, max_iter, tol)
    v, info, res = field.invert(sinusoids(dimx, dimy, amp), max_iter=max_iter, tol=tol)
    print(f"{dimx}x{dimy} A={amp}: {info} residuals {res.tolist()}")
    assert info["iterations"] == len(want_res) and len(res) == len(want_res)
    same(res, want_res, "residuals")
    same(v, want_v, "inverse field")
    same(F(info["residual"]), want_res[-1], "reported residual")
    assert info["out_of_bounds"] == want_oob
    assert info["converged"] == want_conv
    return v, info, res


@pytest.mark.parametrize("shape,amp", INVERTIBLE, ids=ids)
def test_invert_converges(gpu, oracle, shape, amp):
    dimx, dimy = shape
    u = sinusoids(dimx, dimy, amp)
    v, info, _ = check_invert(dimx, dimy, amp, 50)
    assert info["converged"] and info["out_of_bounds"] <= 0.05 * dimx * dimy
    # (id + u) o (id + v) is the identity where it is defined
    r = u.copy()
    oracle.lib().oracle_accumulate(r.reshape(-1), v.reshape(-1), dimx, dimy)
    i = np.arange(dimx, dtype=F)[None, :]
    j = np.arange(dimy, dtype=F)[:, None]
    fx, fy = np.floor(i + v[..., 0]), np.floor(j + v[..., 1])
    inb = ~((fx < 0) | (fx >= dimx) | (fy < 0) | (fy >= dimy))
    assert np.abs(r[inb]).max() < 1e-3


@pytest.mark.parametrize("shape", [(2, 2), (2, 65), (65, 2), (63, 5), (65, 33)], ids=ids)
def test_invert_small_and_ragged(gpu, oracle, shape):
    check_invert(*shape, 1.0, 12)


def test_invert_folded_does_not_converge(gpu, oracle):
    _, info, res = check_invert(97, 61, 12.0, 60)
    assert not info["converged"] and info["iterations"] == 60 and len(res) == 60


def test_invert_single_update(gpu, oracle):
    _, info, _ = check_invert(97, 61, 3.0, 1)
    assert info["iterations"] == 1 and not info["converged"]


def test_invert_chunk_boundary(gpu, oracle):
    """The host reads the report once per INVERT_CHUNK updates; where the
    chunks end changes nothing.  The folded field never stops by itself, so the
    runs end below, on and beyond a boundary; the tight tolerance makes a
    converging field stop inside the second chunk."""
    runs = {}
    for max_iter in (INVERT_CHUNK - 3, INVERT_CHUNK, INVERT_CHUNK + 1, 2 * INVERT_CHUNK + 3):
        _, info, res = check_invert(97, 61, 12.0, max_iter)
        assert info["iterations"] == max_iter
        runs[max_iter] = res
    longest = runs[2 * INVERT_CHUNK + 3]
    for max_iter, res in runs.items():
        same(res, longest[:max_iter], f"prefix of {max_iter} updates")
    _, info, _ = check_invert(64, 64, 2.0, 50, tol=1e-5)
    assert info["converged"] and INVERT_CHUNK < info["iterations"] < 2 * INVERT_CHUNK


NAN_PLANTS = ((0, 0, 0), (16, 40, 1), (32, 64, 0))  # first pixel, interior, last pixel


@pytest.mark.parametrize("max_iter", [1, 2, 3])
def test_invert_nan_pixels(gpu, oracle, max_iter):
    """65 x 33 with three NaN words.  The first update starts from v = 0, so
    its coordinates are finite and the NaN arrives through the sampled values
    (at the planted pixels and their left and upper neighbours, weight 0); from
    the second update on those pixels carry a NaN coordinate with an in-range
    partner, which the reference's conversion puts outside the grid: they are
    counted, keep their v, and the count agrees with the composition two lines
    below it.  A NaN residual is never below the tolerance."""
    dimx, dimy, amp, tol = 65, 33, 1.0, 1e-3
    want_v, want_res, want_oob, want_conv = invert_ref(dimx, dimy, amp, max_iter, tol, NAN_PLANTS)
    assert not want_conv and len(want_res) == max_iter and np.isnan(want_res).all()
    assert np.isnan(want_v).sum() <= 0.25 * want_v.size
    assert (want_oob > 0) == (max_iter > 1)
    v, info, res = field.invert(planted_field(dimx, dimy, amp, NAN_PLANTS), max_iter=max_iter,
                                tol=tol)
    print(f"{max_iter} updates: {info}, oracle out_of_bounds {want_oob}")
    assert info["iterations"] == max_iter and not info["converged"]
    assert np.isnan(res).all() and np.isnan(info["residual"])
    assert info["out_of_bounds"] == want_oob
    nan = np.isnan(want_v)
    assert np.array_equal(np.isnan(v), nan)
    same(np.where(nan, F(0), v), np.where(nan, F(0), want_v), "inverse field beside the NaN")


def test_invert_repeatable(gpu):
    u = sinusoids(130, 33, 2.5)
    a, b = field.invert(u), field.invert(u)
    assert np.array_equal(bits(a[0]), bits(b[0])) and a[1] == b[1]
    assert np.array_equal(bits(a[2]), bits(b[2]))


# ------------------------------------------------------------------ similarity
def images(dimx, dimy):
    rng = np.random.default_rng(7 * dimx + dimy)
    a = rng.uniform(0.0, 1.0, (dimy, dimx)).astype(F)
    b = (0.6 * a + 0.4 * rng.uniform(0.0, 1.0, (dimy, dimx))).astype(F)
    return a, b


def numpy_similarity(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    da, db = a - a.mean(), b - b.mean()
    return ((a - b) ** 2).mean(), (da * db).mean() / np.sqrt((da * da).mean() * (db * db).mean())


@pytest.mark.parametrize("shape", [(2, 2), (63, 5), (64, 64), (97, 61), (130, 33), (300, 9)],
                         ids=ids)
def test_similarity(gpu, shape):
    a, b = images(*shape)
    mse, ncc = field.similarity(a, b)
    wm, wn = numpy_similarity(a, b)
    print(f"{shape}: mse {mse!r} numpy {wm!r}; ncc {ncc!r} numpy {wn!r}")
    assert abs(mse - wm) <= 1e-11 * abs(wm) and abs(ncc - wn) <= 1e-11 * abs(wn)
    assert field.similarity(a, b) == (mse, ncc)
    m0, n0 = field.similarity(a, a)
    assert m0 == 0.0 and abs(n0 - 1.0) <= 1e-11


def test_similarity_constant_image(gpu):
    a, _ = images(97, 61)
    for c in (0.0, 0.1, 0.7):
        flat = np.full_like(a, c)
        for x, y in ((a, flat), (flat, a), (flat, flat)):
            mse, ncc = field.similarity(x, y)  # OF2D_OK: no exception
            assert np.isnan(ncc)
            want = ((x.astype(np.float64) - y.astype(np.float64)) ** 2).mean()
            assert abs(mse - want) <= 1e-11 * want


# ------------------------------------------------------------------ on a registration
def interleaved(m):
    """[dimx, dimy, 2] (the boundary's layout) -> float32 [dimy, dimx, 2]."""
    return np.ascontiguousarray(np.transpose(np.asarray(m), (1, 0, 2)), dtype=F)


def image32(a):
    return np.ascontiguousarray(np.asarray(a).T, dtype=F)


@pytest.mark.parametrize("reg,niter,params,gain", [(0, [40], [0.1], 1.0),
                                                   (4, [10], [1.0, 2.0, 1.0, 1.0, 5], 3.0)],
                         ids=["hs", "diffeomorphic"])
def test_on_a_registration(gpu, oracle, reg, niter, params, gain):
    dims = (64, 48)
    ref, mov = S.texture_pair(64, seed=6, ny=48)
    mov = mov * gain
    with ImageRegistration(dims, niter, 0, reg, params, 1, fixed_iters=1) as r:
        r.register(ref, mov)
        m0 = r.motion()
        assert np.abs(m0).max() > 0.05  # something was estimated
        u = interleaved(m0)
        jac, st = r.jacobian()
        inv, info = r.inverse_motion()
        q = r.quality(ref, mov)
        warped = r.warp(mov)
        none, st2 = r.jacobian(jac=False)
        assert none is None and st2 == st
        assert np.array_equal(r.motion().view(np.uint64), m0.view(np.uint64))
    assert jac.shape == dims and inv.shape == dims + (2,)
    want = oracle_jac(oracle, u)
    same(jac.T, want, "jacobian of the registration's motion")
    assert np.array_equal(jac, jac.astype(F))  # float values, carried as double
    fj, fst = field.jacobian(u)
    assert st == fst
    fv, finfo, _ = field.invert(u)
    same(interleaved(inv), fv, "inverse of the registration's motion")
    assert info == finfo
    before = field.similarity(image32(ref), image32(mov))
    after = field.similarity(image32(ref), image32(warped))
    assert (q["mse_before"], q["ncc_before"]) == before
    assert (q["mse_after"], q["ncc_after"]) == after
    assert q["mse_after"] < q["mse_before"]  # the registration did register


# ------------------------------------------------------------------ the demo's report
def test_demo_report(gpu):
    """examples/demo_registration.py --report prints the analysis after the
    demo's own lines (which stay as they are without the flag)."""
    import os
    import re
    import subprocess
    import sys
    from conftest import ROOT
    demo = os.path.join(ROOT, "examples", "demo_registration.py")
    out = subprocess.run([sys.executable, demo, "--reg", "0", "--size", "64", "--report"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    text = out.stdout
    assert re.search(r"^min Jacobian ", text, re.M), text[-2000:]
    m = re.search(r"^Jacobian: min ([-0-9.]+) max ([-0-9.]+), folded pixels (\d+)$", text, re.M)
    assert m and float(m.group(1)) <= float(m.group(2)), text[-2000:]
    assert re.search(r"^Inverse: \d+ iterations, residual [0-9.e+-]+ px", text, re.M), text[-2000:]
    m = re.search(r"^MSE ([0-9.e+-]+) -> ([0-9.e+-]+), NCC ([-0-9.]+) -> ([-0-9.]+)$", text, re.M)
    assert m and float(m.group(2)) < float(m.group(1)), text[-2000:]
