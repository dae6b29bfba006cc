"""The separable Gaussian smoothing of the Demons solvers ("demons_separable",
prim.*(method=1)) on the MI355X.

On the interior pixels (every tap's linear index inside the field) the
smoothing is a row pass along the linear index and a column pass with the
fp64 marginals of the normalised kw x kw table; every other pixel keeps the
direct form bit for bit.  The yardstick of the smoothing itself is a float64
evaluation of the reference's rule (Field.tpp:209-269) written below; the
registrations are held against the live oracle at SURVEY.md 8(c)'s bar
(1e-4 px, equal iteration counts).

Arrays are in the C-ABI's layout: image [dimy, dimx], motion [dimy, dimx, 2].
"""
import functools
import re

import numpy as np
import pytest

from opticalflow2d_amd import ImageRegistration, prim
from opticalflow2d_amd import synthetic as S

pytestmark = pytest.mark.gpu
F = np.float32

# 83 x 70: ragged, one partial tile column; 200 x 37: several tile columns, the
# x-edge wrap, dimy no tile multiple; 130 x (2c + 2): the fewest interior j-lines
WIDTHS = [3, 5, 7, 9, 15]
SIGMAS = [1.5, 2.5]


def grids(kw):
    return [(83, 70), (200, 37), (130, kw + 1)]


CASES = [(g, kw, s) for kw in WIDTHS for s in SIGMAS for g in grids(kw)]
case_ids = [f"{g[0]}x{g[1]}-kw{kw}-s{s}" for g, kw, s in CASES]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def field(dimx, dimy, seed):
    """Normal noise x 3 plus a constant 5 (the constant exposes normalisation)."""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(dimy, dimx, 2)) * 3.0 + 5.0).astype(F)


def table(kw, sigma):
    """Kernel::set_gaussian (Kernel.cpp:45-73) as the oracle builds it: fp64,
    idx = (ii + c) + (jj + c) * kw."""
    from oracle import oracle as O
    k = np.zeros(kw * kw, np.float64)
    O.lib().oracle_gaussian_kernel(int(kw), float(sigma), k)
    return k


def conv64(f, k, kw):
    """Field.tpp:209-269 in float64: tap (ii, jj) of pixel L is element L + ii
    + jj dimx of the LINEAR array, valid iff that index lies in [0, N); the sum
    over the valid taps divided by their weight sum."""
    dimy, dimx, _ = f.shape
    n, c = dimx * dimy, (kw - 1) // 2
    pad = c + c * dimx
    lin = np.zeros((n + 2 * pad, 2))
    lin[pad:pad + n] = f.reshape(n, 2).astype(np.float64)
    ok = np.zeros(n + 2 * pad)
    ok[pad:pad + n] = 1.0
    acc, w = np.zeros((n, 2)), np.zeros(n)
    for ii in range(-c, c + 1):
        for jj in range(-c, c + 1):
            o = pad + ii + jj * dimx
            kk = k[(ii + c) + (jj + c) * kw]
            acc += lin[o:o + n] * kk
            w += ok[o:o + n] * kk
    assert (w > 0).all()
    return (acc / w[:, None]).reshape(dimy, dimx, 2)


def interior(dimx, dimy, kw):
    """conv_px's predicate: lin - c - c dimx >= 0 and lin + c + c dimx < N."""
    c, n = (kw - 1) // 2, dimx * dimy
    lin = np.arange(n)
    return ((lin - c - c * dimx >= 0) & (lin + c + c * dimx < n)).reshape(dimy, dimx)


def bound(f, k, kw):
    """(2 kw + 8) 2^-24 S per pixel, S the same convolution of |f|: kw fp32
    multiply-adds per pass, the rounding of the row sums, one ulp per
    float-cast weight per pass and one ulp for the factorisation."""
    return (2 * kw + 8) * 2.0 ** -24 * conv64(np.abs(f), k, kw)


@functools.lru_cache(maxsize=None)
def smoothed(dimx, dimy, kw, sigma):
    """(field, direct, separable, path) of smooth_compose mode 3, once per case."""
    f = field(dimx, dimy, 1000 * kw + dimx)
    z = np.zeros_like(f)
    d, _, p0 = prim.smooth_compose(f, z, kw, sigma, 3, method=0)
    s, _, p1 = prim.smooth_compose(f, z, kw, sigma, 3, method=1)
    assert p0 == 0
    for a in (f, d, s):
        a.setflags(write=False)
    return f, d, s, p1


def check_bound(got, f, kw, sigma, what):
    k = table(kw, sigma)
    err = np.abs(got.astype(np.float64) - conv64(f, k, kw))
    ratio = float((err / bound(f, k, kw)).max())
    print(f"{what}: max |err| {err.max():.3e}, max err / bound {ratio:.3f}")
    assert ratio <= 1.0, what


# ------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("grid,kw,sigma", CASES, ids=case_ids)
def test_smoothing_against_fp64(gpu, oracle, grid, kw, sigma):
    f, _, s, path = smoothed(grid[0], grid[1], kw, sigma)
    assert path == 1
    assert interior(grid[0], grid[1], kw).any()
    check_bound(s, f, kw, sigma, f"separable {grid} kw {kw} sigma {sigma}")


@pytest.mark.parametrize("grid,kw,sigma", CASES, ids=case_ids)
def test_boundary_pixels_keep_the_direct_form(gpu, oracle, grid, kw, sigma):
    _, d, s, path = smoothed(grid[0], grid[1], kw, sigma)
    assert path == 1
    edge = ~interior(grid[0], grid[1], kw)
    c = (kw - 1) // 2
    assert edge.sum() == 2 * (c * grid[0] + c)
    assert np.array_equal(bits(s)[edge], bits(d)[edge])
    # and the interior is not the direct form's rounding everywhere: the
    # separable kernels did run there
    assert not np.array_equal(bits(s), bits(d))


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("grid,kw", [((83, 70), 4), ((83, 70), 1), ((83, 70), 17),
                                     ((11, 40), 13)],
                         ids=["kw4", "kw1", "kw17", "11x40-kw13"])
def test_fallbacks_run_the_direct_form(gpu, grid, kw):
    dimx, dimy = grid
    f, u = field(dimx, dimy, 7), field(dimx, dimy, 8)
    d, _, p0 = prim.smooth_compose(f, u, kw, 1.5, 3, method=0)
    s, _, p1 = prim.smooth_compose(f, u, kw, 1.5, 3, method=1)
    assert (p0, p1) == (0, 0)
    assert np.array_equal(bits(s), bits(d))
    d, ds, p0 = prim.smooth_norm(f, u, kw, 1.5, method=0)
    s, ss, p1 = prim.smooth_norm(f, u, kw, 1.5, method=1)
    assert (p0, p1) == (0, 0)
    assert np.array_equal(bits(s), bits(d)) and ss == ds
    Iref, Imov = images(dimx, dimy, 3)
    d, sd, p0 = prim.demons_update(Iref, Imov, u * F(0.1), 1.0, 0.25, kw, 1.5, 0, method=0)
    s, st, p1 = prim.demons_update(Iref, Imov, u * F(0.1), 1.0, 0.25, kw, 1.5, 0, method=1)
    assert (p0, p1) == (0, 0) and sd == st
    assert np.array_equal(bits(s), bits(d))


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("partials", [True, False], ids=["sums", "nosums"])
@pytest.mark.parametrize("grid,kw", [((83, 70), 5), ((200, 37), 9), ((130, 16), 15)],
                         ids=["83x70-kw5", "200x37-kw9", "130x16-kw15"])
def test_smooth_norm_separable(gpu, oracle, grid, kw, partials):
    """The bound of the smoothing, the boundary pixels bit for bit, and the
    launch's fp64 partial sums against the sums over the field it returned
    (1e-12 relative, as test_gpu_primitives.py holds the direct kernel)."""
    dimx, dimy = grid
    f, prev = field(dimx, dimy, 21), field(dimx, dimy, 22)
    got, sums, path = prim.smooth_norm(f, prev, kw, 1.5, partials=partials, method=1)
    assert path == 1
    check_bound(got, f, kw, 1.5, f"smooth_norm {grid} kw {kw}")
    direct, _, p0 = prim.smooth_norm(f, prev, kw, 1.5, partials=partials, method=0)
    edge = ~interior(dimx, dimy, kw)
    assert p0 == 0 and np.array_equal(bits(got)[edge], bits(direct)[edge])
    if not partials:
        assert sums is None
        return
    # Motion::norm's terms (Motion.cpp:42-47): float32 difference, fp64 squares
    e, p = (got - prev).astype(np.float64), prev.astype(np.float64)
    want = (np.sqrt(e[..., 0] ** 2 + e[..., 1] ** 2).sum(),
            np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2).sum())
    for s, r in zip(sums, want):
        print(f"smooth_norm {grid} kw {kw}: sum {s!r} want {r!r} rel {abs(s - r) / r:.3e}")
        assert abs(s - r) <= 1e-12 * r


# ------------------------------------------------------------------ 5
def images(dimx, dimy, seed):
    """A mixed-sign image pair without flat patches (the force divides)."""
    rng = np.random.default_rng(seed)
    j, i = np.mgrid[0:dimy, 0:dimx].astype(np.float64)
    a = 20.0 * np.sin(0.21 * i + 0.13 * j) + 15.0 * np.cos(0.17 * j - 0.05 * i)
    a = a + rng.normal(size=a.shape)
    b = 0.9 * a + 3.0 * np.sin(0.4 * i) * np.cos(0.3 * j) + 0.5
    return a.astype(F), b.astype(F)


def motion(dimx, dimy, seed):
    rng = np.random.default_rng(seed)
    j, i = np.mgrid[0:dimy, 0:dimx].astype(np.float64)
    u = np.stack([1.7 * np.sin(0.11 * i + 0.07 * j), 1.3 * np.cos(0.09 * j - 0.05 * i)], -1)
    return (u + 0.2 * rng.normal(size=u.shape)).astype(F)


@pytest.mark.parametrize("kw", [5, 9, 15])
@pytest.mark.parametrize("dimx", [200, 321])  # 321: two right-edge tile columns
def test_fused_equals_unfused(gpu, dimx, kw):
    dimy = 40
    Iref, Imov = images(dimx, dimy, dimx + kw)
    u = motion(dimx, dimy, kw)
    for sigma_x in (0.25, 0.3):  # multiplies by the reciprocal / divides
        corr, st_force = prim.demons_force(Iref, Imov, u, 1.0, sigma_x)
        for mode in (0, 1, 3):
            want, _, p_un = prim.smooth_compose(corr, u, kw, 1.5, mode, method=1)
            got, status, path = prim.demons_update(Iref, Imov, u, 1.0, sigma_x, kw, 1.5, mode,
                                                   method=1)
            assert (path, p_un) == (1, 1)
            assert status == st_force
            assert np.array_equal(bits(got), bits(want)), (dimx, kw, sigma_x, mode)


# ------------------------------------------------------------------ 6, 7
def run_oracle(oracle, dims, niter, nscales, reg, params, nrefine, ref, mov, fixed, verbose=0):
    o = oracle.Registration(dims, niter, nscales, reg, params, nrefine, verbose,
                            fixed_iters=bool(fixed))
    o.register(ref, mov)
    w = dict(motion=o.motion(), warped=o.warp(mov), iters=o.iterations(), errs=o.last_errors())
    o.close()
    return w


def expected_paths(dims, nscales, nrefine, kw, sep):
    out = []
    for s in range(nscales, -1, -1):
        out += [(dims[0] >> s, dims[1] >> s, kw, sep)] * nrefine
    return out


def check_registration(g, w, what):
    dm = float(np.abs(g["motion"] - w["motion"]).max())
    dw = float(np.abs(g["warped"] - w["warped"]).max())
    print(f"{what}: max |d motion| {dm:.3e} px, max |d warped| {dw:.3e}, iterations {g['iters']}")
    assert g["iters"] == w["iters"], what
    assert dm <= 1e-4, what
    assert dw <= 1e-4, what


FIXED = [
    ("thirion-83x70-kw5", (83, 70), 3, [1.0, 0.25, 1.5, 2.5, 5, 0], [12], 1.0),
    ("thirion-83x70-kw7", (83, 70), 3, [1.0, 0.25, 1.5, 2.5, 7, 0], [12], 1.0),
    # the fused kernel at a width the direct path cannot fuse
    ("thirion-388x150-kw9", (388, 150), 3, [1.0, 0.25, 1.5, 2.5, 9, 0], [6], 1.0),
    ("diffeomorphic-330x120-kw5", (330, 120), 4, [1.0, 2.0, 1.0, 1.0, 5], [5], 3.0),
]


@pytest.mark.parametrize("name,dims,reg,params,niter,gain", FIXED, ids=[c[0] for c in FIXED])
def test_registration_fixed_iterations(gpu, oracle, name, dims, reg, params, niter, gain):
    kw = int(params[4])
    ref, mov = S.texture_pair(dims[0], seed=dims[0] + kw, ny=dims[1])
    mov = mov * gain
    with ImageRegistration(dims, niter, 0, reg, params, 1, fixed_iters=1,
                           demons_separable=1) as r:
        r.register(ref, mov)
        g = dict(motion=r.motion(), warped=r.warp(mov), iters=r.iterations())
        assert r.demons_paths() == expected_paths(dims, 0, 1, kw, 1)
    w = run_oracle(oracle, dims, niter, 0, reg, params, 1, ref, mov, fixed=True)
    check_registration(g, w, name)


# The convergence-on case.  Seed and iteration limits were chosen on the CPU
# with the oracle: the first three loops run to their limits with every error
# far above the break threshold, and the last loop breaks one iteration before
# its limit (40 of 41) with every error more than 2.7 % of the threshold away
# from it; oracle_errors_clear asserts all of that before anything is compared.
CONV_SEED = 5
CONV = dict(dims=(128, 96), niter=[41, 10], nscales=1, reg=3,
            params=[1.0, 0.25, 2.0, 2.0, 5, 0], nrefine=2)
THRESHOLD = 0.001


def conv_pair():
    return S.texture_pair(128, seed=CONV_SEED, ny=96)


def oracle_errors_clear(oracle):
    """Every Logger error of the oracle's run is more than 1 % of the threshold
    away from it.  The last loop's errors are read in full precision; those of
    the earlier loops from the reference's own verbose lines, which print four
    decimals: a line other than 0.0010 is at least 5 % away."""
    ref, mov = conv_pair()
    oracle.lib().oracle_clear_output()
    w = run_oracle(oracle, CONV["dims"], CONV["niter"], CONV["nscales"], CONV["reg"],
                   CONV["params"], CONV["nrefine"], ref, mov, fixed=False, verbose=1)
    text = oracle.lib().oracle_captured_output().decode()
    oracle.lib().oracle_clear_output()
    printed = re.findall(r"Error:([0-9.]+)", text)
    assert len(printed) == sum(w["iters"]), (len(printed), w["iters"])
    earlier = printed[:sum(w["iters"][:-1])]
    assert "0.0010" not in earlier, earlier
    assert len(w["errs"]) == w["iters"][-1]
    # the break is taken, and in the last loop only
    assert w["iters"][:-1] == [10, 10, 41] and w["iters"][-1] < 41, w["iters"]
    assert (np.abs(w["errs"].astype(np.float64) - THRESHOLD) > 0.01 * THRESHOLD).all(), w["errs"]
    return w


def test_registration_convergence_on(gpu, oracle):
    """Pyramid, two refinements, convergence on: a moved break would change the
    iteration counts, and the fixture is first shown to be clear of the
    threshold so that it could not hide one."""
    w = oracle_errors_clear(oracle)
    ref, mov = conv_pair()
    with ImageRegistration(CONV["dims"], CONV["niter"], CONV["nscales"], CONV["reg"],
                           CONV["params"], CONV["nrefine"], demons_separable=1) as r:
        r.register(ref, mov)
        g = dict(motion=r.motion(), warped=r.warp(mov), iters=r.iterations())
        assert r.demons_paths() == expected_paths(CONV["dims"], 1, 2, 5, 1)
    check_registration(g, w, "thirion-128x96-pyramid-refine")


def test_toggle_back_to_the_direct_form(gpu, oracle):
    """One context: an estimate with the separable kernels, then the option
    off: the second result is the oracle's bit for bit.  A handle's motion
    carries over from one estimate to the next, so the first estimate registers
    the reference image onto itself: every force is zero and the motion stays
    exactly zero (asserted; the oracle does the same), and the second estimate
    starts where a fresh handle would."""
    dims, niter, params = (83, 70), [12], [1.0, 0.25, 1.5, 2.5, 5, 0]
    ref, mov = S.texture_pair(83, seed=50, ny=70)
    w = run_oracle(oracle, dims, niter, 0, 3, params, 1, ref, mov, fixed=True)
    with ImageRegistration(dims, niter, 0, 3, params, 1, fixed_iters=1, demons_separable=1) as r:
        r.register(ref, ref)
        assert r.demons_paths() == [(83, 70, 5, 1)]
        assert r.iterations() == [12] and not r.motion().any()
        r.set_option("demons_separable", 0)
        r.register(ref, mov)
        assert r.demons_paths() == [(83, 70, 5, 0)]
        assert r.iterations() == w["iters"]
        assert np.array_equal(r.motion(), w["motion"])
        assert np.array_equal(r.warp(mov), w["warped"])
