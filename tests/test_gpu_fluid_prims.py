"""The SOR sweep, the Fluid step kernels and the Elastic Logger pass one launch
at a time, against the oracle's CPU primitives.

Every entry of `opticalflow2d_amd.prim` used here allocates a bare level with
the solver's own helpers and makes the launch calls Registration::loop_fluid /
loop_elastic make (csrc/of2d_prims.h).  What is held to what:

* every float32 output (v, R, maxabs, dt, the per-tile maxima, uo, the packed
  force, dI, It, the granules, the Jacobian minimum): on the bits (`same`),
  against oracle_sor_sweep, oracle_get_force, oracle_fluid_increment,
  oracle_motion_maxabs, oracle_jacobian + oracle_image_min,
  oracle_spatial_derivative and oracle_temporal_derivative;
* the fp64 Logger sums: 1e-12 relative (`check_sums`) against math.fsum of the
  reference's fp64 terms sqrt((double)x^2 + (double)y^2) (Motion.cpp:42-47).
  The kernels' fixed-order tree adds at most nb * 2^-53 relative (nb <= 60
  here);
* the decisions of fluid_report_decide_kernel: a float32 restatement of
  ImageRegistrationFluid.cpp:99-124 with Logger::update_error (Logger.cpp:
  32-51), `decide_reference`, on every word and every field of the report.

Inputs are seeded generators kept here.  The "moderate" family is
hostile_values(big=False) at amplitude 50 with planted +-1e6 spikes, +-1e-40
subnormals and -0.0 on the last row and column and beside every strip seam
(columns 63 k and 63 k + 1); the "big" family plants +-1e30, on two shapes.
NaN payloads differ between x86 and the GPU, so every input and every oracle
result is finite: test_cases_are_finite_and_hold_every_class (CPU).

Shapes are (dimx, dimy), the smallest that reach each branch of
sor_strip_kernel's group loops (head groups while g < 124, single interior
groups from dimy 191, the unrolled trip from dimy 287, one more 48-row group
at dimy = 19 + 48 k), its strip edges (63 columns a strip: dimx 65 | 66, 128 |
129) and the hand-over of launch_sor_increment between the fallback pair (28
tiles of 64 x 32) and the increment workers (29 and more).

Found by this file: fluid_step_kernel and logger_kernel took the Logger
magnitudes as sqrtf(ex * ex + ey * ey) in float32 and widened afterwards
(test_step, test_step_logger_sums_*, test_elastic_logger: 54 of their 56 sum
cases).  On fields of magnitude about one the sums were 6e-11 .. 4e-8
relative off, at 1e-25 they were 0, at 1e25 inf.  Both kernels now square and
root in fp64, as the Demons and Curvature kernels do; the sums agree with the
reference to 2.7e-16 or better.

Out of scope: epoch and ticket wrap-around after 2^32 sweeps.
"""
import functools
import math

import numpy as np
import pytest

from opticalflow2d_amd import prim
from test_gpu_primitives import SHAPES, check_sums, hostile_values, same

gpu_test = pytest.mark.gpu
F = np.float32
ids = lambda s: "x".join(str(v) for v in s) if isinstance(s, tuple) else str(s)  # noqa: E731

# (mu, lambda, omega): lambda != 0 couples the components; omega = 1 makes
# 1 - omega = +0 (signs of zero); omega > 1 over-relaxes with a negative 1 - omega
PARAMS = [(0.25, 0.0, 0.66), (0.5, 0.25, 0.66), (0.1, 0.0, 0.9), (0.3, 0.1, 1.0), (1.0, -0.5, 1.5)]
SWEEPS = (1, 2, 5)
SWEEP_X = [(dx, 37) for dx in (2, 3, 4, 64, 65, 66, 128, 129, 192)]
SWEEP_Y = [(66, dy) for dy in (2, 3, 4, 18, 19, 66, 67, 114, 115, 190, 191, 286, 287, 335)]
BIG_SHAPES = [(66, 19), (129, 191)]
POISON_SHAPES = [(66, 19), (129, 191), (322, 290)]
POISON_WORDS = (0x7FC00000, 0xFFFFFFFF)
# method 1: shape -> the path launch_sor_increment has to report
INC_SHAPES = {(193, 225): 1,   # 32 tiles
              (193, 224): 0,   # 28 tiles: the fallback pair
              (322, 290): 1,   # 6 strips, the last of 5 columns; ragged last tile row and column
              (130, 480): 1,
              (257, 225): 1,   # dimx = 64 k + 1: the last tile column has no relaxed column
              (258, 225): 1}
INC_PARAMS = [PARAMS[1], PARAMS[3], PARAMS[4]]
STEP_SHAPES = [(2, 2), (5, 4), (63, 5), (64, 32), (65, 33), (129, 65), (200, 37)]
DTS = (0.5, float(np.nextafter(F(65), F(0))), 65.0, float("inf"))
PACK_SHAPES = [s for s in SHAPES if s[0] >= 2 and s[1] >= 2] + [(65, 33), (130, 70)]
NOSTOP = 0x7F7F7F7F
UNWRITTEN = 0xABABABAB


def nstrips(dimx):
    return 0 if dimx < 3 else (dimx - 2 + 62) // 63


def ntiles(shape):
    return prim.increment_nblocks(*shape)


# ------------------------------------------------------------------ generators
def seam_columns(dimx):
    """The last column, and the last / first column of neighbouring strips."""
    cols = {dimx - 1}
    for k in range(1, dimx // 63 + 1):
        cols.update(c for c in (63 * k, 63 * k + 1) if c < dimx)
    return sorted(cols)


def plant_rows(dimy):
    return sorted({0, 1, dimy // 2, max(dimy - 2, 0), dimy - 1})


def motion_field(shape, seed, big=False, amp=50.0):
    """[dimy, dimx, 2]: mixed-sign smooth values with plants (module docstring)."""
    dimx, dimy = shape
    a = np.array(hostile_values(dimx, dimy, seed, comps=2, amp=amp, big=False))
    plants = [1e6, -1e6, 1e-40, -1e-40, -0.0] + ([1e30, -1e30] if big else [])
    n = seed
    for c in seam_columns(dimx):
        for r in plant_rows(dimy):
            a[r, c, n % 2] = F(plants[n % len(plants)])
            n += 1
    for i in range(0, dimx, max(1, dimx // 7)):
        a[dimy - 1, i, n % 2] = F(plants[n % len(plants)])
        n += 1
    a[dimy - 1, 0, 1] = F(-0.0)
    if dimx > 1:
        a[0, dimx - 1, 0] = F(1e-40)
    a.setflags(write=False)
    return a


def image_field(shape, seed):
    dimx, dimy = shape
    a = np.array(hostile_values(dimx, dimy, seed, comps=1, amp=50.0, big=False))
    a.setflags(write=False)
    return a


def seed_of(shape, k=0):
    return 131 * shape[0] + shape[1] + 7 * k


# ------------------------------------------------------------------ references
def lib(oracle):
    return oracle.lib()


def o_sweeps(oracle, v, b, params, counts):
    """{n: v after n sweeps} for n in counts."""
    dimy, dimx, _ = v.shape
    x = np.array(v)
    bb = np.ascontiguousarray(b)
    out = {}
    for n in range(1, max(counts) + 1):
        lib(oracle).oracle_sor_sweep(x.reshape(-1), bb.reshape(-1), dimx, dimy, *params)
        if n in counts:
            out[n] = x.copy()
    return out


def o_force(oracle, u, dI, It):
    f = np.zeros(u.shape, F)
    lib(oracle).oracle_get_force(np.ascontiguousarray(u).reshape(-1),
                                 np.ascontiguousarray(dI).reshape(-1),
                                 np.ascontiguousarray(It).reshape(-1), It.size, f.reshape(-1))
    return f


def o_increment(oracle, u, v):
    """(R, maxabs, dt, per-tile maxima) of OpticalFlowFluid.cpp:60-95."""
    dimy, dimx, _ = v.shape
    R = np.zeros(v.shape, F)
    lib(oracle).oracle_fluid_increment(np.ascontiguousarray(u).reshape(-1),
                                       np.ascontiguousarray(v).reshape(-1), dimx, dimy,
                                       R.reshape(-1))
    maxabs = F(lib(oracle).oracle_motion_maxabs(R.reshape(-1), dimx * dimy))
    with np.errstate(divide="ignore"):
        dt = F(0.65) / maxabs
    # Motion::maxabs's terms (float)(y^2 + y^2), their maximum per 64 x 32 tile from 0
    y = R[..., 1].astype(np.float64)
    q = (y * y + y * y).astype(F)
    nbx, nby = (dimx + 63) // 64, (dimy + 31) // 32
    part = np.zeros(nbx * nby, F)
    for by in range(nby):
        for bx in range(nbx):
            part[by * nbx + bx] = max(F(0), q[32 * by:32 * by + 32, 64 * bx:64 * bx + 64].max())
    return R, maxabs, dt, part


def logger_sums(cur, prev):
    """math.fsum of Motion::norm's fp64 terms of cur - prev (float32) and of prev."""
    e = cur - prev
    assert e.dtype == F
    e, q = e.astype(np.float64), prev.astype(np.float64)
    return (math.fsum(np.sqrt(e[..., 0] ** 2 + e[..., 1] ** 2).ravel()),
            math.fsum(np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2).ravel()))


def granules(col0, tag):
    g = np.zeros((col0.shape[0], 4), np.uint32)
    g[:, :2] = np.ascontiguousarray(col0, dtype=F).view(np.uint32)
    g[:, 2:] = tag
    return g


def same_words(got, want, what):
    assert got.dtype == np.uint32 and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} words differ, first at {tuple(bad[0])}"


@functools.lru_cache(maxsize=None)
def sweep_case(shape, params, big=False):
    """(v, b, {n: oracle v after n sweeps}); shared, read-only."""
    from oracle import oracle as O
    v = motion_field(shape, seed_of(shape, 1), big)
    b = motion_field(shape, seed_of(shape, 2), big)
    ref = o_sweeps(O, v, b, params, SWEEPS)
    for a in ref.values():
        a.setflags(write=False)
    return v, b, ref


@functools.lru_cache(maxsize=None)
def estimate(shape):
    return motion_field(shape, seed_of(shape, 3), amp=3.0)


# ------------------------------------------------------------------ CPU: the cases themselves
def subnormal(a):
    return (a != 0) & (np.abs(a) < np.finfo(F).tiny)


def negzero(a):
    return (a == 0) & np.signbit(a)


def test_cases_are_finite_and_hold_every_class(oracle):
    """Every input and every oracle result of the sweep cases is finite (no NaN
    payloads to compare), and the classes the module claims are there: a -0.0
    and a subnormal in the results, plants on interior rows of both columns of
    every strip seam, the big plants in the big family."""
    cases = ([(s, p, False) for s in SWEEP_X + SWEEP_Y + list(INC_SHAPES) + POISON_SHAPES
              for p in PARAMS] + [(s, p, True) for s in BIG_SHAPES for p in PARAMS])
    for shape, params, big in cases:
        v, b, ref = sweep_case(shape, params, big)
        assert np.isfinite(v).all() and np.isfinite(b).all(), (shape, params)
        for n, x in ref.items():
            assert np.isfinite(x).all(), (shape, params, n)
            assert negzero(x).any() and subnormal(x).any(), (shape, params, n)
        if big:
            assert (np.abs(v) >= 1e30).any() and (np.abs(b) >= 1e30).any()
        dimx, dimy = shape
        if dimx >= 3 and dimy >= 3:
            assert not np.array_equal(ref[1].view(np.uint32), v.view(np.uint32))
        planted = (np.abs(v) >= 1e6) | subnormal(v) | negzero(v)
        for c in seam_columns(dimx):
            assert planted[:, c].any(), (shape, c)
            if dimy >= 5 and 0 < c < dimx - 1:
                assert planted[1:dimy - 1, c].any(), (shape, c)
    for shape in INC_SHAPES:
        u = estimate(shape)
        for params in INC_PARAMS:
            _, _, ref = sweep_case(shape, params)
            R, maxabs, dt, part = o_increment(oracle, u, ref[1])
            assert np.isfinite(R).all() and np.isfinite(maxabs) and maxabs > 0 and np.isfinite(dt)
            assert F(np.sqrt(part.max())) == maxabs


def test_shapes_sit_where_the_module_says():
    assert [nstrips(d) for d in (2, 3, 64, 65, 66, 128, 129, 192, 322)] == [0, 1, 1, 1, 2, 2, 3, 4, 6]
    assert (322 - 2) - 5 * 63 == 5                      # the last strip's columns
    assert {s: int(ntiles(s) >= 29) for s in INC_SHAPES} == INC_SHAPES
    assert ntiles((193, 224)) == 28 and ntiles((193, 225)) == 32
    assert all(s[0] <= 322 and s[1] <= 480 for s in list(INC_SHAPES) + SWEEP_X + SWEEP_Y)
    assert DTS[1] < 65.0 and F(DTS[1]) < F(65) and F(DTS[2]) == F(65)


# ------------------------------------------------------------------ sweep, method 0
def check_sweep0(shape, params, big=False):
    v, b, ref = sweep_case(shape, params, big)
    for n in SWEEPS:
        r = prim.sor_sweep(v, b, *params, nsweeps=n)
        what = f"sor_sweep {shape} params {params} sweeps {n}{' big' if big else ''}"
        assert r["status"] == 0, what
        same(r["v"], ref[n], what)
        swept = shape[0] >= 3 and shape[1] >= 3
        assert r["words"][0] == (nstrips(shape[0]) * n if swept else 0), what


@gpu_test
@pytest.mark.parametrize("shape", SWEEP_X + SWEEP_Y, ids=ids)
def test_sweep(gpu, oracle, shape):
    """launch_sor: 1, 2 and 5 sweeps on one workspace (from the second on a
    strip meets the previous epoch's granules, with other values) for every
    parameter set; dimx < 3 or dimy < 3 leaves v as it was and takes no ticket."""
    for params in PARAMS:
        check_sweep0(shape, params)
    if shape[0] < 3 or shape[1] < 3:
        v, b, _ = sweep_case(shape, PARAMS[0])
        same(prim.sor_sweep(v, b, *PARAMS[0], nsweeps=2)["v"], v, f"no interior {shape}")


@gpu_test
@pytest.mark.parametrize("shape", BIG_SHAPES, ids=ids)
def test_sweep_big_values(gpu, oracle, shape):
    for params in PARAMS:
        check_sweep0(shape, params, big=True)


@gpu_test
@pytest.mark.parametrize("word", POISON_WORDS, ids=hex)
@pytest.mark.parametrize("shape", POISON_SHAPES, ids=ids)
def test_sweep_padding_cannot_reach_a_pixel(gpu, oracle, shape, word):
    """Every padding cell of the skewed array and every granule of every
    region hold `word` before v, b and the region-0 granules are written: the
    result is the one of a zeroed workspace, the oracle's."""
    for params in (PARAMS[1], PARAMS[4]):
        v, b, ref = sweep_case(shape, params)
        for method in (0, 1):
            kw = dict(u=estimate(shape)) if method else {}
            clean = prim.sor_sweep(v, b, *params, nsweeps=2, method=method, **kw)
            dirty = prim.sor_sweep(v, b, *params, nsweeps=2, method=method, poison=word, **kw)
            what = f"poison {word:#x} {shape} {params} method {method}"
            assert clean["status"] == 0 and dirty["status"] == 0, what
            same(dirty["v"], ref[2], what)
            same(dirty["v"], clean["v"], what)
            assert dirty["words"] == clean["words"], what
            if method:
                same(dirty["R"], clean["R"], what + " R")
                same(dirty["part"], clean["part"], what + " part")
                same([dirty["maxabs"], dirty["dt"]], [clean["maxabs"], clean["dt"]], what)


# ------------------------------------------------------------------ sweep, method 1
def check_increment_result(oracle, r, u, v_ref, what):
    R, maxabs, dt, part = o_increment(oracle, u, v_ref)
    same(r["R"], R, what + " R")
    same([r["maxabs"]], [maxabs], what + " maxabs")
    same([r["dt"]], [dt], what + " dt")
    same(r["part"], part, what + " part")
    return part


@gpu_test
@pytest.mark.parametrize("shape", list(INC_SHAPES), ids=ids)
def test_sweep_with_increment(gpu, oracle, shape):
    """launch_sor_increment: the path it takes, v as method 0 (the oracle's), R
    on the bits, maxabs = oracle_motion_maxabs(R), dt = 0.65f / maxabs, and the
    partial maxima in increment_kernel's slots."""
    u = estimate(shape)
    for params in INC_PARAMS:
        v, b, ref = sweep_case(shape, params)
        for n in (1, 2):
            r = prim.sor_sweep(v, b, *params, nsweeps=n, method=1, u=u)
            what = f"sor_sweep+increment {shape} {params} sweeps {n}"
            assert r["path"] == INC_SHAPES[shape], what
            assert r["status"] == 0, what
            same(r["v"], ref[n], what)
            part = check_increment_result(oracle, r, u, ref[n], what)
            same(prim.fluid_increment(u, ref[n])[3], part, what + " slots of launch_increment")
            ns, nt = nstrips(shape[0]), ntiles(shape)
            if r["path"]:
                # a launch adds ns + nwg to the role ticket and ntiles + 4 nwg to the tile counter
                nwg = r["words"][1] // n - ns
                assert r["words"] == (0, n * (ns + nwg), n * (nt + 4 * nwg)) and nwg >= 8, what
            else:
                assert r["words"] == (n * ns, 0, 0), what


@gpu_test
@pytest.mark.parametrize("shape", [(193, 225), (193, 224), (257, 225)], ids=ids)
def test_sweep_with_increment_zero_estimate(gpu, oracle, shape):
    """The regrid word set: R is the increment of a zero estimate (gradients +0)
    whatever the estimate's buffer holds."""
    params = INC_PARAMS[0]
    v, b, ref = sweep_case(shape, params)
    r = prim.sor_sweep(v, b, *params, method=1, u=estimate(shape), zero_est=True)
    assert r["path"] == INC_SHAPES[shape] and r["status"] == 0
    same(r["v"], ref[1], f"zero estimate {shape}")
    check_increment_result(oracle, r, np.zeros_like(v), ref[1], f"zero estimate {shape}")


@gpu_test
@pytest.mark.parametrize("shape", [(193, 225), (193, 224)], ids=ids)
def test_sweep_with_increment_zero_maxabs(gpu, oracle, shape):
    """R.y == 0 everywhere: maxabs 0 and dt = 0.65f / 0 = inf.  lambda = -mu
    uncouples the components, so v.y and b.y = 0 stay 0, and u.y = 0."""
    params = (0.5, -0.5, 0.9)
    v0, b0, _ = sweep_case(shape, PARAMS[0])
    v, b, u = np.array(v0), np.array(b0), np.array(estimate(shape))
    v[..., 1] = b[..., 1] = u[..., 1] = 0.0
    ref = o_sweeps(oracle, v, b, params, (1,))[1]
    R, maxabs, dt, _ = o_increment(oracle, u, ref)
    assert np.isfinite(ref).all() and not R[..., 1].any() and maxabs == 0 and np.isposinf(dt)
    r = prim.sor_sweep(v, b, *params, method=1, u=u)
    assert r["path"] == INC_SHAPES[shape] and r["status"] == 0
    same(r["v"], ref, f"zero maxabs {shape}")
    check_increment_result(oracle, r, u, ref, f"zero maxabs {shape}")


@gpu_test
@pytest.mark.parametrize("method,shape", [(0, (129, 191)), (1, (193, 225)), (1, (193, 224))],
                         ids=lambda v: ids(v))
def test_sweep_past_the_break_does_nothing(gpu, oracle, method, shape):
    """A launch of an iteration past the stop word changes neither v, R, the
    partials, the ticket nor the counters, and the sweeps after it are exact."""
    params = INC_PARAMS[0]
    v, b, ref = sweep_case(shape, params)
    kw = dict(method=method, u=estimate(shape)) if method else {}
    two = prim.sor_sweep(v, b, *params, nsweeps=2, **kw)
    same(two["v"], ref[2], "two sweeps")
    for skip in (1, 2):      # in the middle, at the end
        r = prim.sor_sweep(v, b, *params, nsweeps=3, skip_at=skip, **kw)
        what = f"skip {skip} of 3, method {method} {shape}"
        assert r["status"] == 0 and r["path"] == two["path"], what
        same(r["v"], ref[2], what)
        assert r["words"] == two["words"], what
        if method:
            same(r["R"], two["R"], what + " R")
            same(r["part"], two["part"], what + " part")
            same([r["maxabs"], r["dt"]], [two["maxabs"], two["dt"]], what)
    r = prim.sor_sweep(v, b, *params, nsweeps=1, skip_at=0, **kw)
    same(r["v"], v, "the only sweep skipped")
    assert r["words"] == (0, 0, 0) and r["status"] == 0
    if method:
        assert not r["R"].any() and not r["part"].any() and r["maxabs"] == 0 and r["dt"] == 0


# ------------------------------------------------------------------ increment
@gpu_test
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=ids)
def test_increment(gpu, oracle, shape):
    """launch_increment against oracle_fluid_increment and Motion::maxabs."""
    u, v = estimate(shape), motion_field(shape, seed_of(shape, 4))
    for zero in (False, True):
        R, maxabs, dt, part = prim.fluid_increment(u, v, zero_est=zero)
        r = dict(R=R, maxabs=maxabs, dt=dt, part=part)
        check_increment_result(oracle, r, np.zeros_like(u) if zero else u, v,
                               f"increment {shape} zero_est {zero}")


# ------------------------------------------------------------------ pack, regrid pack
def zero_sign_inputs(shape):
    """u = +0, It = -0.0 on every other pixel, gradients negative on every
    third: the force is +0 or -0 by the reference's order of operations."""
    dimx, dimy = shape
    u = np.zeros((dimy, dimx, 2), F)
    g = np.array(motion_field(shape, seed_of(shape, 5), amp=2.0))
    g[::, ::3] = -np.abs(g[::, ::3])
    it = np.array(image_field(shape, seed_of(shape, 6)))
    it.reshape(-1)[::2] = F(-0.0)
    return u, g, it


def pack_inputs(shape):
    return (estimate(shape), motion_field(shape, seed_of(shape, 5), amp=2.0),
            image_field(shape, seed_of(shape, 6)))


def test_zero_sign_case_has_both_zeros(oracle):
    for shape in PACK_SHAPES:
        f = o_force(oracle, *zero_sign_inputs(shape))
        assert negzero(f).any() and ((f == 0) & ~np.signbit(f)).any(), shape


@gpu_test
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=ids)
def test_sor_pack(gpu, oracle, shape):
    """launch_sor_pack in both modes: b = oracle_get_force on the bits (sign of
    zero included), v untouched (force only) or = u (Elastic), region 0 =
    column 0 of v tagged with the epoch."""
    v0 = motion_field(shape, seed_of(shape, 7))
    for name, (u, g, it) in (("hostile", pack_inputs(shape)), ("zeros", zero_sign_inputs(shape))):
        f = o_force(oracle, u, g, it)
        for epoch in (1, 0x80000001):
            v, b, gran = prim.sor_pack(u, g, it, v0=v0, epoch=epoch)
            what = f"sor_pack {name} {shape} epoch {epoch:#x}"
            same(b, f, what + " force only, b")
            same(v, v0, what + " force only, v")
            same_words(gran, granules(v0[:, 0], epoch), what + " force only, granules")
            v, b, gran = prim.sor_pack(u, g, it, epoch=epoch)
            same(b, f, what + " elastic, b")
            same(v, u, what + " elastic, v")
            same_words(gran, granules(u[:, 0], epoch), what + " elastic, granules")


@gpu_test
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=ids)
def test_regrid_pack(gpu, oracle, shape):
    """launch_regrid_pack under the control words: after a regrid dI, It are
    set_derivatives of the new warped image, b the force of a zero estimate,
    region 0 re-tagged; without one nothing is written."""
    dimx, dimy = shape
    Iref, Iaux = image_field(shape, seed_of(shape, 8)), image_field(shape, seed_of(shape, 9))
    v0 = motion_field(shape, seed_of(shape, 7))
    old = (motion_field(shape, seed_of(shape, 10)), image_field(shape, seed_of(shape, 11)),
           motion_field(shape, seed_of(shape, 12)))
    rng = np.random.default_rng(seed_of(shape))
    gold = rng.integers(0, 2 ** 32, (dimy, 4), dtype=np.uint32)
    dI, It, b, gran = prim.regrid_pack(Iref, Iaux, v0, 0, *old, gold, epoch=9)
    for name, got, want in zip(("dI", "It", "b"), (dI, It, b), old):
        same(got, want, f"regrid_pack without a regrid {shape}: {name}")
    same_words(gran, gold, f"regrid_pack without a regrid {shape}: granules")
    wd, wt = np.zeros((dimy, dimx, 2), F), np.zeros((dimy, dimx), F)
    lib(oracle).oracle_spatial_derivative(np.ascontiguousarray(Iaux).reshape(-1), dimx, dimy,
                                          wd.reshape(-1))
    lib(oracle).oracle_temporal_derivative(np.ascontiguousarray(Iref).reshape(-1),
                                           np.ascontiguousarray(Iaux).reshape(-1), dimx * dimy,
                                           wt.reshape(-1))
    dI, It, b, gran = prim.regrid_pack(Iref, Iaux, v0, 1, *old, gold, epoch=9)
    same(dI, wd, f"regrid_pack {shape}: dI")
    same(It, wt, f"regrid_pack {shape}: It")
    same(b, o_force(oracle, np.zeros_like(wd), wd, wt), f"regrid_pack {shape}: b")
    same_words(gran, granules(v0[:, 0], 9), f"regrid_pack {shape}: granules")


# ------------------------------------------------------------------ step
def step_reference(oracle, u, R, prev, dI, It, v0, dt, zero_est, epoch):
    """fluid_step_kernel from the reference's parts (OpticalFlowFluid.cpp:97-139,
    Logger.cpp:34-42, Image.cpp:189-218, OpticalFlow.cpp:15-39), float32."""
    dimy, dimx, _ = u.shape
    base = np.zeros_like(u) if zero_est else u
    dt = F(dt)
    with np.errstate(all="ignore"):
        un = base + R * dt if dt < F(65) else np.array(base)
    assert un.dtype == F
    pv = u if prev is None else prev      # the buffer's content, also after a regrid
    jac = np.zeros((dimy, dimx), F)
    with np.errstate(all="ignore"):
        lib(oracle).oracle_jacobian(np.ascontiguousarray(un).reshape(-1), dimx, dimy,
                                    jac.reshape(-1))
    jmin = F(lib(oracle).oracle_image_min(jac.reshape(-1), dimx * dimy))
    return dict(uo=un, sums=logger_sums(un, pv), jmin=jmin, b=o_force(oracle, un, dI, It),
                gran=granules(v0[:, 0], epoch + 1))


def step_inputs(shape):
    return dict(u=estimate(shape), R=motion_field(shape, seed_of(shape, 13), amp=1.0),
                prev=motion_field(shape, seed_of(shape, 14), amp=3.0),
                dI=motion_field(shape, seed_of(shape, 5), amp=2.0),
                It=image_field(shape, seed_of(shape, 6)), v0=motion_field(shape, seed_of(shape, 7)))


def check_step(oracle, a, dt, with_prev, zero, what, jacobian=True):
    prev = a["prev"] if with_prev else None
    want = step_reference(oracle, a["u"], a["R"], prev, a["dI"], a["It"], a["v0"], dt, zero, 5)
    got = prim.fluid_step(a["u"], a["R"], a["dI"], a["It"], a["v0"], dt, prev=prev,
                          zero_est=zero, epoch=5)
    same(got["uo"], want["uo"], what + " uo")
    same(got["b"], want["b"], what + " b")
    same_words(got["gran"], want["gran"], what + " granules")
    if jacobian:
        same([got["jmin"]], [want["jmin"]], what + " jmin")
    assert all(math.isfinite(s) for s in want["sums"]), what
    check_sums(got["sums"], want["sums"], what)
    return want


@gpu_test
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=ids)
def test_step(gpu, oracle, shape):
    """launch_fluid_step + launch_fluid_report: dt below, next to, on and above
    the threshold 65 (the last two copy the estimate), with a separate prev
    and with the input as prev, from the estimate and from the zero estimate
    of a regrid."""
    a = step_inputs(shape)
    for dt in DTS:
        for with_prev in (True, False):
            for zero in (False, True):
                want = check_step(oracle, a, dt, with_prev, zero,
                                  f"fluid_step {shape} dt {dt} prev {with_prev} zero_est {zero}")
                if dt >= 65 and not zero:
                    same(want["uo"], a["u"], "dt >= 65 copies u")


@gpu_test
@pytest.mark.parametrize("scale", (1.0, 1e-25, 1e25), ids=("unit", "tiny", "huge"))
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=ids)
def test_step_logger_sums_over_the_float_range(gpu, oracle, shape, scale):
    """Fields of magnitude about 1, 1e-25 and 1e25: float32 squares of the last
    two leave the float range (0 below ~1e-23, inf above 1.8e19), the
    reference's fp64 terms do not.  (The Jacobian of the 1e25 field overflows
    to inf - inf and is not compared.)"""
    dimx, dimy = shape
    rng = np.random.default_rng(1700 * dimx + dimy)
    a = step_inputs(shape)
    for k in ("u", "R", "prev"):
        a[k] = (scale * rng.standard_normal((dimy, dimx, 2))).astype(F)
    a["dI"] = rng.standard_normal((dimy, dimx, 2)).astype(F)
    a["It"] = rng.standard_normal((dimy, dimx)).astype(F)
    for with_prev in (True, False):
        want = check_step(oracle, a, 0.5, with_prev, False,
                          f"fluid_step sums {shape} scale {scale} prev {with_prev}",
                          jacobian=scale < 1e20)
        assert all(s > 0 for s in want["sums"])


# ------------------------------------------------------------------ elastic logger
@gpu_test
@pytest.mark.parametrize("scale", (None, 1.0, 1e-25, 1e25), ids=("hostile", "unit", "tiny", "huge"))
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=ids)
def test_elastic_logger(gpu, oracle, shape, scale):
    """launch_logger + launch_reduce_partials: u and the new prev are the
    working array's v on the bits, the sums the fp64 Logger's."""
    dimx, dimy = shape
    if scale is None:
        v, prev = motion_field(shape, seed_of(shape, 15)), motion_field(shape, seed_of(shape, 16))
    else:
        rng = np.random.default_rng(1900 * dimx + dimy)
        v = (scale * rng.standard_normal((dimy, dimx, 2))).astype(F)
        prev = (scale * rng.standard_normal((dimy, dimx, 2))).astype(F)
    u, pv, sums = prim.elastic_logger(v, prev)
    what = f"elastic_logger {shape} scale {scale}"
    same(u, v, what + " u")
    same(pv, v, what + " prev")
    want = logger_sums(v, prev)
    assert all(math.isfinite(s) and s > 0 for s in want)
    check_sums(sums, want, what)


# ------------------------------------------------------------------ decide
def decide_reference(lpart, jpart, seq, npx, fixed, it, words, scal, marker=F(-1234.5)):
    """fluid_report_decide_kernel's report and words (module docstring), float32;
    the partials of the cases sum exactly in any order."""
    status, stop, regrid, mcur = words
    if int(np.uint32(stop).view(np.int32)) < it:          # past the break: nothing
        return dict(words=tuple(words), flags=UNWRITTEN, scal2=marker)
    a, b = math.fsum(lpart[:, 0]), math.fsum(lpart[:, 1])
    m = F(np.inf)
    for x in jpart:
        m = x if x < m else m
    sd, sp = (F(seq[0]), F(seq[1])) if seq is not None else (F(a), F(b))
    n = F(npx)
    prevnorm, diffnorm = sp / n, sd / n
    err = F(0) if prevnorm == 0 else diffnorm / prevnorm
    assert type(err) is F
    brk = (not fixed) and bool(err < F(0.001)) and it > 1
    rg = (not brk) and bool(m < F(0.5))
    if brk:
        stop = min(int(np.uint32(stop).view(np.int32)), it)
    return dict(words=(status, stop, 1 if rg else 0, mcur ^ 1 if rg else mcur), sums=(a, b),
                maxabs=F(scal[0]), dt=F(scal[1]), jmin=m, seq=(sd, sp), err=err, scal2=m,
                status=status, flags=4 | (1 if brk else 0) | (2 if rg else 0))


def check_decide(lpart, jpart, seq, npx, fixed, it, words, what, scal=(1.25, 0.52)):
    want = decide_reference(lpart, jpart, seq, npx, fixed, it, words, scal)
    got = prim.fluid_decide(lpart, jpart, npx, fixed, it, words, seq=seq, scal=scal)
    assert got["words"] == want["words"], (what, got["words"], want["words"])
    assert got["flags"] == want["flags"], (what, got["flags"], want["flags"])
    same([got["scal2"]], [want["scal2"]], what + " scal[2]")
    if want["flags"] == UNWRITTEN:
        assert got["status"] == UNWRITTEN, what
        return want
    assert got["status"] == want["status"], what
    assert got["sums"] == want["sums"], (what, got["sums"], want["sums"])
    for k in ("maxabs", "dt", "jmin", "err"):
        same([got[k]], [want[k]], f"{what} {k}")
    same(list(got["seq"]), list(want["seq"]), what + " seq")
    return want


def decide_partials(nb, err, jmin, npx=4096.0):
    """nb partial pairs whose sums are exact in any order: sum |prev| = npx
    (prevnorm 1), sum |diff| = err * npx, in two halves; the Jacobian minimum in
    the last partial."""
    lp = np.zeros((nb, 2))
    lp[:, 1] = 1.0
    lp[nb - 1, 1] = npx - (nb - 1)
    lp[0, 0] += float(err) * npx / 2
    lp[nb - 1, 0] += float(err) * npx / 2
    jp = np.full(nb, 7.0, F)
    jp[: nb // 2] = F(0.75)
    if np.isinf(jmin):
        jp[:] = F(np.inf)
    jp[nb - 1] = F(jmin)
    return lp, jp


ERR_AT = F(0.001)
ERRS = (np.nextafter(ERR_AT, F(0)), ERR_AT, np.nextafter(ERR_AT, F(1)))
JMINS = (float(np.nextafter(F(0.5), F(0))), 0.5, -3.0, float("inf"))


@gpu_test
@pytest.mark.parametrize("fixed", (0, 1))
def test_decide_table(gpu, fixed):
    """Every row of the decision table: the break needs !fixed, err < 0.001f
    (one float either side, through the exact sums and through the fp64 sums)
    and it > 1; a break suppresses the regrid; the regrid needs jmin < 0.5f and
    flips the motion index."""
    seen = set()
    for it in (0, 1, 2):
        for err in ERRS:
            for via_seq in (False, True):
                for jmin in JMINS:
                    for mcur in (0, 1):
                        lp, jp = decide_partials(2, 0.5 if via_seq else err, jmin)
                        seq = (F(err) * F(64), F(64)) if via_seq else None
                        w = check_decide(lp, jp, seq, 4096.0, fixed, it, (0, NOSTOP, 1 - mcur, mcur),
                                         f"decide fixed {fixed} it {it} err {err!r} seq {via_seq} "
                                         f"jmin {jmin} mcur {mcur}")
                        same([w["err"]], [err], "the case's err")
                        seen.add(w["flags"])
    assert seen == ({4, 6} if fixed else {4, 5, 6})


@gpu_test
@pytest.mark.parametrize("nb", (1, 2, 1024, 1025, 2500))
def test_decide_partial_counts(gpu, nb):
    """The 1024-thread reduction at one partial, two, one per thread, one more
    and several per thread; the Jacobian minimum sits in the last partial."""
    for err, jmin, it in ((ERRS[0], JMINS[0], 2), (ERRS[2], JMINS[0], 2), (ERRS[0], 0.5, 1),
                          (ERRS[1], -3.0, 0)):
        npx = 4096.0
        lp, jp = decide_partials(nb, err, jmin, npx)
        w = check_decide(lp, jp, None, npx, 0, it, (3, NOSTOP, 0, 1), f"decide nb {nb} err {err!r}")
        same([w["jmin"]], [jmin], "the minimum is the last partial's")
    # random partials: the sums at the project's bar
    rng = np.random.default_rng(nb)
    lp, jp = rng.uniform(0.0, 3.0, (nb, 2)), rng.uniform(0.6, 2.0, nb).astype(F)
    got = prim.fluid_decide(lp, jp, 64.0 * nb, 1, 3, (0, NOSTOP, 0, 0))
    check_sums(got["sums"], (math.fsum(lp[:, 0]), math.fsum(lp[:, 1])), f"decide sums nb {nb}")
    same([got["jmin"]], [jp.min()], f"decide jmin nb {nb}")


@gpu_test
def test_decide_zero_prevnorm_and_stop_word(gpu):
    """prevnorm == 0 gives err 0 (a break from it = 2 on); a stop word that
    already holds this or an earlier iteration keeps it (atomicMin), a later
    one takes this one; a launch past the stop word writes nothing."""
    lp, jp = decide_partials(2, 0.25, 0.25)
    lp[:, 1] = 0.0
    for it in (1, 2, 5):
        w = check_decide(lp, jp, None, 4096.0, 0, it, (0, NOSTOP, 0, 0), f"prevnorm 0 it {it}")
        assert w["err"] == 0 and w["flags"] == (5 if it > 1 else 6)
    w = check_decide(lp, jp, (F(3), F(0)), 4096.0, 1, 2, (0, NOSTOP, 0, 0), "prevnorm 0, fixed")
    assert w["flags"] == 6
    lp, jp = decide_partials(3, ERRS[0], 0.25)
    for stop, it, after in ((2, 2, 2), (3, 2, 2), (7, 4, 4), (NOSTOP, 2, 2)):
        w = check_decide(lp, jp, None, 4096.0, 0, it, (1, stop, 1, 1), f"stop {stop} it {it}")
        assert w["words"] == (1, after, 0, 1) and w["flags"] == 5
    for stop, it in ((1, 2), (0, 1), (2, 7)):
        w = check_decide(lp, jp, None, 4096.0, 0, it, (1, stop, 1, 1), f"past the stop word {stop} {it}")
        assert w["flags"] == UNWRITTEN and w["words"] == (1, stop, 1, 1)
