"""The field, Demons and pyramid kernels one launch at a time, against the
oracle's CPU primitives, on inputs chosen to break them.

Every entry of `opticalflow2d_amd.prim` makes one call of the launch function
the solvers call (csrc/of2d_prims.h, "test and diagnostic entries").  Every
comparison is on the float32 bit patterns (uint32 views, so -0.0 != +0.0):
that is the project's bar for these kernels and there is no tolerance in this
file, with one exception: the fp64 Logger sums of smooth_norm, a tree sum of
the reference's terms (test_smooth_norm_logger_sums, 1e-12 relative).

Inputs are seeded generators kept here.  A hostile field is a smooth random
base with planted pixels (PLANTS): sampling targets exactly on an integer, on
the last column / row (integer, fractional, one ulp below), outside on each of
the four sides by a fraction and by 1e6, a 64-pixel run of zero motion (a wave
that skips the division) and one with an odd pixel inside (a wave that mixes
both paths), displacements of -0.0 and +-1e-40; values of mixed sign, up to
1e30, subnormal (1e-40) and -0.0.
test_inputs_reach_what_they_claim (CPU) classifies every pixel the way the
kernels do and asserts each class is there.

Every input here is finite and every |coordinate| < 2^30.  NaN, inf and
beyond-int coordinates and non-finite sources live in
test_gpu_nonfinite_sampling.py, which holds the kernels to what the
reference's x86-64 build does with (int)floor(...) there (cvttss2si: INT_MIN,
so the pixel is outside and keeps its own value) and compares NaN positions
instead of NaN sign and payload, which differ between x86 and the GPU.
Gradients and the Demons force need dimx, dimy >= 2: the reference's one-sided
differences read past a one-pixel axis.

Arrays are in the C-ABI's layout: image [dimy, dimx], motion [dimy, dimx, 2].

Out of scope here: the SOR sweep, Fluid and Elastic kernels
(test_gpu_fluid_prims.py), the HS and seqnorm kernels (test_gpu_hs.py,
test_gpu_seqnorm.py), Curvature
(test_gpu_curvature_prims.py, test_gpu_dct.py, test_gpu_curvature*.py) and the slab
and rank layers.
"""
import functools

import numpy as np
import pytest

from opticalflow2d_amd import prim

gpu_test = pytest.mark.gpu
F = np.float32

# dimx x dimy: the smallest grids, the wave and block edges of the 64 x 4
# pixel blocks, pitch = dimx and the pitch rollover, one ragged medium case
SHAPES = [(1, 1), (1, 7), (7, 1), (3, 3), (5, 4), (63, 5), (64, 4), (65, 9), (127, 3), (128, 6),
          (129, 5), (200, 37)]
# the shapes with room for every planted class and both 64-pixel runs
FULL = [s for s in SHAPES if s[0] >= 64 and s[1] >= 4]
# (row0, nrows) of a 70 x 37 grid: the whole, top, middle, bottom, single rows
WINDOWS = [(0, 37), (0, 10), (5, 20), (30, 7), (36, 1), (1, 1)]
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


# ------------------------------------------------------------------ generators
def smooth(rng, dimy, dimx, comps, amp):
    """A few random plane waves of mixed sign, amplitude ~amp."""
    j, i = np.mgrid[0:dimy, 0:dimx].astype(np.float64)
    out = np.zeros((dimy, dimx, comps))
    for c in range(comps):
        for _ in range(3):
            kx, ky, ph = rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9), rng.uniform(0, 6.3)
            out[..., c] += rng.uniform(0.3, 1.0) * np.sin(kx * i + ky * j + ph)
    out = (amp * out / 2).astype(F)
    return out[..., 0] if comps == 1 else out


SPECIALS = [1e30, -1e30, 1e-40, -1e-40, -0.0, 0.0, 3.5e29, -7.25]


def hostile_values(dimx, dimy, seed, comps=1, amp=50.0, big=True):
    """Mixed-sign smooth values with planted magnitudes (big: up to 1e30),
    subnormals and -0.0; the last row and column hold some of them."""
    rng = np.random.default_rng(seed)
    a = smooth(rng, dimy, dimx, comps, amp).reshape(dimy, dimx, comps)
    sp = [v for v in SPECIALS if big or abs(v) < 1e29]
    n = min(len(sp) * 2, dimx * dimy)
    pos = rng.choice(dimx * dimy, size=n, replace=False)
    for k, p in enumerate(pos):
        a[p // dimx, p % dimx, k % comps] = F(sp[k % len(sp)])
    a[dimy - 1, dimx - 1, 0] = F(sp[seed % len(sp)])
    a[dimy - 1, 0, comps - 1] = F(-0.0)
    return a[..., 0].copy() if comps == 1 else a


def below(v):
    return float(np.nextafter(F(v), F(-np.inf)))


def axis_targets(d):
    """name -> target coordinate on an axis of length d."""
    return {
        "int": float(d // 2),
        "last": float(d - 1),
        "last_frac": d - 1 + 0.37,
        "last_below": below(d - 1),      # floor d - 2, fraction next to 1
        "frac": d // 2 + 0.25 if d > 1 else 0.25,
        "out_lo": -1e-6,
        "in_hi": below(d),               # dim - 1 + 1 - ulp: the last one inside
        "out_hi": float(d),
        "far_lo": -1e6,
        "far_hi": 1e6,
    }


# (x target, y target) of the planted pixels
PLANTS = ([(x, y) for x in ("int", "last", "last_frac", "last_below", "out_lo", "in_hi", "out_hi",
                            "far_lo", "far_hi") for y in ("int", "frac")] +
          [(x, y) for y in ("last", "last_frac", "last_below", "out_lo", "in_hi", "out_hi",
                            "far_lo", "far_hi") for x in ("int", "frac")] +
          [("last", "last"), ("last_frac", "last_frac"), ("last_below", "last_below"),
           ("last", "last_frac"), ("in_hi", "in_hi"), ("out_hi", "out_hi"), ("out_lo", "out_lo"),
           ("far_lo", "far_hi")])


def displacement(src, target):
    """float32 m with float32(src + m) == float32(target) where one exists."""
    src = int(src)
    t = F(target)
    m = F(float(t) - src)
    cands = [m]
    for _ in range(2):
        cands = [np.nextafter(cands[0], F(-np.inf))] + cands + [np.nextafter(cands[-1], F(np.inf))]
    res = [F(src) + c for c in cands]
    for c, r in zip(cands, res):
        if r == t:
            return c
    # not representable from this pixel: the nearest result on the target's
    # lower side (still below the integer, still outside)
    lower = [(r, c) for c, r in zip(cands, res) if r < t]
    return max(lower)[1] if lower else m


@functools.lru_cache(maxsize=None)
def hostile_motion(dimx, dimy, seed=0, row0=0, gdimy=None):
    """A displacement field [dimy, dimx, 2]: smooth sub-pixel to few-pixel base,
    then (where the grid has room) row 1 all zero for the first 64 pixels, row
    2 the same with one odd pixel inside, -0.0 and +-1e-40 displacements on the
    first pixels, then PLANTS on the free pixels.
    Targets are taken on a grid of gdimy rows of which this is rows row0..."""
    gdimy = dimy if gdimy is None else gdimy
    rng = np.random.default_rng(1000 * dimx + dimy + 7919 * seed)
    u = smooth(rng, dimy, dimx, 2, 2.5)
    free = np.ones((dimy, dimx), bool)
    tx, ty = axis_targets(dimx), axis_targets(gdimy)
    if dimx >= 64 and dimy >= 4:
        u[1, :64] = 0.0
        u[2, :64] = 0.0
        u[2, 37] = (displacement(37, tx["last_frac"]), F(0.0))  # weight 1 - fx: a division
        free[1:3, :64] = False
    u[0, 0] = (F(-0.0), F(-0.0))
    free[0, 0] = dimx * dimy == 1
    # subnormal displacements of both signs whose target stays the pixel itself
    if dimx > 1:
        u[0, 1] = (F(-1e-40), F(1e-40))
        free[0, 1] = False
    elif dimy > 1:
        u[1, 0] = (F(1e-40), F(-1e-40))
        free[1, 0] = False
    cells = [(j, i) for j in range(dimy) for i in range(dimx) if free[j, i]]
    step = max(1, len(cells) // (len(PLANTS) + 1))
    for k, (xs, ys) in enumerate(PLANTS):
        if k * step >= len(cells):
            break
        # small grids: rotate through PLANTS by seed so the shapes share them
        xs, ys = PLANTS[(k + seed * 5) % len(PLANTS)] if len(cells) < len(PLANTS) else (xs, ys)
        j, i = cells[k * step]
        u[j, i] = (displacement(i, tx[xs]), displacement(row0 + j, ty[ys]))
    u.setflags(write=False)
    return u


def classify(u, row0=0, gdimy=None):
    """Per pixel, in float32 as warp_px / accumulate_px do it: ok, ax, ay, the
    weight, which side the target is outside on, integer landing."""
    dimy, dimx, _ = u.shape
    gdimy = dimy if gdimy is None else gdimy
    j, i = np.mgrid[0:dimy, 0:dimx]
    px = i.astype(F) + u[..., 0]
    py = (j + row0).astype(F) + u[..., 1]
    assert px.dtype == F and py.dtype == F
    dx, dy = np.floor(px), np.floor(py)
    fx, fy = px - dx, py - dy
    one = F(1)
    c = dict(px=px, py=py, dx=dx, dy=dy, fx=fx, fy=fy)
    c["left"], c["right"] = dx < 0, dx >= dimx
    c["top"], c["bottom"] = dy < 0, dy >= gdimy
    c["ok"] = ~(c["left"] | c["right"] | c["top"] | c["bottom"])
    c["ax"], c["ay"] = dx < dimx - 1, dy < gdimy - 1
    w = (one - fx) * (one - fy)
    w = np.where(c["ax"], w + fx * (one - fy), w)
    w = np.where(c["ay"], w + (one - fx) * fy, w)
    w = np.where(c["ax"] & c["ay"], w + fx * fy, w)
    assert w.dtype == F
    c["w"] = w
    c["w1"] = w == one
    c["intx"], c["inty"] = fx == 0, fy == 0
    return c


def sampling_classes(u, row0=0, gdimy=None):
    """The planted classes present in u: name -> pixel count."""
    c = classify(u, row0, gdimy)
    dimy, dimx, _ = u.shape
    gdimy = dimy if gdimy is None else gdimy
    ok, near1 = c["ok"], F(1) - F(1e-4)
    lastx, lasty = c["dx"] == dimx - 1, c["dy"] == gdimy - 1
    cls = {
        "integer landing": ok & c["intx"] & c["inty"] & ((u[..., 0] != 0) | (u[..., 1] != 0)),
        "last column only, integer": ok & lastx & ~lasty & c["intx"],
        "last column only, fractional": ok & lastx & ~lasty & ~c["intx"] & (c["fx"] < 0.9),
        "below last column (fx near 1)": ok & (c["dx"] == dimx - 2) & (c["fx"] > near1),
        "last row only, integer": ok & lasty & ~lastx & c["inty"],
        "last row only, fractional": ok & lasty & ~lastx & ~c["inty"] & (c["fy"] < 0.9),
        "below last row (fy near 1)": ok & (c["dy"] == gdimy - 2) & (c["fy"] > near1),
        "last column and row, integer": ok & lastx & lasty & c["intx"] & c["inty"],
        "last column and row, fractional": ok & lastx & lasty & ~c["intx"] & ~c["inty"],
        "below last column and row": ok & (c["dx"] == dimx - 2) & (c["dy"] == gdimy - 2) &
                                     (c["fx"] > near1) & (c["fy"] > near1),
        "inside at dim - ulp (x)": ok & lastx & (c["fx"] > near1),
        "inside at dim - ulp (y)": ok & lasty & (c["fy"] > near1),
        "outside left by a fraction": c["left"] & (c["px"] > -1),
        "outside right at dim": c["px"] == dimx,
        "outside top by a fraction": c["top"] & (c["py"] > -1),
        "outside bottom at dim": c["py"] == gdimy,
        "outside left by 1e6": c["px"] < -9e5,
        "outside right by 1e6": c["px"] > 9e5,
        "outside top by 1e6": c["py"] < -9e5,
        "outside bottom by 1e6": c["py"] > 9e5,
        "edge weight != 1": ok & ~c["w1"] & (~c["ax"] | ~c["ay"]),
        "subnormal displacement > 0": ok & ((u > 0) & (u < np.finfo(F).tiny)).any(axis=2),
        "subnormal displacement < 0": ok & ((u < 0) & (u > -np.finfo(F).tiny)).any(axis=2),
        "displacement -0.0": ok & (np.signbit(u) & (u == 0)).any(axis=2),
    }
    return {k: int(v.sum()) for k, v in cls.items()}


def wave_runs(u):
    """(all-w==1 runs, mixed runs) over the 64-aligned pixel runs of full
    waves: lanes that are inside the image and whose target is in range."""
    c = classify(u)
    dimy, dimx, _ = u.shape
    all1 = mixed = 0
    for j in range(dimy):
        for i0 in range(0, dimx - 63, 64):
            need = (c["ok"] & ~c["w1"])[j, i0:i0 + 64]
            all1 += int(not need.any())
            mixed += int(need.any() and not need.all())
    return all1, mixed


# resampling pairs (fine, coarse), dimx x dimy, as the pyramid makes them
PAIRS = [((83, 70), (41, 35)), ((37, 23), (18, 11)), ((18, 11), (9, 5)), ((129, 65), (64, 32)),
         ((5, 4), (2, 2)), ((2, 2), (1, 1)), ((7, 1), (3, 1))]

# exp fields: (name, sqrt(max 2 y^2) aimed at, squarings expected)
EXP_CASES = [("small", 0.3, 0), ("below1", 1 - 1e-3, 1), ("above1", 1 + 1e-3, 2),
             ("below2", 2 * (1 - 1e-3), 2), ("above2", 2 * (1 + 1e-3), 3),
             ("below16", 16 * (1 - 1e-3), 5), ("above16", 16 * (1 + 1e-3), 6),
             ("large", 1000.0, 11), ("x_large_y_tiny", 0.01, 0)]
EXP_SHAPE = (65, 9)


@functools.lru_cache(maxsize=None)
def exp_field(name):
    dimx, dimy = EXP_SHAPE
    target = {n: t for n, t, _ in EXP_CASES}[name]
    f = smooth(np.random.default_rng(42), dimy, dimx, 2, 1.0).astype(np.float64)
    y = f[..., 1]
    f *= target / np.sqrt((2 * y * y).max())
    f = f.astype(F)
    if name == "x_large_y_tiny":
        f[..., 0] *= F(5000.0)  # |x| up to ~50: the count looks at .y alone
    f.setflags(write=False)
    return f


def reference_nsq(f):
    """Motion.cpp:51-58 and :253-261 in float32."""
    y = f[..., 1].astype(np.float64).reshape(-1)
    m = F(0)
    for s in (y * y + y * y).astype(F):
        m = s if m < s else m
    c = np.ceil(F(1) + np.log2(np.sqrt(m, dtype=F), dtype=F))
    return max(0, int(c))


# ------------------------------------------------------------------ CPU: inputs
def test_inputs_reach_what_they_claim():
    """Runs without a GPU: the planted classes are there, in float32 as the
    kernels compute them."""
    union = {}
    for dimx, dimy in SHAPES:
        for seed in (0, 1):
            u = hostile_motion(dimx, dimy, seed)
            assert np.isfinite(u).all() and np.abs(u).max() < 2.0 ** 30
            got = sampling_classes(u)
            for k, v in got.items():
                union[k] = union.get(k, 0) + v
            if (dimx, dimy) in FULL:
                missing = [k for k, v in got.items() if v == 0]
                assert not missing, f"{dimx}x{dimy} seed {seed}: no pixel of {missing}"
                all1, mixed = wave_runs(u)
                assert all1 >= 1 and mixed >= 1, (dimx, dimy, all1, mixed)
    assert all(v > 0 for v in union.values())
    # row windows of a taller grid (compose_zero): the classes on global rows
    for row0, nrows in WINDOWS:
        u = hostile_motion(70, nrows, 3, row0, 37)
        got = sampling_classes(u, row0, 37)
        for k in ("outside top by a fraction", "outside bottom at dim", "last row only, integer",
                  "outside left by a fraction", "outside right at dim",
                  "subnormal displacement > 0", "subnormal displacement < 0"):
            assert got[k] > 0, (row0, nrows, k)
    # values: mixed sign, 1e30, subnormal, -0.0
    for dimx, dimy in FULL:
        a = hostile_values(dimx, dimy, 5)
        assert (a > 0).any() and (a < 0).any() and np.abs(a).max() == F(1e30)
        assert ((a != 0) & (np.abs(a) < np.finfo(F).tiny)).any()
        assert (np.signbit(a) & (a == 0)).any() and np.isfinite(a).all()


def test_resample_pairs_reach_the_edges():
    for (dxi, dyi), (dxo, dyo) in PAIRS:
        # upsampling coarse -> fine (Field.tpp:172-176 in float32)
        i, j = np.arange(dxi, dtype=F), np.arange(dyi, dtype=F)
        px, py = i * F(dxo) / F(dxi), j * F(dyo) / F(dyi)
        dx, dy = np.floor(px), np.floor(py)
        fx, fy = (px - dx)[None, :], (py - dy)[:, None]
        ax, ay = (dx < dxo - 1)[None, :], (dy < dyo - 1)[:, None]
        one = F(1)
        w = (one - fx) * (one - fy)
        w = np.where(ax, w + fx * (one - fy), w)
        w = np.where(ay, w + (one - fx) * fy, w)
        w = np.where(ax & ay, w + fx * fy, w)
        assert (~ax).any() or (~ay).any(), "no pixel loses a tap"
        assert (w != one).any(), "every weight is 1"
        assert (dx < dxo).all() and (dy < dyo).all()
        # downsampling: the box never reaches past the input (the last tap row
        # is j*fy + jj <= dyo*fy - 1 <= dyi - 1 by the integer division, so the
        # kernels' `y >= dyi` skip is unreachable); odd sizes drop the last line
        bx, by = dxi // dxo, dyi // dyo
        if ((dxi, dyi), (dxo, dyo)) != ((2, 2), (1, 1)):
            assert dxo * bx < dxi or dyo * by < dyi


def test_exp_fields_have_the_intended_squarings():
    for name, _, nsq in EXP_CASES:
        assert reference_nsq(exp_field(name)) == nsq, name
    f = exp_field("x_large_y_tiny")
    assert np.abs(f[..., 0]).max() > 20 and np.abs(f[..., 1]).max() < 0.01


# ------------------------------------------------------------------ oracle side
def OL():
    from oracle import oracle as O
    return O.lib()


def o_warp(I, u):
    out = np.ascontiguousarray(I, F).copy()
    OL().oracle_warp2d(out, np.ascontiguousarray(u, F), I.shape[1], I.shape[0])
    return out


def o_accumulate(m_old, v):
    out = np.ascontiguousarray(m_old, F).copy()
    OL().oracle_accumulate(out, np.ascontiguousarray(v, F), v.shape[1], v.shape[0])
    return out


def o_kernel(kw, sigma):
    k = np.zeros(kw * kw, np.float64)
    OL().oracle_gaussian_kernel(kw, sigma, k)
    return k


def full_weight(k, kw):
    """The weight sum of a pixel with every tap valid, in Field.tpp:242-256's order."""
    c, w = (kw - 1) // 2, 0.0
    for ii in range(-c, c + 1):
        for jj in range(-c, c + 1):
            w += k[(ii + c) + (jj + c) * kw]
    return w


def o_smooth(f, kw, sigma):
    out = np.ascontiguousarray(f, F).copy()
    OL().oracle_convolute_motion(out, f.shape[1], f.shape[0], o_kernel(kw, sigma), kw)
    return out


def o_update(u, c, mode):
    if mode == 0:
        return o_accumulate(u, c)
    return (u + c) if mode == 1 else (u if mode == 2 else c)


def o_gradients(Iref, Iaux):
    dimy, dimx = Iref.shape
    dI = np.zeros((dimy, dimx, 2), F)
    It = np.zeros((dimy, dimx), F)
    OL().oracle_spatial_derivative(np.ascontiguousarray(Iaux, F), dimx, dimy, dI)
    OL().oracle_temporal_derivative(np.ascontiguousarray(Iref, F), np.ascontiguousarray(Iaux, F),
                                    dimx * dimy, It)
    return dI, It


def o_force(Iref, Imov, u, sigma_i, sigma_x):
    """(corr, rc): warp, derivatives, Demons.cpp:34-63."""
    dI, It = o_gradients(Iref, o_warp(Imov, u))
    c = np.zeros_like(dI)
    rc = OL().oracle_demons_force(dI, It, It.size, sigma_i, sigma_x, c)
    return c, rc


# ------------------------------------------------------------------ sampling
@gpu_test
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_warp(gpu, oracle, shape, seed):
    dimx, dimy = shape
    I, u = hostile_values(dimx, dimy, 5 + seed), hostile_motion(dimx, dimy, seed)
    same(prim.warp(I, u), o_warp(I, u), "warp")


@gpu_test
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_accumulate(gpu, oracle, shape, seed):
    dimx, dimy = shape
    m, v = hostile_values(dimx, dimy, 9 + seed, comps=2), hostile_motion(dimx, dimy, seed)
    same(prim.accumulate(m, v), o_accumulate(m, v), "accumulate")


@gpu_test
@pytest.mark.parametrize("zero_est", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_regrid(gpu, oracle, shape, zero_est):
    """est hostile onto a smooth motion; then est = 0, so that the new motion
    is the hostile old one and the fused warp sees the planted pixels."""
    dimx, dimy = shape
    I = hostile_values(dimx, dimy, 11)
    if zero_est:
        m_old, est = hostile_motion(dimx, dimy, 1), np.zeros((dimy, dimx, 2), F)
    else:
        m_old = smooth(np.random.default_rng(3), dimy, dimx, 2, 3.0)
        est = hostile_motion(dimx, dimy, 0)
    m_new, est0, Iaux = prim.regrid(m_old, est, I)
    want = o_accumulate(m_old, est)
    same(m_new, want, "regrid motion")
    same(est0, np.zeros_like(est0), "regrid zeroed estimate")
    same(Iaux, o_warp(I, want), "regrid Iaux")


@gpu_test
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_compose_zero(gpu, oracle, shape):
    dimx, dimy = shape
    v = hostile_motion(dimx, dimy, 1)
    same(prim.compose_zero(v), o_accumulate(np.zeros_like(v), v), "compose_zero")


@gpu_test
@pytest.mark.parametrize("window", WINDOWS, ids=ids)
def test_compose_zero_row_window(gpu, oracle, window):
    """Rows row0.. of a 70 x 37 grid: the slab form against the same rows of
    the oracle's full-grid result (the other rows hold a smooth field)."""
    row0, nrows = window
    full = smooth(np.random.default_rng(8), 37, 70, 2, 2.5)
    full[row0:row0 + nrows] = hostile_motion(70, nrows, 3, row0, 37)
    want = o_accumulate(np.zeros_like(full), full)[row0:row0 + nrows]
    same(prim.compose_zero(full[row0:row0 + nrows], row0, 37), want, "compose_zero window")


@gpu_test
@pytest.mark.parametrize("shape", [(1, 1), (65, 9), (129, 5)], ids=ids)
def test_add_motion_and_boundary_copies(gpu, shape):
    dimx, dimy = shape
    a, b = hostile_values(dimx, dimy, 1, comps=2), hostile_values(dimx, dimy, 2, comps=2)
    same(prim.add_motion(a, b), a + b, "add_motion")
    d = np.random.default_rng(dimx).normal(size=(dimy, dimx)) * 10.0 ** 20
    d[0, 0], d[-1, -1] = -0.0, 1e-40
    same(prim.d2f(d), d.astype(F), "d2f")
    img = hostile_values(dimx, dimy, 3)
    assert prim.f2d(img).tobytes() == img.astype(np.float64).tobytes()
    want = np.stack([a[..., 0], a[..., 1]]).astype(np.float64)
    assert prim.motion_to_planar(a).tobytes() == want.tobytes()


# ------------------------------------------------------------------ resampling
@gpu_test
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{ids(p[0])}-{ids(p[1])}")
def test_resample_pair_both_directions(gpu, oracle, pair):
    """The targets start from values of their own, as the kernels read them
    before they write.  For the sizes the launches accept no old value
    survives, though: a downsampled pixel always has a tap (the `y >= dyi` skip
    is unreachable, test_resample_pairs_reach_the_edges) and an upsampled one
    always a weight >= (1 - fx)(1 - fy) > 0, so what the pre-fill checks is
    that nothing of it leaks into the result."""
    (dxi, dyi), (dxo, dyo) = pair
    L = OL()
    img, mot = hostile_values(dxi, dyi, 21), hostile_values(dxi, dyi, 22, comps=2)
    fill_i, fill_m = hostile_values(dxo, dyo, 23), hostile_values(dxo, dyo, 24, comps=2)
    want = fill_i.copy()
    L.oracle_downsample_image(img, dxi, dyi, want, dxo, dyo)
    same(prim.downsample_image(img, fill_i), want, "downsample image")
    want = fill_m.copy()
    L.oracle_downsample_motion(mot, dxi, dyi, want, dxo, dyo)
    same(prim.downsample_motion(mot, fill_m), want, "downsample motion")
    # coarse -> fine, from a target that already holds values
    small = hostile_values(dxo, dyo, 25, comps=2)
    fill = hostile_values(dxi, dyi, 26, comps=2, big=False)
    want = fill.copy()
    L.oracle_upsample_motion(small, dxo, dyo, want, dxi, dyi)
    same(prim.upsample_motion(small, fill), want, "upsample motion")


# ------------------------------------------------------------------ gradients
@gpu_test
@pytest.mark.parametrize("shape", [(2, 2), (129, 5), (200, 37)], ids=ids)
def test_gradients_full_grid(gpu, oracle, shape):
    dimx, dimy = shape
    Iref, Iaux = hostile_values(dimx, dimy, 31), hostile_values(dimx, dimy, 32)
    dI, It = prim.gradients(Iref, Iaux)
    wI, wt = o_gradients(Iref, Iaux)
    same(dI, wI, "dI")
    same(It, wt, "It")


@gpu_test
@pytest.mark.parametrize("window", WINDOWS, ids=ids)
def test_gradients_row_window(gpu, oracle, window):
    row0, nrows = window
    Iref, Iaux = hostile_values(70, 37, 33), hostile_values(70, 37, 34)
    dI, It = prim.gradients(Iref, Iaux, row0, nrows)
    wI, wt = o_gradients(Iref, Iaux)
    same(dI, wI[row0:row0 + nrows], "dI window")
    same(It, wt[row0:row0 + nrows], "It window")


# ------------------------------------------------------------------ Demons
def textured(dimx, dimy, seed):
    """A mixed-sign image pair without flat patches (the force divides)."""
    rng = np.random.default_rng(seed)
    a = smooth(rng, dimy, dimx, 1, 40.0) + rng.normal(size=(dimy, dimx)).astype(F)
    b = a * F(0.9) + smooth(rng, dimy, dimx, 1, 6.0) + F(0.5)
    return a.astype(F), b.astype(F)


@gpu_test
@pytest.mark.parametrize("sigma_x", [0.25, 0.3])
@pytest.mark.parametrize("shape", [s for s in SHAPES if min(s) >= 2], ids=ids)
def test_demons_force(gpu, oracle, shape, sigma_x):
    dimx, dimy = shape
    Iref, Imov = textured(dimx, dimy, 41)
    u = hostile_motion(dimx, dimy, 0)
    want, rc = o_force(Iref, Imov, u, 1.0, sigma_x)
    got, status = prim.demons_force(Iref, Imov, u, 1.0, sigma_x)
    assert rc == 0 and status == 0
    same(got, want, "demons force")


@gpu_test
def test_demons_force_reports_a_zero_denominator(gpu, oracle):
    Iref = np.zeros((9, 65), F)
    u = np.zeros((9, 65, 2), F)
    _, rc = o_force(Iref, Iref, u, 1.0, 0.25)
    _, status = prim.demons_force(Iref, Iref, u, 1.0, 0.25)
    assert rc == -1 and status & 1


WIDTHS = [1, 2, 3, 4, 5, 6, 7, 9, 11, 15]
# (sigma, is (float)wfull == 1 for odd kw, for even kw): every tap of an odd
# kernel is inside the summed square, so its normalised sum is 1 whatever the
# sigma (the != 1 variants of widths 3, 5, 7 are not reachable through
# Kernel::set_gaussian); an even kernel sums a (kw - 1)^2 square of its kw^2
# taps: below 1 unless the Gaussian is so narrow that only the centre is not 0
SIGMAS = [(1.5, True, False), (0.05, True, True)]


def logger_sums(out, prev):
    """Motion::norm's terms (Motion.cpp:42-47) of the Logger's two norms, summed
    in fp64: |out - prev| (a float32 difference) and |prev|."""
    e, p = (out - prev).astype(np.float64), prev.astype(np.float64)
    return (np.sqrt(e[..., 0] ** 2 + e[..., 1] ** 2).sum(),
            np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2).sum())


def check_sums(sums, ref, what):
    for s, r in zip(sums, ref):
        print(f"{what}: sum {s!r} want {r!r} rel {abs(s - r) / r if r else 0.0:.3e}")
        assert abs(s - r) <= 1e-12 * r, what


def check_smoothing(dimx, dimy, kw, seed):
    # corr becomes a displacement in mode 0: no 1e30 there (|coordinate| < 2^30)
    corr = hostile_values(dimx, dimy, seed, comps=2, amp=3.0, big=False)
    u = hostile_values(dimx, dimy, seed + 1, comps=2, amp=3.0)
    umid = hostile_values(dimx, dimy, seed + 2, comps=2, amp=3.0)
    # the Logger sums: no 1e30, which one term would meet the bound with alone
    umid_s = hostile_values(dimx, dimy, seed + 3, comps=2, amp=3.0, big=False)
    prev_s = hostile_values(dimx, dimy, seed + 4, comps=2, amp=3.0, big=False)
    for sigma, odd1, even1 in SIGMAS:
        k = o_kernel(kw, sigma)
        wfull = full_weight(k, kw)
        assert (F(wfull) == F(1)) == (odd1 if kw % 2 else (even1 or kw == 1)), (kw, sigma, wfull)
        sm = o_smooth(corr, kw, sigma)
        for mode in range(4):
            got, w = prim.smooth_compose(corr, u, kw, sigma, mode)
            assert w == wfull, "the product's Gaussian is the oracle's"
            same(got, o_update(u, sm, mode), f"smooth_compose kw {kw} sigma {sigma} mode {mode}")
        sm = o_smooth(umid_s, kw, sigma)
        got, sums = prim.smooth_norm(umid_s, prev_s, kw, sigma, partials=True)
        same(got, sm, f"smooth_norm (sums) kw {kw} sigma {sigma}")
        check_sums(sums, logger_sums(sm, prev_s), f"smooth_norm {dimx}x{dimy} kw {kw} sigma {sigma}")
        sm = o_smooth(umid, kw, sigma)
        got, _ = prim.smooth_norm(umid, u, kw, sigma, partials=True)
        same(got, sm, f"smooth_norm kw {kw} sigma {sigma}")
        got, _ = prim.smooth_norm(umid, u, kw, sigma, partials=False)
        same(got, sm, f"smooth_norm (no partials) kw {kw} sigma {sigma}")


@gpu_test
@pytest.mark.parametrize("kw", WIDTHS)
@pytest.mark.parametrize("shape", [(70, 37), (130, 9)], ids=ids)
def test_smoothing_widths(gpu, oracle, shape, kw):
    check_smoothing(shape[0], shape[1], kw, 50 + kw)


@gpu_test
@pytest.mark.parametrize("dimy", [1, 3, 35])  # 35: above the 32-row tile
@pytest.mark.parametrize("dimx", [1, 2, 3, 5, 8])
def test_smoothing_narrow_grids(gpu, oracle, dimx, dimy):
    """dimx < kw: the linear-index tap rule wraps a tap across more than one
    j-line (Field.tpp:245-254), as on the coarsest pyramid levels."""
    for kw in (3, 5, 7, 9):
        check_smoothing(dimx, dimy, kw, 70 + kw)


@gpu_test
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_smooth_compose_hostile_composition(gpu, oracle, shape):
    """kw = 1 smooths nothing (one weight of 1, which only turns -0.0 into
    +0.0): the planted displacements reach the smoothing kernel's own
    composition (compose_px)."""
    dimx, dimy = shape
    c, u = hostile_motion(dimx, dimy, 0), hostile_values(dimx, dimy, 61, comps=2)
    for sigma in (1.5, 0.05):
        sm = o_smooth(c, 1, sigma)
        assert np.array_equal(sm, c)
        got, _ = prim.smooth_compose(c, u, 1, sigma, 0)
        same(got, o_accumulate(u, sm), "smooth_compose kw 1 mode 0")


@gpu_test
@pytest.mark.parametrize("kw", [3, 15])
@pytest.mark.parametrize("shape", [(70, 37), (5, 35)], ids=ids)
def test_smooth_norm_logger_sums(gpu, oracle, shape, kw):
    """The one comparison that is not bitwise: the launch's fp64 partial sums
    of |out - prev| and |prev| against an fp64 sum over the oracle's field,
    1e-12 relative.  check_smoothing asserts the same for every width, sigma
    and narrow grid; this is the plain case.

    The terms are Motion::norm's (Motion.cpp:42-47): the float32 field and
    difference, their squares, sum and root in fp64; only the order of the
    fp64 additions differs, ~1e-16 per term.  (With float32 squares and the
    hardware float32 root the launch came out 1.2e-8 .. 1.6e-8 below: this
    test found that and smooth_norm_kernel now takes the terms in fp64.)"""
    dimx, dimy = shape
    umid = hostile_values(dimx, dimy, 81, comps=2, amp=3.0, big=False)
    prev = hostile_values(dimx, dimy, 82, comps=2, amp=3.0, big=False)
    got, sums = prim.smooth_norm(umid, prev, kw, 1.5, partials=True)
    want = o_smooth(umid, kw, 1.5)
    same(got, want, "smooth_norm field")
    check_sums(sums, logger_sums(want, prev), f"smooth_norm sums {shape} kw {kw}")


@gpu_test
@pytest.mark.parametrize("dimy", [31, 33])
@pytest.mark.parametrize("dimx", [127, 128, 129, 191, 192])
def test_demons_update(gpu, oracle, dimx, dimy):
    """The fused kernel from dimx 128 on, the unfused pair below, against the
    oracle's force + convolute + update; sigma_x 0.25 squares to a power of
    two (the fused kernel multiplies by the reciprocal), 0.3 does not."""
    Iref, Imov = textured(dimx, dimy, 91)
    u = hostile_motion(dimx, dimy, 0)
    for sigma_x in (0.25, 0.3):
        c, rc = o_force(Iref, Imov, u, 1.0, sigma_x)
        assert rc == 0
        for kw in (3, 5, 7):
            sm = o_smooth(c, kw, 1.5)
            for mode in ((0, 1, 2, 3) if kw == 5 else (0,)):
                got, status = prim.demons_update(Iref, Imov, u, 1.0, sigma_x, kw, 1.5, mode)
                assert status == 0
                same(got, o_update(u, sm, mode),
                     f"demons_update {dimx}x{dimy} sigma_x {sigma_x} kw {kw} mode {mode}")


@gpu_test
@pytest.mark.parametrize("name", [c[0] for c in EXP_CASES])
def test_motion_exp(gpu, oracle, name):
    dimx, dimy = EXP_SHAPE
    f = exp_field(name)
    want = np.ascontiguousarray(f).copy()
    OL().oracle_motion_exp(want, dimx, dimy)
    got, nsq, status = prim.motion_exp(f)  # sigma_i 0: the bound is 32
    assert nsq == {n: k for n, _, k in EXP_CASES}[name]
    assert status == 0
    same(got, want, f"exp {name}")


@gpu_test
def test_motion_exp_reports_the_bound(gpu):
    """sigma_i / sigma_x = 4 bounds the count at 1; a field that needs 3
    squarings sets the status bit (the solver then raises)."""
    _, nsq, status = prim.motion_exp(exp_field("above2"), 1.0, 0.25)
    assert nsq == 3 and status & 2
