"""The sampling kernels on NaN, inf and beyond-int coordinates and on non-finite
sources, one launch at a time against the oracle's CPU primitives, and a few
small registrations that make NaN motion by themselves.

The rule.  The reference converts a sampling coordinate with (int)floor(...),
which its x86-64 build performs with cvttss2si: a NaN, an inf and every value
beyond int give INT_MIN, so the range test that follows rejects the pixel and it
keeps its own value.  The device's conversion gives 0 for a NaN (a pixel inside
the grid) and saturates beyond int; floor_int() (csrc/of2d_device.h) restores
the NaN case, and every sampling kernel goes through it: warp_px,
accumulate_px, warp_batch, compose_px, exp_square_kernel, compose_zero_kernel
and the out-of-bounds count of invert_step_kernel (tests/test_gpu_analysis.py).
A non-finite tap is multiplied by its weight as in the reference, a zero weight
included (inf * 0 = NaN): the branch-free kernels must not skip it.

Bar: the rule of assert_bits in test_gpu_hs_division_range.py.  The positions of NaN are
equal and every other word has the oracle's float32 bits; NaN sign and payload
are not compared (x86 and the GPU differ there).  No case may hide behind NaN:
the CPU part asserts for every case that at most 25 % of the oracle's output
words are NaN, and that every coordinate class has a pixel whose kept own value
is not NaN (a NaN coordinate leaves the oracle's pixel at its own, finite
value, so those words are compared on their bits).

Inputs (generators below, C-ABI layout: image [dimy, dimx], motion
[dimy, dimx, 2]):
  coordinate classes (coord_motion): a smooth sub-pixel field with planted
    displacements, per component beside an in-range partner and in pairs: NaN,
    +-inf, +-3e9, a coordinate of exactly 2^31 (x86 INT_MIN, device INT_MAX),
    exactly -2^31 (a legitimate INT_MIN), exactly 2^31 - 128 (the largest float
    that is a valid int); (NaN, NaN), (NaN, 1e6), (-0.0, NaN), (+inf, -inf),
    (2^31, -2^31), (3e9, NaN); a NaN at pixel (0, 0) and at the last pixel; where
    the grid has room, row 1 holds a 64-pixel aligned run of zero motion with one
    NaN lane (that wave takes the `w != 1` ballot path for one lane only) and
    row 2 a 64-pixel run that is all NaN.  Small grids rotate through the
    plants by seed.
  value classes (value_image, value_motion): finite sub-pixel coordinates and a
    source with NaN, +inf and -inf at an interior pixel, in column 0, in the
    last column and in the last row; the pixels left of and above each planted
    one have zero motion, so the planted value is their right / lower tap with
    weight exactly 0.  Grids below 64 pixels take one +-inf plant (one NaN
    source pixel would put NaN into more than a quarter of their output).

The CPU part restates warp_px and the composition in float32 numpy with a
switch for the conversion: with the x86 rule the restatement equals the oracle
on the bits, with the device's rule (NaN -> 0) it differs from the oracle on
every input that carries a NaN coordinate whose other component is in range
(or NaN as well, which the device also turns into pixel 0): each such input
separates a kernel that converts correctly from one that does not.

Separable smoothing (smooth_compose method 1, kw 3): the separable kernels
round the smoothed correction differently from the reference's direct
convolution (their bar is in test_gpu_demons_separable.py), so for that path
the expected field is the oracle's composition of the launch's own smoothed
correction (mode 3, same method); the composition itself is still held to the
oracle's bits.
"""
import functools

import numpy as np
import pytest

from opticalflow2d_amd import prim
from opticalflow2d_amd import synthetic as S
from test_gpu_primitives import (OL, classify, displacement, exp_field, ids, o_accumulate,
                                 o_force, o_smooth, o_warp, smooth, textured)

gpu_test = pytest.mark.gpu
F = np.float32
NAN, INF = F(np.nan), F(np.inf)
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1
CAP = 0.25

SHAPES = [(1, 1), (3, 3), (7, 1), (65, 9), (129, 5)]
FULL = [(65, 9), (129, 5)]          # room for every plant and both runs
SMALL = [s for s in SHAPES if s not in FULL]
UPDATE_SHAPES = [(127, 31), (129, 33)]  # unfused / fused demons_update
SEEDS = (0, 1, 2, 3)
WINDOWS = [(5, 20), (30, 7)]        # (row0, nrows) of a 70 x 37 grid
PAIRS = [((37, 23), (18, 11)), ((5, 4), (2, 2))]

def assert_bits(got, expect, what):
    """The rule of test_gpu_hs_division_range.assert_bits (equal NaN masks, equal
    float32 bits everywhere else), naming the first word that differs."""
    g, w = np.asarray(got, F), np.asarray(expect, F)
    assert g.shape == w.shape, what
    gn, wn = np.isnan(g), np.isnan(w)
    bad = gn != wn
    if bad.any():
        k = tuple(int(v) for v in np.argwhere(bad)[0])
        pytest.fail(f"{what}: {int(bad.sum())} NaN positions differ, first at {k}: "
                    f"got {g[k]!r} want {w[k]!r}")
    bad = (g.view(np.uint32) != w.view(np.uint32)) & ~wn
    if bad.any():
        k = tuple(int(v) for v in np.argwhere(bad)[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {g.size} words differ, first at {k}: "
                    f"got {g[k]!r} want {w[k]!r}")


# ------------------------------------------------------------------ coordinates
COORD = {"nan": NAN, "+inf": INF, "-inf": -INF, "+3e9": F(3e9), "-3e9": F(-3e9),
         "2^31": F(2.0 ** 31), "-2^31": F(-2.0 ** 31), "2^31-128": F(2.0 ** 31 - 128),
         "1e6": F(1e6), "-0": F(-0.0), "in": F(0.25)}
EXACT = ("2^31", "-2^31", "2^31-128")   # the coordinate itself is the value
SINGLE = ["nan", "+inf", "-inf", "+3e9", "-3e9", "2^31", "-2^31", "2^31-128"]
PLANTS = ([(c, "in") for c in SINGLE] + [("in", c) for c in SINGLE] +
          [("nan", "nan"), ("nan", "1e6"), ("-0", "nan"), ("+inf", "-inf"), ("2^31", "-2^31"),
           ("+3e9", "nan")])


def component(name, src):
    return displacement(src, COORD[name]) if name in EXACT else COORD[name]


@functools.lru_cache(maxsize=None)
def coord_motion(dimx, dimy, seed=0, row0=0, gdimy=None, runs=True):
    """The planted displacement field of the module docstring; rows row0.. of a
    grid of gdimy rows."""
    rng = np.random.default_rng(77 * dimx + dimy + 7919 * seed)
    u = smooth(rng, dimy, dimx, 2, 0.45)
    free = np.ones((dimy, dimx), bool)
    if runs and dimx >= 64 and dimy >= 4:
        u[1, :64] = 0.0
        u[1, 37] = (NAN, F(0.0))
        u[2, :64] = NAN
        free[1:3, :64] = False
    if dimx * dimy > 1:
        u[0, 0] = (NAN, F(0.25))
        u[-1, -1] = (F(0.0), NAN)
        free[0, 0] = free[-1, -1] = False
    cells = [(j, i) for j in range(dimy) for i in range(dimx) if free[j, i]]
    step = max(1, len(cells) // (len(PLANTS) + 1))
    used = set()
    for k, (xs, ys) in enumerate(PLANTS):
        if k * step >= len(cells):
            break
        if len(cells) < len(PLANTS):
            xs, ys = PLANTS[(k + seed * 7) % len(PLANTS)]
        j, i = cells[k * step]
        if xs in EXACT and i >= 64:
            # from a column beyond 64 no float32 sum lands on -2^31 exactly
            planned = {cells[q * step] for q in range(len(PLANTS)) if q * step < len(cells)}
            j, i = next(c for c in cells if c[1] in range(i % 64, 64) and c not in planned | used)
        used.add((j, i))
        u[j, i] = (component(xs, i), component(ys, row0 + j))
    u.setflags(write=False)
    return u


def to_int(v, rule):
    """(int)floorf(v) of a float32 array as int64: "x86" gives INT_MIN for NaN,
    inf and beyond int (cvttss2si), "device" 0 for NaN and saturates."""
    with np.errstate(invalid="ignore"):
        fl = np.floor(v).astype(np.float64)
    nan, hi, lo = np.isnan(fl), fl >= 2.0 ** 31, fl < -2.0 ** 31
    out = np.where(nan | hi | lo, 0.0, fl).astype(np.int64)
    if rule == "x86":
        out[nan | hi | lo] = IMIN
    else:
        assert rule == "device"
        out[hi], out[lo] = IMAX, IMIN
    return out


def coordinates(u, row0=0):
    dimy, dimx, _ = u.shape
    j, i = np.mgrid[0:dimy, 0:dimx]
    with np.errstate(invalid="ignore"):
        return i.astype(F) + u[..., 0], (j + row0).astype(F) + u[..., 1]


def coord_classes(u, row0=0, gdimy=None):
    """name -> pixel mask, under the x86 rule.  "... | in": the other component
    is inside the grid, so the class alone decides."""
    dimy, dimx, _ = u.shape
    gdimy = dimy if gdimy is None else gdimy
    px, py = coordinates(u, row0)
    dx, dy = to_int(px, "x86"), to_int(py, "x86")
    inx, iny = (dx >= 0) & (dx < dimx), (dy >= 0) & (dy < gdimy)
    cls = {}
    for ax, p, other in (("x", px, iny), ("y", py, inx)):
        with np.errstate(invalid="ignore"):
            cls[f"{ax} nan | in"] = np.isnan(p) & other
            cls[f"{ax} +inf | in"] = (p == INF) & other
            cls[f"{ax} -inf | in"] = (p == -INF) & other
            cls[f"{ax} beyond int, high | in"] = np.isfinite(p) & (p > F(2.0 ** 31)) & other
            cls[f"{ax} beyond int, low | in"] = np.isfinite(p) & (p < F(-2.0 ** 31)) & other
            cls[f"{ax} 2^31 | in"] = (p == F(2.0 ** 31)) & other
            cls[f"{ax} -2^31 | in"] = (p == F(-2.0 ** 31)) & other
            cls[f"{ax} 2^31 - 128 | in"] = (p == F(2.0 ** 31 - 128)) & other
    with np.errstate(invalid="ignore"):
        cls["(nan, nan)"] = np.isnan(px) & np.isnan(py)
        cls["(nan, 1e6)"] = np.isnan(px) & (py > 9e5) & (py < 2e6)
        cls["(-0.0, nan)"] = np.signbit(u[..., 0]) & (u[..., 0] == 0) & np.isnan(py)
        cls["(+inf, -inf)"] = (px == INF) & (py == -INF)
        cls["(2^31, -2^31)"] = (px == F(2.0 ** 31)) & (py == F(-2.0 ** 31))
    return cls


def separating(u, row0=0, gdimy=None):
    """Pixels that the device's conversion samples and the x86 one skips: a NaN
    coordinate whose other component is in range, or NaN too."""
    dimy, dimx, _ = u.shape
    gdimy = dimy if gdimy is None else gdimy
    px, py = coordinates(u, row0)
    dx, dy = to_int(px, "device"), to_int(py, "device")
    return (np.isnan(px) | np.isnan(py)) & (dx >= 0) & (dx < dimx) & (dy >= 0) & (dy < gdimy)


def runs(u):
    """(64-aligned runs of in-range zero motion with exactly one NaN lane, runs
    whose every lane has a NaN coordinate)."""
    dimy, dimx, _ = u.shape
    px, py = coordinates(u)
    nan = np.isnan(px) | np.isnan(py)
    zero = (u[..., 0] == 0) & (u[..., 1] == 0)
    one = full = 0
    for j in range(dimy):
        for i0 in range(0, dimx - 63, 64):
            n, z = nan[j, i0:i0 + 64], zero[j, i0:i0 + 64]
            one += int(n.sum() == 1 and z.sum() == 63)
            full += int(n.all())
    return one, full


# ------------------------------------------------------------------ values
def finite_values(dimx, dimy, seed, comps=1):
    a = smooth(np.random.default_rng(500 + seed), dimy, dimx, comps, 50.0)
    return a.reshape(dimy, dimx) if comps == 1 else a


def value_positions(dimx, dimy):
    """(j, i) of the planted source pixels: interior, column 0, last column,
    last row."""
    pos = [(dimy // 2, dimx // 2), (min(dimy // 2 + 1, dimy - 1), 0), (min(1, dimy - 1), dimx - 1),
           (dimy - 1, dimx // 3)]
    return list(dict.fromkeys(pos))


def value_image(dimx, dimy, seed, comps=1, n=None, nan=None):
    """Smooth finite values with +inf, -inf and (from 64 pixels on) NaN planted
    at n of value_positions, rotated by seed."""
    a = finite_values(dimx, dimy, seed + 20, comps).reshape(dimy, dimx, comps).copy()
    pos = value_positions(dimx, dimy)
    big = dimx * dimy >= 64
    vals = [INF, NAN, -INF] if (big if nan is None else nan) else [INF, -INF]
    n = (len(pos) if big else 1) if n is None else n
    for k in range(n):
        j, i = pos[(k + seed) % len(pos)]
        a[j, i, (k + seed) % comps] = vals[(k + seed) % len(vals)]
    return a[..., 0].copy() if comps == 1 else a


@functools.lru_cache(maxsize=None)
def value_motion(dimx, dimy, scale=1.0):
    """Finite, sub-pixel; zero on the pixels left of and above each of
    value_positions (their right / lower tap gets weight exactly 0)."""
    u = smooth(np.random.default_rng(31 * dimx + dimy), dimy, dimx, 2, 0.45 * scale)
    for c, d in enumerate((dimx, dimy)):
        if d == 1:  # a negative fraction would leave a one-pixel axis
            u[..., c] = np.abs(u[..., c])
    pos = value_positions(dimx, dimy)
    for j, i in pos:
        u[j, i] = np.abs(u[j, i])  # the planted pixel samples itself
        for q in ((j, i - 1), (j - 1, i)):
            if q[0] >= 0 and q[1] >= 0 and q not in pos:
                u[q] = 0.0
    u.setflags(write=False)
    return u


def value_classes(src, u):
    """name -> count, for a source [dimy, dimx(, C)] sampled by the finite u."""
    dimy, dimx, _ = u.shape
    s = src.reshape(dimy, dimx, -1)
    bad = ~np.isfinite(s).all(axis=2)
    c = classify(u)
    dx, dy = c["dx"].astype(int), c["dy"].astype(int)
    ok = c["ok"]
    pad = np.zeros((dimy + 1, dimx + 1), bool)
    pad[:dimy, :dimx] = bad
    bx, by = np.where(ok, dx, 0), np.where(ok, dy, 0)
    cls = {"NaN": int(np.isnan(s).sum()), "+inf": int((s == INF).sum()),
           "-inf": int((s == -INF).sum()),
           "sampled": int((ok & (pad[by, bx] | (c["ax"] & pad[by, bx + 1]) |
                                 (c["ay"] & pad[by + 1, bx]) |
                                 (c["ax"] & c["ay"] & pad[by + 1, bx + 1]))).sum()),
           "right tap of a zero fraction": int((ok & c["ax"] & c["intx"] & pad[by, bx + 1]).sum()),
           "lower tap of a zero fraction": int((ok & c["ay"] & c["inty"] & pad[by + 1, bx]).sum()),
           "interior": int(bad[1:-1, 1:-1].sum()), "column 0": int(bad[:, 0].sum()),
           "last column": int(bad[:, -1].sum()), "last row": int(bad[-1].sum())}
    return cls


# ------------------------------------------------------------------ restatement
def bilinear(src, u, rule, row0=0):
    """The taps and weights of Image::warp2d / Motion::accumulate in float32:
    src [gdimy, dimx, C], u rows row0.. -> (ok, w, val [dimy, dimx, C])."""
    gdimy, dimx, C = src.shape
    px, py = coordinates(u, row0)
    with np.errstate(all="ignore"):
        dx, dy = to_int(px, rule), to_int(py, rule)
        fx, fy = px - dx.astype(F), py - dy.astype(F)
        ok = ~((dx < 0) | (dx >= dimx) | (dy < 0) | (dy >= gdimy))
        ax, ay = dx < dimx - 1, dy < gdimy - 1
        flat = np.concatenate([src.reshape(-1, C), np.zeros((dimx + 2, C), F)])
        b = np.where(ok, dy * dimx + dx, 0)
        one = F(1)
        a0, a1, b0, b1 = ((one - fx)[..., None], fx[..., None], (one - fy)[..., None],
                          fy[..., None])
        val = (flat[b] * a0) * b0
        w = (one - fx) * (one - fy)
        val = np.where(ax[..., None], val + (flat[b + 1] * a1) * b0, val)
        w = np.where(ax, w + fx * (one - fy), w)
        val = np.where(ay[..., None], val + (flat[b + dimx] * a0) * b1, val)
        w = np.where(ay, w + (one - fx) * fy, w)
        val = np.where((ax & ay)[..., None], val + (flat[b + dimx + 1] * a1) * b1, val)
        w = np.where(ax & ay, w + fx * fy, w)
    assert val.dtype == F and w.dtype == F
    return ok, w, val


def r_warp(I, u, rule):
    ok, w, val = bilinear(I[..., None], u, rule)
    with np.errstate(all="ignore"):
        return np.where(ok & (w != 0), val[..., 0] / w, I)


def r_accumulate(m, v, rule, row0=0):
    """m: the whole grid; v: rows row0.. -> those rows of the composition."""
    ok, w, val = bilinear(m, v, rule, row0)
    with np.errstate(all="ignore"):
        q = v + val / w[..., None]
    own = m[row0:row0 + v.shape[0]]
    return np.where(ok[..., None], np.where((w != 0)[..., None], q, v), own)


def nan_share(*arrays):
    n = sum(int(np.isnan(a).sum()) for a in arrays)
    return n / sum(a.size for a in arrays)


def under_cap(what, *arrays):
    share = nan_share(*arrays)
    assert share <= CAP, f"{what}: {share:.1%} of the oracle's words are NaN"


# ------------------------------------------------------------------ cases
KINDS = ("coord", "value")
SAMPLING = [(s, k, seed) for s in SHAPES for k in KINDS for seed in SEEDS]
sid = lambda c: f"{ids(c[0])}-{c[1]}-{c[2]}"  # noqa: E731


@functools.lru_cache(maxsize=None)
def sampling_inputs(shape, kind, seed):
    """(image, motion values, sampling field)."""
    dimx, dimy = shape
    if kind == "coord":
        out = (finite_values(dimx, dimy, seed), finite_values(dimx, dimy, seed + 5, 2),
               coord_motion(dimx, dimy, seed))
    else:
        out = (value_image(dimx, dimy, seed), value_image(dimx, dimy, seed + 1, 2),
               value_motion(dimx, dimy))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want_warp(shape, kind, seed):
    I, _, u = sampling_inputs(shape, kind, seed)
    return o_warp(I, u)


@functools.lru_cache(maxsize=None)
def want_accumulate(shape, kind, seed):
    _, m, u = sampling_inputs(shape, kind, seed)
    return o_accumulate(m, u)


# (the small grids have no "old" variant: the planted old values, which the
# output keeps, would be more than a quarter of it)
REGRID = [(s, v, seed) for s in SHAPES for v in ("est", "old", "value") for seed in SEEDS[:2]
          if v != "old" or s in FULL]


@functools.lru_cache(maxsize=None)
def regrid_case(shape, variant, seed):
    """est: the planted estimate onto a smooth motion; old: est = 0, so the new
    motion is the planted old one (without the runs: the identity composition
    spreads every NaN to its left and upper neighbours) and the fused warp sees
    it; value: a non-finite image and old motion under a finite estimate.
    -> (m_old, est, I, m_new, Iaux)."""
    dimx, dimy = shape
    if variant == "est":
        m_old = smooth(np.random.default_rng(3), dimy, dimx, 2, 0.4)
        est, I = coord_motion(dimx, dimy, seed), finite_values(dimx, dimy, seed)
    elif variant == "old":
        m_old = coord_motion(dimx, dimy, seed, runs=False)
        est, I = np.zeros((dimy, dimx, 2), F), finite_values(dimx, dimy, seed)
    else:
        I, m_old, est = sampling_inputs(shape, "value", seed)
    m_new = o_accumulate(m_old, est)
    return m_old, est, I, m_new, o_warp(I, m_new)


@functools.lru_cache(maxsize=None)
def window_case(window):
    row0, nrows = window
    full = smooth(np.random.default_rng(8), 37, 70, 2, 0.45)
    full[row0:row0 + nrows] = coord_motion(70, nrows, 3, row0, 37)
    return full, o_accumulate(np.zeros_like(full), full)[row0:row0 + nrows]


FORCE_SHAPES = [s for s in SHAPES if min(s) >= 2]
FORCE = [(s, k) for s in FORCE_SHAPES for k in KINDS if not (k == "value" and s == (3, 3))]


@functools.lru_cache(maxsize=None)
def force_case(shape, kind, sigma_x=0.25):
    """coord: NaN, inf and beyond-int in u; value: NaN and inf in Imov (two
    plants: the warp and the gradients spread each over a dozen pixels; no room
    on 3 x 3).  -> (Iref, Imov, u, corr, rc)."""
    dimx, dimy = shape
    Iref, Imov = textured(dimx, dimy, 41)
    if kind == "coord":
        u = coord_motion(dimx, dimy, 1)
    else:
        u = value_motion(dimx, dimy)
        plant = value_image(dimx, dimy, 1, n=2)
        Imov = np.where(np.isfinite(plant), Imov, plant)
    c, rc = o_force(Iref, Imov, u, 1.0, sigma_x)
    return Iref, Imov, u, c, rc


COMPOSE = [(s, k, kw) for s in SHAPES for k in KINDS for kw in (1, 3, 4)]


@functools.lru_cache(maxsize=None)
def compose_case(shape, kind, kw):
    """coord: the planted field is the correction (kw 1 smooths nothing, so
    the exact classes reach compose_px; kw 3 and 4 spread each NaN over up to
    9 / 16 coordinates); value: a finite correction samples a non-finite u.
    -> (corr, u, smoothed corr, out)."""
    dimx, dimy = shape
    if kind == "coord":
        corr, u = coord_motion(dimx, dimy, 2), finite_values(dimx, dimy, 7, 2)
    else:
        corr, u = value_motion(dimx, dimy), value_image(dimx, dimy, 2, 2)
    sm = o_smooth(corr, kw, 1.5)
    return corr, u, sm, o_accumulate(u, sm)


UPDATE = [(s, k) for s in UPDATE_SHAPES for k in ("u", "Imov")]


@functools.lru_cache(maxsize=None)
def update_case(shape, kind, kw):
    """u: the planted field is the motion (coordinates of warp_batch, values of
    compose_px); Imov: two non-finite pixels of the moving image make the
    correction NaN around them (coordinates of compose_px).
    -> (Iref, Imov, u, out)."""
    dimx, dimy = shape
    Iref, Imov = textured(dimx, dimy, 91)
    if kind == "u":
        u = coord_motion(dimx, dimy, 0)
    else:
        u = value_motion(dimx, dimy)
        plant = value_image(dimx, dimy, 0, n=2, nan=True)
        Imov = np.where(np.isfinite(plant), Imov, plant)
    c, rc = o_force(Iref, Imov, u, 1.0, 0.25)
    assert rc == 0
    return Iref, Imov, u, o_accumulate(u, o_smooth(c, kw, 1.5))


EXP = [(f, v, c) for f in ("above1", "below16") for v in ("nan", "inf") for c in (1, 0)]
EXP_NSQ = {"above1": 2, "below16": 5}
EXP_PIXEL = (4, 30)


def nsq_x86(f):
    """Motion.cpp:51-58 and :253-261 in float32: the running maximum `m < s`
    skips a NaN term; static_cast<int> of inf is INT_MIN (then clamped to 0)."""
    y = f[..., 1].astype(np.float64).reshape(-1)
    m = F(0)
    with np.errstate(all="ignore"):
        for s in (y * y + y * y).astype(F):
            m = s if m < s else m
        c = np.ceil(F(1) + np.log2(np.sqrt(m, dtype=F), dtype=F))
    n = int(c) if np.isfinite(c) and IMIN < c <= IMAX else IMIN
    return max(0, n)


@functools.lru_cache(maxsize=None)
def exp_case(field, value, comp):
    f = exp_field(field).copy()
    f[EXP_PIXEL][comp] = NAN if value == "nan" else INF
    want = f.copy()
    OL().oracle_motion_exp(want, f.shape[1], f.shape[0])
    f.setflags(write=False)
    return f, want


def planted_values(a, seed):
    """a with NaN, +inf, -inf planted on one word in 60 (at least one)."""
    a = a.copy()
    flat = a.reshape(-1)
    vals = [NAN, INF, -INF]
    n = max(1, flat.size // 60)
    for k in range(n):
        flat[(k * 61 + 7 * seed) % flat.size] = vals[(k + seed) % 3]
    return a


@functools.lru_cache(maxsize=None)
def resample_case(pair):
    """-> (img, mot, small, fills (image, motion, fine motion), wants)."""
    (dxi, dyi), (dxo, dyo) = pair
    L = OL()
    img = planted_values(finite_values(dxi, dyi, 21), 0)
    mot = planted_values(finite_values(dxi, dyi, 22, 2), 1)
    small = planted_values(finite_values(dxo, dyo, 25, 2), 2)
    fills = (finite_values(dxo, dyo, 23), finite_values(dxo, dyo, 24, 2),
             finite_values(dxi, dyi, 26, 2))
    wants = [f.copy() for f in fills]
    L.oracle_downsample_image(img, dxi, dyi, wants[0], dxo, dyo)
    L.oracle_downsample_motion(mot, dxi, dyi, wants[1], dxo, dyo)
    L.oracle_upsample_motion(small, dxo, dyo, wants[2], dxi, dyi)
    return img, mot, small, fills, wants


# ------------------------------------------------------------------ end to end
E2E_DIMS = (40, 24)
E2E_PIXEL = (20, 12)
HS = dict(niter=[3, 3, 3], nscales=2, reg=0, params=[0.3], nrefine=1)
E2E = {"hs-nan": (HS, np.nan, 1.0), "hs-inf": (HS, np.inf, 1.0),
       "thirion-nan": (dict(niter=[3], nscales=0, reg=3, params=[1.0, 0.25, 2.0, 2.0, 5, 0],
                            nrefine=1), np.nan, 1.0),
       "diffeomorphic-nan": (dict(niter=[3], nscales=0, reg=4, params=[1.0, 2.0, 1.0, 1.0, 5],
                                  nrefine=1), np.nan, 3.0)}


def e2e_pair(value, gain=1.0, seed=3):
    ref, mov = S.texture_pair(E2E_DIMS[0], seed=seed, ny=E2E_DIMS[1])
    mov = mov * gain
    if value is not None:
        mov[E2E_PIXEL] = value
    return ref, mov


def oracle_motion(O, cfg, ref, mov):
    o = O.Registration(E2E_DIMS, cfg["niter"], cfg["nscales"], cfg["reg"], cfg["params"],
                       cfg["nrefine"], 0, fixed_iters=True)
    try:
        o.register(ref, mov)
        return o.motion()
    finally:
        o.close()


_E2E = {}


def want_e2e(O, name):
    if name not in _E2E:
        cfg, value, gain = E2E[name]
        _E2E[name] = oracle_motion(O, cfg, *e2e_pair(value, gain))
    return _E2E[name]


BATCH_SEEDS = (5, 3, 6)  # the middle pair carries the NaN pixel


def batch_pairs():
    pairs = [e2e_pair(np.nan if k == 1 else None, 1.0, s) for k, s in enumerate(BATCH_SEEDS)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


# ------------------------------------------------------------------ CPU part
def test_inputs_reach_what_they_claim():
    """Every coordinate and value class is present at every shape with room
    and in the union over the small shapes."""
    union = {}
    for dimx, dimy in SHAPES:
        for seed in SEEDS:
            u = coord_motion(dimx, dimy, seed)
            got = {k: int(v.sum()) for k, v in coord_classes(u).items()}
            for k, v in got.items():
                union[k] = union.get(k, 0) + (v if (dimx, dimy) in SMALL else 0)
            if (dimx, dimy) in FULL:
                assert not [k for k, v in got.items() if v == 0], (dimx, dimy, seed, got)
                assert runs(u) == (1, 1), (dimx, dimy, runs(u))
                px, py = coordinates(u)
                assert np.isnan(px[0, 0]) and np.isnan(py[-1, -1])
                assert separating(u).sum() >= 64 + 4
            # the base field is sub-pixel: the planted pixels alone leave the grid far
            base = np.isfinite(u) & (np.abs(u) < 1e5)
            assert np.abs(u[base]).max(initial=0) < 1.0
    # 7 x 1 and 1 x 1 have one line: a y coordinate beside an in-range x needs
    # dimx > 1, so the union is taken over 3 x 3 and 7 x 1 (and 1 x 1 adds what it can)
    assert not [k for k, v in union.items() if v == 0], union
    for row0, nrows in WINDOWS:
        got = {k: int(v.sum()) for k, v in
               coord_classes(coord_motion(70, nrows, 3, row0, 37), row0, 37).items()}
        assert not [k for k, v in got.items() if v == 0], (row0, nrows, got)
    vunion = {}
    for shape in SHAPES:
        for seed in SEEDS:
            I, m, u = sampling_inputs(shape, "value", seed)
            assert np.isfinite(u).all() and np.abs(u).max() < 1.0
            for src in (I, m):
                got = value_classes(src, u)
                assert got["sampled"] > 0, (shape, seed)
                for k, v in got.items():
                    vunion[(shape in FULL, k)] = vunion.get((shape in FULL, k), 0) + v
                if shape in FULL:
                    # four plants, three values: each seed holds all of them
                    assert not [k for k, v in got.items() if v == 0], (shape, seed, got)
    assert not [k for k, v in vunion.items() if v == 0 and k != (False, "NaN")], vunion
    assert vunion[(False, "NaN")] == 0  # below 64 pixels: +-inf only (docstring)


def test_oracle_keeps_the_own_value(oracle):
    """Every pixel whose coordinate is NaN, inf or beyond int keeps its own
    value in the oracle's warp and accumulate, whatever the other component."""
    for shape in SHAPES:
        for seed in SEEDS:
            I, m, u = sampling_inputs(shape, "coord", seed)
            px, py = coordinates(u)
            with np.errstate(invalid="ignore"):
                # (2^31 - 128 and -2^31 are valid ints, far outside every grid here)
                out = ~(np.abs(px) < F(2.0 ** 30)) | ~(np.abs(py) < F(2.0 ** 30))
            assert out.sum() >= 1
            w, a = want_warp(shape, "coord", seed), want_accumulate(shape, "coord", seed)
            assert np.array_equal(w.view(np.uint32)[out], I.view(np.uint32)[out]), (shape, seed)
            assert np.array_equal(a.view(np.uint32)[out], m.view(np.uint32)[out]), (shape, seed)
            # coordinate classes put no NaN into the oracle's output at all
            assert not np.isnan(w).any() and not np.isnan(a).any()


def test_restatement_separates_the_conversions(oracle):
    """x86 rule: the numpy restatement is the oracle on the bits.  Device rule
    (NaN -> 0): it differs from the oracle on every input with a separating
    pixel, so a kernel with the bare conversion fails on each of them."""
    nsep = 0
    for case in SAMPLING:
        I, m, u = sampling_inputs(*case)
        assert_bits(r_warp(I, u, "x86"), want_warp(*case), f"warp {sid(case)}")
        assert_bits(r_accumulate(m, u, "x86"), want_accumulate(*case), f"accumulate {sid(case)}")
        if case[1] == "coord" and (separating(u).any() or case[0] in FULL):
            nsep += 1
            for got, want in ((r_warp(I, u, "device"), want_warp(*case)),
                              (r_accumulate(m, u, "device"), want_accumulate(*case))):
                assert (np.isnan(got) != np.isnan(want)).any(), case
        else:
            # finite coordinates: the two rules agree
            assert_bits(r_warp(I, u, "device"), want_warp(*case), f"warp {sid(case)}")
    # every seed of the larger shapes, and most of the small ones (a 1 x 1
    # grid holds one plant, which is not always a NaN)
    assert nsep >= len(SEEDS) * (len(SHAPES) - 1)
    for case in REGRID:
        m_old, est, I, m_new, Iaux = regrid_case(*case)
        assert_bits(r_accumulate(m_old, est, "x86"), m_new, f"regrid {case}")
        assert_bits(r_warp(I, m_new, "x86"), Iaux, f"regrid Iaux {case}")
        if case[1] == "est" and separating(est).any():
            assert (np.isnan(r_accumulate(m_old, est, "device")) != np.isnan(m_new)).any(), case
        if case[1] == "old":
            assert separating(m_new).any(), case
            assert (np.isnan(r_warp(I, m_new, "device")) != np.isnan(Iaux)).any(), case
    for window in WINDOWS:
        full, want = window_case(window)
        row0, nrows = window
        v = full[row0:row0 + nrows]
        zero = np.zeros_like(full)
        assert_bits(r_accumulate(zero, v, "x86", row0), want, f"window {window}")
        assert separating(v, row0, 37).any()
        assert (np.isnan(r_accumulate(zero, v, "device", row0)) != np.isnan(want)).any()
    for case in COMPOSE:
        corr, u, sm, want = compose_case(*case)
        assert_bits(r_accumulate(u, sm, "x86"), want, f"compose {case}")
        if case[1] == "coord" and (separating(sm).any() or case[0] in FULL):
            assert (np.isnan(r_accumulate(u, sm, "device")) != np.isnan(want)).any(), case


def test_no_case_hides_behind_nan(oracle):
    """At most 25 % of the oracle's output words are NaN in every case that
    the GPU part compares."""
    for case in SAMPLING:
        under_cap(f"warp {sid(case)}", want_warp(*case))
        under_cap(f"accumulate {sid(case)}", want_accumulate(*case))
    for case in REGRID:
        _, _, _, m_new, Iaux = regrid_case(*case)
        under_cap(f"regrid {case} motion", m_new)
        under_cap(f"regrid {case} Iaux", Iaux)
    for shape in SHAPES:
        v = coord_motion(*shape, 1)
        assert not np.isnan(o_accumulate(np.zeros_like(v), v)).any()
    for window in WINDOWS:
        assert not np.isnan(window_case(window)[1]).any()
    for case in FORCE:
        under_cap(f"force {case}", force_case(*case)[3])
    for case in COMPOSE:
        under_cap(f"compose {case}", compose_case(*case)[3])
    for case in UPDATE:
        for kw in (3, 5):
            under_cap(f"update {case} kw {kw}", update_case(*case, kw)[3])
    for case in EXP:
        f, want = exp_case(*case)
        under_cap(f"exp {case}", want)
        assert not np.array_equal(np.isnan(want), np.ones(want.shape, bool))
    for pair in PAIRS:
        for k, w in enumerate(resample_case(pair)[4]):
            under_cap(f"resample {pair} output {k}", w)
    for name in E2E:
        m = want_e2e(oracle, name)
        under_cap(f"end to end {name}", m)
        assert m.any(), name
    refs, movs = batch_pairs()
    for k in range(3):
        under_cap(f"batch pair {k}", oracle_motion(oracle, HS, refs[k], movs[k]))


def test_exp_counts(oracle):
    """A NaN term is skipped by the reference's running maximum; an inf in .y
    makes the count INT_MIN, clamped to 0; .x is not looked at."""
    for field, value, comp in EXP:
        f, _ = exp_case(field, value, comp)
        want = 0 if (value, comp) == ("inf", 1) else EXP_NSQ[field]
        assert nsq_x86(f) == want, (field, value, comp)
        assert nsq_x86(exp_field(field)) == EXP_NSQ[field]


# ------------------------------------------------------------------ GPU: primitives
@gpu_test
@pytest.mark.parametrize("case", SAMPLING, ids=sid)
def test_warp(gpu, oracle, case):
    I, _, u = sampling_inputs(*case)
    assert_bits(prim.warp(I, u), want_warp(*case), f"warp {sid(case)}")


@gpu_test
@pytest.mark.parametrize("case", SAMPLING, ids=sid)
def test_accumulate(gpu, oracle, case):
    """accumulate_px already converts through floor_int: a regression test."""
    _, m, u = sampling_inputs(*case)
    assert_bits(prim.accumulate(m, u), want_accumulate(*case), f"accumulate {sid(case)}")


@gpu_test
@pytest.mark.parametrize("case", REGRID, ids=sid)
def test_regrid(gpu, oracle, case):
    m_old, est, I, want_m, want_I = regrid_case(*case)
    m_new, est0, Iaux = prim.regrid(m_old, est, I)
    assert_bits(m_new, want_m, f"regrid motion {case}")
    assert_bits(est0, np.zeros_like(est0), f"regrid zeroed estimate {case}")
    assert_bits(Iaux, want_I, f"regrid Iaux {case}")


@gpu_test
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_compose_zero(gpu, oracle, shape):
    v = coord_motion(*shape, 1)
    assert_bits(prim.compose_zero(v), o_accumulate(np.zeros_like(v), v), f"compose_zero {shape}")


@gpu_test
@pytest.mark.parametrize("window", WINDOWS, ids=ids)
def test_compose_zero_row_window(gpu, oracle, window):
    row0, nrows = window
    full, want = window_case(window)
    assert_bits(prim.compose_zero(full[row0:row0 + nrows], row0, 37), want,
                f"compose_zero window {window}")


@gpu_test
@pytest.mark.parametrize("case", FORCE, ids=lambda c: f"{ids(c[0])}-{c[1]}")
def test_demons_force(gpu, oracle, case):
    Iref, Imov, u, want, rc = force_case(*case)
    got, status = prim.demons_force(Iref, Imov, u, 1.0, 0.25)
    assert (rc != 0) == bool(status & 1) and (status & ~1) == 0, (rc, status)
    assert_bits(got, want, f"demons force {case}")


@gpu_test
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("case", COMPOSE, ids=lambda c: f"{ids(c[0])}-{c[1]}-kw{c[2]}")
def test_smooth_compose(gpu, oracle, case, method):
    shape, kind, kw = case
    corr, u, sm, want = compose_case(*case)
    got, _, path = prim.smooth_compose(corr, u, kw, 1.5, 0, method=method)
    assert path == int(method == 1 and kw == 3 and shape[0] >= kw), (case, method, path)
    if path:
        # the separable kernels' own smoothed correction (module docstring)
        sm, _, p3 = prim.smooth_compose(corr, u, kw, 1.5, 3, method=1)
        assert p3 == 1
        want = o_accumulate(u, sm)
        under_cap(f"separable compose {case}", want)
    assert_bits(got, want, f"smooth_compose {case} method {method}")


@gpu_test
@pytest.mark.parametrize("case", UPDATE, ids=lambda c: f"{ids(c[0])}-{c[1]}")
def test_demons_update(gpu, oracle, case):
    """(127, 31): the unfused pair of kernels; (129, 33): the fused one."""
    for kw in (3, 5):
        Iref, Imov, u, want = update_case(*case, kw)
        got, status = prim.demons_update(Iref, Imov, u, 1.0, 0.25, kw, 1.5, 0)
        assert status == 0
        assert_bits(got, want, f"demons_update {case} kw {kw}")


@gpu_test
@pytest.mark.parametrize("case", EXP, ids=lambda c: f"{c[0]}-{c[1]}-{'xy'[c[2]]}")
def test_motion_exp(gpu, oracle, case):
    f, want = exp_case(*case)
    got, nsq, status = prim.motion_exp(f)
    assert nsq == nsq_x86(f) and status == 0
    assert_bits(got, want, f"exp {case}")


@gpu_test
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{ids(p[0])}-{ids(p[1])}")
def test_resample(gpu, oracle, pair):
    img, mot, small, fills, wants = resample_case(pair)
    assert_bits(prim.downsample_image(img, fills[0]), wants[0], "downsample image")
    assert_bits(prim.downsample_motion(mot, fills[1]), wants[1], "downsample motion")
    assert_bits(prim.upsample_motion(small, fills[2]), wants[2], "upsample motion")


# ------------------------------------------------------------------ GPU: end to end
@gpu_test
@pytest.mark.parametrize("name", list(E2E))
def test_registration(gpu, oracle, name):
    from opticalflow2d_amd import ImageRegistration
    cfg, value, gain = E2E[name]
    ref, mov = e2e_pair(value, gain)
    with ImageRegistration(E2E_DIMS, cfg["niter"], cfg["nscales"], cfg["reg"], cfg["params"],
                           cfg["nrefine"], fixed_iters=1) as r:
        r.register(ref, mov)
        assert r.iterations() == cfg["niter"]
        got = r.motion()
    assert_bits(got, want_e2e(oracle, name), f"{name}: motion")


@gpu_test
def test_batch_with_one_nan_pair(gpu, oracle):
    from test_gpu_batch import run_batch
    refs, movs = batch_pairs()
    got = run_batch(E2E_DIMS, HS["niter"], HS["nscales"], HS["params"][0], HS["nrefine"], refs, movs,
                    fixed_iters=1)
    assert got["status"].tolist() == [0, 0, 0] and got["error"] == ""
    for k in range(3):
        assert_bits(got["motion"][k], oracle_motion(oracle, HS, refs[k], movs[k]), f"pair {k}")
    for k in (0, 2):
        solo = run_batch(E2E_DIMS, HS["niter"], HS["nscales"], HS["params"][0], HS["nrefine"],
                         refs[k:k + 1], movs[k:k + 1], fixed_iters=1)
        assert not np.isnan(solo["motion"][0]).any()
        assert np.array_equal(solo["motion"][0].view(np.uint64),
                              got["motion"][k].view(np.uint64)), f"pair {k} against its solo run"
