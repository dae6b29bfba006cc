"""The two division sequences of the fused Horn-Schunck kernels at the corners
of their range, above it and on non-finite input, against the oracle.

hs::div2_unscaled (hs_jacobi_impl.h) stands in for the compiler's IEEE division
where its header comment argues the two give the same bits: every gradient 0 or
in [2^-30, 2^20), the denominator (alpha^2 + gx^2) + gy^2 in [2^-40, 2^40)
(hs_precheck_kernel's word per field, "the flag" below: 0 in range, 1 not) and
|sc| in [2^-50, 2^30) on every lane of a wave's row step (the ballot of the
triple and of the quad; sc == 0 takes the IEEE sequence).  The tests of
test_gpu_hs.py and test_gpu_hs_quad.py reach only the low end of these ranges;
this file holds the high end, the exact corner values, single lanes out of
range, overflow, NaN / inf pixels and underflowing squares.

Bar: no tolerance.  The motion equals the oracle's on the float32 bits, signs
of zero included; where the oracle's motion holds NaN the NaN masks are equal
and every other element equal on the bits (NaN payloads differ between x86 and
the GPU, as tests/test_gpu_seqnorm.py allows).  No case may hide behind NaN:
the returned motion is the iterate composed onto the zero motion, which is 0
where the iterate is NaN or points outside the image, and the CPU part asserts
that at most half of the pixels are hidden in that way for every case and
iteration count used here, and that cases 1 to 6 have no NaN in the iterate.

Geometry the inputs are laid out for (257 x 151, of2d_device.h hs3_rows): a
wave's row step covers the 128 px of strip b, x in [120 b - 4, 120 b + 124),
and a wave marches 4 j-lines ("row band": j-lines 4 k .. 4 k + 3, odd waves
upward).  The third strip reaches into the pitch padding, where It = 0, so its
row steps always take the IEEE sequence; strips 0 and 1 take the unscaled
sequence whenever the flag is 0 and every lane's sc is in range.  The CPU part
restates the precheck predicate and the first iteration's ballot (q = 0, so
sc = It) in numpy on the oracle's dI and It and asserts the class each case
is meant to be in.  It = Imov - Iref (IterativeSolver.cpp:22-56), and the
gradients are the moving image's alone.

Exact gradients.  A central difference over a ramp whose slope changes from s1
to s2 gives (s1 + s2) / 2 on the joint, which for the band of slope 2^-30
would lie below the bound and set the flag by itself.  The corner inputs
therefore use the shortest piecewise-linear profile whose central differences
are exactly +s, 0, -s and nothing else ("lattice" below): period 4, values
0, 0, 2 s, 0, so that the pixel before a peak has the neighbours 0 and 2 s
(gradient +s), the one after it 2 s and 0 (-s), and the peak and the pixel two
from it equal neighbours (0).  2 s is a float32 whenever s is, so the values
are exact for slopes such as 2^20 minus one ulp, for which s * x is not.  Bands
of different slopes (20 px wide, starting where the profile is 0) join without
any intermediate value.

The cases (name: what, flag):
  1 high       texture x 2^24: some gradients >= 2^20, not all.  Flag 1.
  2 sc         texture, ref + 2^32 x Gaussian bump: |It| from 2^-10 to 2^32.
               Flag 0; the ballot trips in the row steps that cross the bump.
  3 lane       texture; 15 single pixels with It = 2^31, It = 0 (ref == mov
               there) or It = 2^-60 (mov = 0 there), each kind at x = 116 (lane
               0 of strip 1), x = 243 (lane 63 of strip 1), x = 256 (the odd
               last column), in the first j-line of a row band (x = 60) and in
               the last (x = 180).  Flag 0, every other sc in range.
  4a/4b/4c     lattice bands of 20 px cycling through the slopes 0, 2^-30,
  (+ y)        2^20 - ulp (4a: flag 0), the same and 2^-30 - ulp (4b: flag 1),
               the same and 2^20 (4c: flag 1).  The issue's wording "the three
               below 2^20 give flag 0" is read as the three values inside
               [2^-30, 2^20) or 0.  Band k (x // 20 = k, or y // 20 with
               "y") carries slope number k mod (number of slopes).  It is 0.5,
               0.75, 1 or 1.25.  The "y" variants put the profile along y, so
               gy carries the values and gx is 0.
  5a .. 5d     texture with a flat band (x in [40, 60), gradient 0, so the
               denominator is alpha^2 alone there) at alpha = 2^-20 (5a, flag
               0), the float below (5b, flag 1), 2^20 - ulp (5c, flag 0) and
               2^20 (5d, flag 1).
  6 sc corner  lattice bands along x cycling through the slopes 2^-30, 0.25,
               2^-29, 2^20 - ulp; It constant on row bands of 19 j-lines cycling
               through 2^-50, 2^-50 - ulp, 2^30 - ulp, 2^30 (j // 19 = k carries
               value number k mod 4) on every pixel with a non-zero gradient
               (the peaks, whose gradient is 0, carry 1.0 in the low bands).
               Flag 0.  Row steps of the first and third value pass the
               ballot in strips 0 and 1, those of the second and fourth trip
               it.  The numerators reach 2^-80 exactly and (2^20 - ulp) x
               (2^30 - ulp); the motion of the latter points outside the image
               and is returned as 0, that of the slopes 2^-30 and 2^-29 beside
               It = 2^30 stays visible.
  7a overflow  texture with a patch (x in [40, 100), j-lines 40..55) that is a
               lattice along y of slope 1e20: gy^2 and the denominator are inf,
               the quotients 0; two pixels with It = 1e20 have inf / inf = NaN,
               and so has every pixel of the patch once q.y * gy * gy
               overflows.  Flag 1.
  7b overflow  texture with j-lines 60..67 alternating +3e38, 0, -3e38, 0: the
               differences themselves overflow, gy = -+inf.  Flag 1 (the
               joints with the texture have finite gradients ~1.5e38).
  8 nan / inf  texture with one NaN (8n) or +inf (8i) pixel in the moving image
               at (60, 75) (inside strip 0) or at (0, 75) (x = 0); 8n-seam: NaN
               at (60, 79), the fourth j-line below rank 0 of two.  NaN and inf
               have frexp exponent 0, so the flag stays 0 and the unscaled
               sequence sees the non-finite operands.
  9 underflow  moving image ~1e-25, It ~ 0.01: the squares underflow and the
               denominator is alpha^2 (alpha 0.3, flag 1).  9z: alpha = 0, the
               denominator is exactly 0 on pixels with a gradient and the
               reference throws "Divide by zero exception".
"""
import functools

import numpy as np
import pytest

from opticalflow2d_amd import synthetic as S

F = np.float32
DIMS = (257, 151)
NX, NY = DIMS
ITERS = [1, 2, 3, 4, 13]  # single step, pair, triple, quad, mixed
CONV_CAP = 40
STRIP = 120               # of2d_device.h kHs3Out
BAND = 4                  # hs3_rows(257, 151)
LO_G, HI_G = F(2.0 ** -30), F(2.0 ** 20)
LO_SC, HI_SC = F(2.0 ** -50), F(2.0 ** 30)


def below(v):
    return np.nextafter(F(v), F(0))


# ------------------------------------------------------------------ inputs
def tex():
    """The textured pair in float32, with It != 0 on every pixel (the clamped
    shift leaves the corner pixel (0, 150) equal in both images)."""
    r, m = S.texture_pair(NX, seed=21, ny=NY)
    r, m = r.astype(F), m.astype(F)
    r[r == m] += F(2.0 ** -10)
    return r, m


def lattice(n, slopes, width=20):
    """The period-4 profile of the module docstring along n pixels, band k of
    `width` px with slope slopes[k % len(slopes)].  No peak on the last pixel,
    whose one-sided difference would be 2 s."""
    v = np.zeros(n, F)
    for k in range(n - 1):
        if k % 4 == 2:
            v[k] = F(2) * F(slopes[(k // width) % len(slopes)])
    return v


S4 = {"4a": [0.0, LO_G, below(HI_G)],
      "4b": [0.0, LO_G, below(HI_G), below(LO_G)],
      "4c": [0.0, LO_G, below(HI_G), HI_G]}
A5 = {"5a": F(2.0 ** -20), "5b": below(2.0 ** -20), "5c": below(2.0 ** 20), "5d": F(2.0 ** 20)}
S6 = [LO_G, 0.25, F(2.0 ** -29), below(HI_G)]
V6 = [LO_SC, below(LO_SC), below(HI_SC), HI_SC]
ROWS6 = 19
# case 3: (x, j, kind); j % 4 is 1 for the three column positions, 0 for the
# first and 3 for the last j-line of a row band
PLANTED = ([(116, j, k) for j, k in ((9, "big"), (21, "zero"), (33, "tiny"))] +
           [(243, j, k) for j, k in ((45, "big"), (57, "zero"), (69, "tiny"))] +
           [(256, j, k) for j, k in ((81, "big"), (93, "zero"), (105, "tiny"))] +
           [(60, j, k) for j, k in ((112, "big"), (124, "zero"), (132, "tiny"))] +
           [(180, j, k) for j, k in ((119, "big"), (127, "zero"), (135, "tiny"))])
# (value, x, j); "seam": j-line 79 is row_end + 3 of rank 0 of two (151 j-lines:
# 76 + 75), so the warp by the zero motion carries it into rank 0's last image
# halo row from the fourth row below the slab
NONFINITE = {"8n-in": (np.nan, 60, 75), "8n-x0": (np.nan, 0, 75), "8i-in": (np.inf, 60, 75),
             "8i-x0": (np.inf, 0, 75), "8n-seam": (np.nan, 60, 79)}

NAMES = (["1", "2", "3"] + [k + o for k in S4 for o in ("", "y")] + list(A5) + ["6", "7a", "7b"] +
         list(NONFINITE) + ["9"])
NO_NAN = [n for n in NAMES if n[0] in "123456"]
# the flag hs_precheck_kernel must compute
FLAG = {"1": 1, "2": 0, "3": 0, "4a": 0, "4ay": 0, "4b": 1, "4by": 1, "4c": 1, "4cy": 1,
        "5a": 0, "5b": 1, "5c": 0, "5d": 1, "6": 0, "7a": 1, "7b": 1, "8n-in": 0, "8n-x0": 0,
        "8i-in": 0, "8i-x0": 0, "8n-seam": 0, "9": 1, "9z": 1}


@functools.lru_cache(maxsize=None)
def case(name):
    """(ref, mov, alpha): float64 images [257, 151] holding float32 values."""
    alpha = 0.3
    x = np.arange(NX)[:, None]
    y = np.arange(NY)[None, :]
    with np.errstate(all="ignore"):
        if name == "1":
            r, m = tex()
            ref, mov = r * F(2.0 ** 24), m * F(2.0 ** 24)
        elif name == "2":
            ref, mov = tex()
            bump = np.exp(-((x - 70.0) ** 2 + (y - 60.0) ** 2) / (2 * 12.0 ** 2))
            ref = ref + (2.0 ** 32 * bump).astype(F)
        elif name == "3":
            ref, mov = tex()
            for px, j, kind in PLANTED:
                if kind == "big":
                    ref[px, j] = mov[px, j] - F(2.0 ** 31)
                elif kind == "zero":
                    ref[px, j] = mov[px, j]
                else:
                    mov[px, j] = 0
                    ref[px, j] = -F(2.0 ** -60)
        elif name[0] == "4":
            along_y = name.endswith("y")
            v = lattice(NY if along_y else NX, S4[name[:2]])
            mov = np.broadcast_to(v[None, :] if along_y else v[:, None], DIMS).astype(F)
            it = (F(0.5) + F(0.25) * ((x + 2 * y) % 4)).astype(F)
            ref = mov - it
        elif name[0] == "5":
            ref, mov = tex()
            mov[40:60, :] = 0.5
            alpha = float(A5[name])
        elif name == "6":
            mov = np.broadcast_to(lattice(NX, S6)[:, None], DIMS).astype(F)
            v = np.array(V6, F)[(np.arange(NY) // ROWS6) % 4]
            low = ((np.arange(NY) // ROWS6) % 4) < 2
            it = np.broadcast_to(v[None, :], DIMS).astype(F)
            peak = (mov != 0) & low[None, :]
            it[peak] = 1.0
            ref = mov - it
        elif name == "7a":
            ref, mov = tex()
            mov[40:100, 40:56] = lattice(16, [F(1e20)])[None, :]
            ref[40:100, 40:56] = mov[40:100, 40:56] - F(1.0)
            ref[60, 45] = -F(1e20)
            ref[80, 51] = -F(1e20)
        elif name == "7b":
            ref, mov = tex()
            mov[:, 60:68] = (np.array([1, 0, -1, 0, 1, 0, -1, 0], F) * F(3e38))[None, :]
        elif name in NONFINITE:
            ref, mov = tex()
            val, px, j = NONFINITE[name]
            mov[px, j] = val
        elif name in ("9", "9z"):
            r, m = tex()
            mov = m * F(1e-25)
            ref = mov + F(0.125) * (r - m)
            alpha = 0.3 if name == "9" else 0.0
        else:
            raise KeyError(name)
    ref = np.ascontiguousarray(ref, F).astype(np.float64)
    mov = np.ascontiguousarray(mov, F).astype(np.float64)
    ref.setflags(write=False)
    mov.setflags(write=False)
    return ref, mov, alpha


# ------------------------------------------------------------------ oracle
def derivatives(oracle, ref, mov):
    """The oracle's (gx, gy, It) as [dimx, dimy] float32 arrays."""
    L = oracle.lib()
    nx, ny = ref.shape
    Im = np.ascontiguousarray(mov.reshape(-1, order="F").astype(F))
    Ir = np.ascontiguousarray(ref.reshape(-1, order="F").astype(F))
    dI = np.zeros(2 * nx * ny, F)
    It = np.zeros(nx * ny, F)
    L.oracle_spatial_derivative(Im, nx, ny, dI)
    L.oracle_temporal_derivative(Ir, Im, nx * ny, It)
    g = dI.reshape(ny, nx, 2)
    return g[:, :, 0].T.copy(), g[:, :, 1].T.copy(), It.reshape(ny, nx).T.copy()


def exp_in(v, lo, hi):
    """hs::exp_in: the frexp exponent within [lo, hi]; 0, inf and NaN have 0."""
    v = np.asarray(v, F)
    _, e = np.frexp(v)
    e = np.where(np.isfinite(v) & (v != 0), e, 0)
    return (e >= lo) & (e <= hi)


def denominator(gx, gy, alpha):
    a = F(alpha)
    with np.errstate(all="ignore"):
        return ((a * a + gx * gx) + gy * gy).astype(F)


def precheck_flag(gx, gy, alpha):
    """hs_precheck_kernel on the image pixels and on one padding pixel (zero
    gradient: the denominator is alpha^2)."""
    a = F(alpha)
    den = denominator(gx, gy, alpha)
    ok = exp_in(gx, -29, 20) & exp_in(gy, -29, 20) & exp_in(den, -39, 40)
    return int(not (ok.all() and exp_in(a * a, -39, 40)))


def sc_ok(It):
    a = np.abs(It)
    return (a >= LO_SC) & (a < HI_SC)  # NaN: false here; the kernel's min/max drop a NaN


def steps_ok(It):
    """[2, dimy]: the first iteration's ballot passes in the row step of strips
    0 and 1 at j-line j (every lane's sc = It in range)."""
    ok = sc_ok(It)
    out = np.zeros((2, NY), bool)
    for b in range(2):
        lo, hi = max(STRIP * b - 4, 0), STRIP * b + 124
        assert hi <= NX
        out[b] = ok[lo:hi].all(axis=0)
    return out


def oracle_fixed(oracle, ref, mov, alpha, iters):
    r = oracle.Registration(ref.shape, [iters], 0, 0, [alpha], 1, 0, fixed_iters=True)
    try:
        r.register(ref, mov)
        return r.motion()
    finally:
        r.close()


_WANT = {}


def want(oracle, name, iters):
    """The oracle's motion of a case after `iters` fixed iterations, once."""
    key = (name, iters)
    if key not in _WANT:
        _WANT[key] = oracle_fixed(oracle, *case(name), iters)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def want_conv(oracle, name):
    """The oracle's convergence-on run (cap 40): motion, iterations, errors."""
    key = (name, "conv")
    if key not in _WANT:
        ref, mov, alpha = case(name)
        r = oracle.Registration(DIMS, [CONV_CAP], 0, 0, [alpha], 1, 0)
        try:
            r.register(ref, mov)
            _WANT[key] = (r.motion(), r.iterations(), r.last_errors())
        finally:
            r.close()
    return _WANT[key]


def bits(a):
    return np.asarray(a, dtype=F).view(np.uint32)


def assert_bits(got, expect, what):
    """Equal NaN masks, and equal float32 bits everywhere else."""
    g, w = np.asarray(got, F), np.asarray(expect, F)
    assert g.shape == w.shape, what
    gn, wn = np.isnan(g), np.isnan(w)
    assert np.array_equal(gn, wn), f"{what}: {int((gn != wn).sum())} NaN positions differ"
    diff = (bits(g) != bits(w)) & ~wn
    assert not diff.any(), (f"{what}: {int(diff.sum())} elements differ, first at "
                            f"{tuple(np.argwhere(diff)[0])}")


# ------------------------------------------------------------------ CPU part
def test_inputs_reach_what_they_claim(oracle):
    """Runs without a GPU: flag, both sides of each bound, the exact corner
    values, in float32 as the kernels compute them."""
    d = {n: derivatives(oracle, *case(n)[:2]) for n in NAMES + ["9z"]}
    for n in NAMES + ["9z"]:
        gx, gy, _ = d[n]
        assert precheck_flag(gx, gy, case(n)[2]) == FLAG[n], n
    inr = lambda g: (g == 0) | ((np.abs(g) >= LO_G) & (np.abs(g) < HI_G))

    # 1: some gradients at or above 2^20, not all; nothing else out of range
    gx, gy, It = d["1"]
    hi = (np.abs(gx) >= HI_G) | (np.abs(gy) >= HI_G)
    assert 100 < hi.sum() < hi.size // 2
    assert (inr(gx) | (np.abs(gx) >= HI_G)).all() and (inr(gy) | (np.abs(gy) >= HI_G)).all()

    # 2: |It| on both sides of 2^30; most row steps of strips 0 and 1 pass the
    # ballot, those that cross the bump trip it
    gx, gy, It = d["2"]
    assert (np.abs(It) >= HI_SC).sum() > 100 and (np.abs(It) < HI_SC).sum() > 100
    ok = steps_ok(It)
    assert ok.sum() > ok.size // 2 and (~ok).sum() >= 30
    assert ok[:, :30].all() and not ok[0, 60]

    # 3: exactly the planted pixels are out of range, each alone in its row step
    gx, gy, It = d["3"]
    bad = ~sc_ok(It)
    planted = np.zeros(DIMS, bool)
    for px, j, kind in PLANTED:
        planted[px, j] = True
        v = It[px, j]
        assert {"big": v == F(2.0 ** 31), "zero": v == 0, "tiny": v == F(2.0 ** -60)}[kind]
    assert np.array_equal(bad, planted)
    assert bad.sum(axis=0).max() == 1 and len(PLANTED) == 15
    assert sorted({j % BAND for px, j, _ in PLANTED if px in (116, 243, 256)}) == [1]
    assert {j % BAND for px, j, _ in PLANTED if px == 60} == {0}
    assert {j % BAND for px, j, _ in PLANTED if px == 180} == {BAND - 1}
    assert 116 == STRIP - 4 and 243 == STRIP + 123 and 256 == NX - 1 and NX % 2 == 1
    assert {(j // BAND) % 2 for _, j, _ in PLANTED} == {0, 1}  # both march directions

    # 4: the gradient values are exactly the slopes, both signs, and 0
    for n, slopes in S4.items():
        vals = sorted({float(s) for s in slopes} | {-float(s) for s in slopes})
        gx, gy, It = d[n]
        assert sorted(set(gx.ravel().astype(float))) == vals, n
        assert not gy.any() and sc_ok(It).all()
        gx, gy, It = d[n + "y"]
        assert sorted(set(gy.ravel().astype(float))) == vals, n
        assert not gx.any() and sc_ok(It).all()
        # every band is wider than 4 px and carries its slope
        for k in range(NX // 20):
            band = np.abs(d[n][0][20 * k:20 * k + 20, 7])
            assert set(band.tolist()) == {0.0, float(slopes[k % len(slopes)])}
    assert float(LO_G) == 2.0 ** -30 and float(below(LO_G)) == 2.0 ** -30 - 2.0 ** -54
    assert float(HI_G) == 2.0 ** 20 and float(below(HI_G)) == 2.0 ** 20 - 2.0 ** -4
    assert inr(d["4a"][0]).all() and not inr(d["4b"][0]).all() and not inr(d["4c"][0]).all()
    assert (np.abs(d["4b"][0])[~inr(d["4b"][0])] == below(LO_G)).all()
    assert (np.abs(d["4c"][0])[~inr(d["4c"][0])] == HI_G).all()

    # 5: alpha^2 alone on the flat band, its side of the bound; gradients
    # in range elsewhere
    for n, a in A5.items():
        gx, gy, It = d[n]
        asq = a * a
        den = denominator(gx, gy, a)
        flat = np.zeros(DIMS, bool)
        flat[41:59, :] = True
        assert not gx[flat].any() and not gy[flat].any() and (den[flat] == asq).all(), n
        assert inr(gx).all() and inr(gy).all() and (gx != 0).sum() > NX * NY // 2
        assert exp_in(asq, -39, 40) == (FLAG[n] == 0), n
        assert sc_ok(It[flat]).all()
    assert float(A5["5a"] * A5["5a"]) == 2.0 ** -40
    assert float(A5["5b"] * A5["5b"]) < 2.0 ** -40
    assert float(A5["5c"] * A5["5c"]) == 2.0 ** 40 - 2.0 ** 17
    assert float(A5["5d"] * A5["5d"]) == 2.0 ** 40
    # 5b: the flat band is below the bound, textured pixels are above it
    den = denominator(d["5b"][0], d["5b"][1], A5["5b"])
    assert (den < F(2.0 ** -40)).any() and exp_in(den, -39, 40).sum() > NX * NY // 2
    assert exp_in(denominator(d["5c"][0], d["5c"][1], A5["5c"]), -39, 40).all()

    # 6: It holds the four values exactly on every pixel with a gradient; the
    # row steps of the in-range values pass the ballot, the others trip it
    gx, gy, It = d["6"]
    assert sorted(set(np.abs(gx).ravel().astype(float))) == sorted({0.0} | {float(s) for s in S6})
    ok = steps_ok(It)
    for j in range(NY):
        k = (j // ROWS6) % 4
        assert (It[gx[:, j] != 0, j] == V6[k]).all(), j
        assert ok[:, j].all() == (k in (0, 2)) and ok[:, j].any() == (k in (0, 2)), j
    assert {(j // ROWS6) % 4 for j in range(NY)} == {0, 1, 2, 3}
    assert float(V6[0]) == 2.0 ** -50 and float(V6[1]) == 2.0 ** -50 - 2.0 ** -74
    assert float(V6[2]) == 2.0 ** 30 - 64 and float(V6[3]) == 2.0 ** 30
    # the numerators gx * sc reach both ends of the comment's range
    num = np.abs(gx[:, :ROWS6] * It[:, :ROWS6])
    assert num[num != 0].min() == F(2.0 ** -80)
    num = np.abs(gx[:, 2 * ROWS6:3 * ROWS6] * It[:, 2 * ROWS6:3 * ROWS6])
    assert num.max() == below(HI_G) * below(HI_SC) and num.max() < F(2.0 ** 50)

    # 7: inf squares and denominators beside finite ones; 7b: inf gradients
    np.seterr(over="ignore")
    gx, gy, It = d["7a"]
    den = denominator(gx, gy, 0.3)
    assert np.isinf(den).sum() > 400 and np.isfinite(den).sum() > NX * NY // 2
    assert np.isfinite(gy).all() and np.abs(gy).max() == F(1e20)
    assert It[60, 45] == F(1e20) and It[80, 51] == F(1e20) and np.isinf(den[60, 45])
    assert np.isinf(np.multiply(gy, It, dtype=F)[60, 45])  # inf / inf
    gx, gy, It = d["7b"]
    assert np.isinf(gy).sum() == 3 * NX and not np.isnan(gy).any()
    assert np.isfinite(gx).all()

    # 8: the pixel and its gradient neighbours
    for n, (val, px, j) in NONFINITE.items():
        gx, gy, It = d[n]
        nonfin = ~np.isfinite(gx) | ~np.isfinite(gy) | ~np.isfinite(It)
        assert nonfin.sum() == (5 if px else 4), n
        assert not np.isfinite(It[px, j]) and not np.isfinite(gy[px, j - 1])
    from opticalflow2d_amd.slab import halo_rows
    assert halo_rows(NY, 0, 2) == (0, 80) and NONFINITE["8n-seam"][2] == 79

    # 9: the squares underflow: the denominator is alpha^2 on every pixel,
    # exactly 0 with alpha = 0 on pixels whose gradient is not
    gx, gy, It = d["9"]
    assert (gx != 0).sum() > NX * NY // 2 and np.abs(gx).max() < LO_G
    assert (denominator(gx, gy, 0.3) == F(0.3) * F(0.3)).all()
    assert not denominator(gx, gy, 0.0).any()
    assert 1e-4 < np.abs(It).max() < 1.0


def oracle_iterate(oracle, name, iters):
    """The iterate u after `iters` updates, before the registration composes it
    onto the zero motion: [dimx, dimy, 2] float32."""
    ref, mov, alpha = case(name)
    gx, gy, It = derivatives(oracle, ref, mov)
    dI = np.ascontiguousarray(np.stack([gx.T, gy.T], axis=2).reshape(-1))
    u = np.zeros(2 * NX * NY, F)
    errs = np.zeros(iters, F)
    assert oracle.lib().oracle_hs_loop(u, dI, np.ascontiguousarray(It.T.reshape(-1)), NX, NY,
                                       alpha, iters, 1, errs) == iters
    return u.reshape(NY, NX, 2).transpose(1, 0, 2)


def hidden(u):
    """Pixels whose iterate the returned motion does not show: the composition
    onto the zero motion (Motion::accumulate) leaves 0 where u is NaN or
    points outside the image."""
    with np.errstate(all="ignore"):
        px = np.arange(NX, dtype=F)[:, None] + u[:, :, 0]
        py = np.arange(NY, dtype=F)[None, :] + u[:, :, 1]
        inside = (np.floor(px) >= 0) & (np.floor(px) < NX) & (np.floor(py) >= 0) & \
                 (np.floor(py) < NY)
    return ~inside


def test_oracle_motion_is_not_hidden(oracle):
    """A case must not hide behind NaN.  The motion the registration returns
    is the iterate composed onto the zero motion, which is 0 wherever the
    iterate is NaN or points outside the image, so a NaN never reaches the
    returned motion and a huge value does not either.  For every case and
    iteration count compared below: at most half of the pixels are hidden in
    that way, the visible ones are the iterate itself, and cases 1 to 6 have
    no NaN at all in the iterate."""
    for n in NAMES:
        for it in ITERS:
            u = oracle_iterate(oracle, n, it)
            h = hidden(u)
            assert h.sum() <= h.size // 2, (n, it, int(h.sum()))
            m = want(oracle, n, it)
            assert not np.isnan(m).sum() and not m[h].any()
            if n[0] != "8":  # there the identity warp of the moving image spreads
                # the pixel to its left and upper neighbours (NaN x weight 0)
                assert np.array_equal(bits(m[~h]), bits(u[~h])), (n, it)
            if n in NO_NAN:
                assert not np.isnan(u).any(), (n, it)
            assert m.any(), (n, it)
        if n[0] in "78":
            assert np.isnan(oracle_iterate(oracle, n, 13)).any(), n
    for n in CONV_NAMES:
        m, its, errs = want_conv(oracle, n)
        assert len(errs) == its[0]
        assert hidden(oracle_iterate(oracle, n, its[0])).sum() <= NX * NY // 2, n
    # 7a: a NaN error is never below the threshold, so the loop runs to the cap
    m, its, errs = want_conv(oracle, "7a")
    assert its == [CONV_CAP] and np.isnan(errs).any()


def test_oracle_raises_on_underflowed_denominator(oracle):
    ref, mov, alpha = case("9z")
    assert alpha == 0.0
    with pytest.raises(oracle.OracleError, match="Divide by zero exception"):
        oracle_fixed(oracle, ref, mov, alpha, 4)


# ------------------------------------------------------------------ GPU part
CONV_NAMES = ["2", "7a"]
GROUP_NAMES = ["1", "2", "3", "7a", "7b", "8n-seam"]
BATCH_NAMES = ["1", "2", "7a", "7b"] + list(NONFINITE) + ["9"]


@pytest.mark.gpu
@pytest.mark.parametrize("gi", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_registration_bitwise(gpu, oracle, name, gi):
    """ImageRegistration, fixed iterations: the single step, the pair, the
    triple (stored gradients and gradients from the image) and their mixes."""
    from opticalflow2d_amd import ImageRegistration
    ref, mov, alpha = case(name)
    for iters in ITERS:
        with ImageRegistration(DIMS, [iters], 0, 0, [alpha], fixed_iters=1,
                               hs_gradients_from_image=gi) as r:
            r.register(ref, mov)
            assert r.iterations() == [iters]
            m = r.motion()
        assert_bits(m, want(oracle, name, iters), f"case {name}, {iters} iterations, gi {gi}")


def slab_run(name, iters, quads):
    from opticalflow2d_amd import SlabSolver
    ref, mov, alpha = case(name)
    s = SlabSolver(NX, NY, alpha)
    try:
        s.set_images(ref, mov)
        s.set_option("hs_fixed_quads", quads)
        per_launch = s.info()["iterations_per_launch"]
        assert s.run(iters, fixed_iters=True) == iters
        return s.motion(), per_launch
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("quads", [1, 0])
@pytest.mark.parametrize("name", NAMES)
def test_slab_bitwise(gpu, oracle, name, quads):
    """SlabSolver, fixed iterations: quads (jacobi4_kernel) or triples, with
    the single step, pair or triple of the tail.

    Case 8 holds the slab to the reference's warp of the moving image by the
    zero motion, which spreads a NaN or inf pixel to its left and upper
    neighbours (slab.cpp set_images, launch_warp_zero_rows)."""
    for iters in ITERS:
        m, per_launch = slab_run(name, iters, quads)
        assert per_launch == (4 if quads else 3)
        assert_bits(m, want(oracle, name, iters),
                    f"case {name}, {iters} iterations, hs_fixed_quads {quads}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_two_rank_split_bitwise(gpu, oracle, name):
    """Two in-process slabs running interior and edge launches (split = 1)
    against the one-rank result (and so the oracle)."""
    from test_gpu_slab_local import run_group
    ref, mov, alpha = case(name)
    iters = 13
    one, _ = slab_run(name, iters, 1)
    m, done = run_group(ref, mov, alpha, 2, iters, True, split=1)
    assert done == [iters, iters]
    assert_bits(m, one, f"case {name}: two ranks against one")
    assert_bits(m, want(oracle, name, iters), f"case {name}: two ranks against the oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("name", BATCH_NAMES)
def test_batch_bitwise(gpu, oracle, name):
    """batch::hs_loop_kernel (plain IEEE division), the same pair twice."""
    from test_gpu_batch import run_batch
    ref, mov, alpha = case(name)
    iters = 13
    got = run_batch(DIMS, [iters], 0, alpha, 1, np.stack([ref, ref]), np.stack([mov, mov]),
                    fixed_iters=1)
    assert got["status"].tolist() == [0, 0] and got["error"] == ""
    assert got["iters"].tolist() == [[iters], [iters]]
    for k in range(2):
        assert_bits(got["motion"][k], want(oracle, name, iters), f"case {name}, pair {k}")


@pytest.mark.gpu
def test_width_one_grid_high_gradients(gpu, oracle):
    """1 x 40: loop_hs launches single steps only (no pair, triple or
    precheck below two columns).  Case 1's scale on one column of the texture.

    With one column the reference's partial_x takes its first branch,
    f[idx + 1] - f[idx] (gradients.h:9-19), and idx + 1 is the pixel of the next
    j-line; on the last j-line it is one element past the array, which no
    reference defines.  That value reaches j-line 39 in the first iteration
    and one j-line further up with each iteration after it (the stencil's
    reach), so after k iterations the j-lines below 40 - k are compared, and
    those are independent of it."""
    from opticalflow2d_amd import ImageRegistration
    r, m = tex()
    ref = (r[100:101, :40] * F(2.0 ** 24)).astype(np.float64)
    mov = (m[100:101, :40] * F(2.0 ** 24)).astype(np.float64)
    gx, gy, _ = derivatives(oracle, ref, mov)
    assert (np.abs(gy) >= HI_G).any() and (np.abs(gy) < HI_G).any()
    assert np.array_equal(gx[0, :39], (mov[0, 1:] - mov[0, :39]).astype(F))
    for iters in (1, 4, 13):
        o = oracle_fixed(oracle, ref, mov, 0.3, iters)[:, :40 - iters]
        assert not np.isnan(o).any() and o.any()
        with ImageRegistration((1, 40), [iters], 0, 0, [0.3], fixed_iters=1) as reg:
            reg.register(ref, mov)
            got = reg.motion()[:, :40 - iters]
        assert_bits(got, o, f"1 x 40, {iters} iterations")


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONV_NAMES)
def test_convergence_on_bitwise(gpu, oracle, name):
    """The default Logger with the convergence test on, cap 40: the oracle's
    iteration count, its errors on the bits (NaN positions included) and its
    motion.  A NaN error is not below 0.001, so 7a runs to the cap."""
    from opticalflow2d_amd import ImageRegistration
    ref, mov, alpha = case(name)
    m, its, errs = want_conv(oracle, name)
    with ImageRegistration(DIMS, [CONV_CAP], 0, 0, [alpha]) as r:
        r.register(ref, mov)
        got_its, got_errs, got = r.iterations(), r.last_errors(), r.motion()
    assert got_its == its
    assert_bits(got_errs, errs, f"case {name}: Logger errors")
    assert_bits(got, m, f"case {name}: motion")


@pytest.mark.gpu
def test_underflowed_denominator_raises(gpu, oracle):
    """alpha = 0 and squares that underflow: the denominator is exactly 0 on
    pixels with a gradient.  The reference's reported error, per pair in a
    batch."""
    from opticalflow2d_amd import ImageRegistration, Of2dError, SlabSolver, _lib
    from test_gpu_batch import make_pairs, oracle_pair, run_batch
    ref, mov, alpha = case("9z")
    with ImageRegistration(DIMS, [4], 0, 0, [alpha], fixed_iters=1) as r:
        with pytest.raises(Of2dError, match="Divide by zero exception"):
            r.register(ref, mov)
    s = SlabSolver(NX, NY, alpha)
    try:
        s.set_images(ref, mov)
        with pytest.raises(Of2dError, match="Divide by zero exception"):
            s.run(4, fixed_iters=True)
    finally:
        s.close()
    refs, movs = make_pairs(DIMS, 3)
    bad = 1
    refs[bad], movs[bad] = ref, mov
    got = run_batch(DIMS, [4], 0, alpha, 1, refs, movs, fixed_iters=1)
    expect = [_lib.OF2D_OK] * 3
    expect[bad] = _lib.OF2D_ERR_RUNTIME
    assert got["status"].tolist() == expect
    assert "Divide by zero exception" in got["error"] and f"pair {bad}" in got["error"]
    for k in (0, 2):
        m, _, _ = oracle_pair(oracle, DIMS, [4], 0, alpha, 1, refs[k], movs[k])
        assert_bits(got["motion"][k], m, f"pair {k}")
