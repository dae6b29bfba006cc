"""Curvature one launch at a time: the rhs kernel, the eigenvalue table, the
2-D transforms on BOTH planes (with and without the fused eigenvalue product)
and the construct kernel with its Logger partials.

Every entry of `opticalflow2d_amd.prim.curv_*` makes one call of the function
Registration::loop_curvature calls (csrc/of2d_prims.h).  What is held to what:

* rhs, construct (field), eigenvalues: on the bits.  The first two are plain
  float32 arithmetic restated in numpy in the kernel's order; the table is the
  oracle's expression on the same host libm.
* transforms: max |got - ref| <= 1e-12 * max |ref| per plane (the project's
  bar, test_gpu_dct.py / test_oracle.py), against REDFT10 / REDFT01 matrices
  built in np.longdouble (80-bit) and applied as M0 @ a @ M1.T.  The oracle's
  naive fp64 sums are not used: on zero-mean input their own error reaches
  2.5e-13 of max |ref| at 2048 points (the argument error of cos(pi (j + 1/2)
  k / n) at large j k), a quarter of the bar.
  test_longdouble_reference_and_oracle_agree (CPU) holds the two references
  together at 5e-13.  The matrices reduce (2j + 1) k modulo 4n in integers
  before the cosine, so their error is that of one longdouble cosine, ~1e-19.
* construct's Logger partials: 1e-12 relative against math.fsum of the fp64
  magnitudes (Motion::norm's terms, the oracle's fp64 Logger).

The planes of a transform case are two different standard_normal arrays, and
every case also runs with either plane zeroed: the zero plane has to come back
exactly zero, on either path (the fast path did not, until its line kernel
gave each plane its own FFT: test_fast_zero_plane_comes_back_zero).
test_gpu_dct.py checks the x plane only, next to a zero y plane.

Arrays: fields in the C-ABI's layout (image [dimy, dimx], motion [dimy, dimx,
2]); transform planes and the eigenvalue table [dimx, dimy].
"""
import functools
import math

import numpy as np
import pytest

from opticalflow2d_amd import dct2d, prim
from opticalflow2d_amd.registration import DCT_NMAX, DCT_NMIN

gpu_test = pytest.mark.gpu
F = np.float32
LD = np.longdouble
LD_OK = bool(np.finfo(LD).eps < 2e-19)
needs_ld = pytest.mark.skipif(not LD_OK, reason="np.longdouble is not an 80-bit type here: "
                                                "no extended-precision transform reference")
RTOL = 1e-12
KINDS = (10, 1)
ids = lambda s: "x".join(str(v) for v in s) if isinstance(s, tuple) else str(s)  # noqa: E731


def fast(n):
    return int(DCT_NMIN <= n <= DCT_NMAX and n & (n - 1) == 0)


# ------------------------------------------------------------------ transform reference
@functools.lru_cache(maxsize=4)
def ld_matrix(n, kind):
    """The REDFT10 (kind 10) / REDFT01 (kind 1) matrix of length n in longdouble:
    Y_k = sum_j M[k, j] X_j.  The angle pi r / (2n) takes r = (2j + 1) k
    (resp. j (2k + 1)) reduced modulo 4n exactly."""
    pi = 4 * np.arctan(LD(1))
    k = np.arange(n, dtype=np.int64)[:, None]
    j = np.arange(n, dtype=np.int64)[None, :]
    r = ((2 * j + 1) * k if kind == 10 else j * (2 * k + 1)) % (4 * n)
    M = 2 * np.cos(pi * r.astype(LD) / LD(2 * n))
    if kind == 1:
        M[:, 0] = 1
    assert M.dtype == LD
    return M


def ld_dct2d(a, kind):
    n0, n1 = a.shape
    return ld_matrix(n0, kind) @ a.astype(LD) @ ld_matrix(n1, kind).T


def planes(shape):
    """Two different zero-mean planes [dimx, dimy]."""
    ax = np.random.default_rng(7000 * shape[0] + shape[1]).standard_normal(shape)
    ay = np.random.default_rng(7000 * shape[0] + shape[1] + 3511).standard_normal(shape)
    return ax, ay


@functools.lru_cache(maxsize=None)
def transform_case(shape, kind):
    """(ax, ay, ref x, ref y): inputs fp64, references longdouble; never modified."""
    ax, ay = planes(shape)
    out = ax, ay, ld_dct2d(ax, kind), ld_dct2d(ay, kind)
    for v in out:
        v.setflags(write=False)
    return out


def plane_err(got, ref):
    """(max |got - ref|, max |ref|) in longdouble."""
    return float(np.abs(got.astype(LD) - ref).max()), float(np.abs(ref).max())


def test_longdouble_reference_and_oracle_agree(oracle):
    """np.longdouble carries 64 bits here, and the longdouble matrices and
    oracle_dct2d are the same transform: within 5e-13 * max |ref| at the three
    shapes the oracle's own error was measured at (2.3e-14, 1.2e-13, 2.5e-13),
    on zero-mean input."""
    assert np.finfo(LD).eps < 2e-19
    for shape in ((129, 65), (1024, 8), (2048, 16)):
        ax, _, ref, _ = transform_case(shape, 10)
        b = np.ascontiguousarray(ax.copy())
        oracle.lib().oracle_dct2d(b, shape[0], shape[1], 10)
        err, scale = plane_err(b, ref)
        print(f"oracle_dct2d {shape} against longdouble: {err / scale:.2e} of max |ref|")
        assert err <= 5e-13 * scale


def run_transform(shape, kind, method):
    """The case's three runs (both planes, y zeroed, x zeroed): every
    non-zero plane at the bar, the paths as expected.  Returns what came back
    in the zeroed planes: {run: (max |.|, max |ref| of the other plane)}."""
    want_paths = (fast(shape[0]), fast(shape[1])) if method else (0, 0)
    ax, ay, rx, ry = transform_case(shape, kind)
    zero = np.zeros(shape)
    leaks = {}
    for what, a, b in (("xy", ax, ay), ("x0", ax, zero), ("0y", zero, ay)):
        gx, gy, paths = prim.curv_dct2d(a, b, kind, method)
        assert paths == want_paths, (what, paths)
        for name, inp, got, ref, other in (("x", a, gx, rx, ry), ("y", b, gy, ry, rx)):
            if inp is zero:
                leaks[what] = float(np.abs(got).max()), float(np.abs(other).max())
                continue
            err, scale = plane_err(got, ref)
            print(f"curv_dct2d {shape} kind {kind} method {method} {what} plane {name}: "
                  f"paths {paths}, max err {err:.3e}, bar {RTOL * scale:.3e} "
                  f"({err / scale:.2e} of max |ref|)")
            assert err <= RTOL * scale, (what, name)
    return leaks


def check_zero_planes(shape, kind, method):
    leaks = run_transform(shape, kind, method)
    for what, (leak, scale) in leaks.items():
        print(f"curv_dct2d {shape} kind {kind} method {method} {what}: the zeroed plane came "
              f"back with max |.| {leak:.3e} ({leak / scale:.2e} of the other plane's max |ref|)")
    assert all(leak == 0.0 for leak, _ in leaks.values()), leaks


# M, N and K of dgemm_nn_kernel one below, on and one above its 16-deep LDS
# stage and its 64-wide tile, K no multiple of the MFMA's 4, 1 to 3 tiles a side
GEMM_SHAPES = [(1, 1), (1, 7), (7, 1), (5, 4), (3, 200), (15, 17), (16, 16), (17, 15), (63, 65),
               (64, 64), (65, 63), (129, 65), (130, 96)]
# the powers of two test_gpu_dct.py leaves out (1024: the first length with one
# line per block; both parities of log2 n, so the half-length FFT ends in a
# radix-4 and in a radix-2 pass), fewer lines than a
# block holds, mixed paths with a ragged last block of lines
FAST_SHAPES = ([(n, 16) for n in (8, 32, 128, 256, 1024, 2048)] +
               [(16, n) for n in (8, 32, 128, 256, 1024, 2048)] +
               [(8, 3), (3, 8), (64, 37), (70, 64)])
# no longdouble matrix at these lengths (1 GB): round trip and single planes
LONG_SHAPES = [(4096, 16), (16, 4096), (DCT_NMAX, 8), (8, DCT_NMAX)]


def test_expected_paths_of_the_cases():
    p = {s: (fast(s[0]), fast(s[1])) for s in FAST_SHAPES + LONG_SHAPES}
    assert all(p[(n, 16)] == (1, 1) and p[(16, n)] == (1, 1)
               for n in (8, 32, 128, 256, 1024, 2048, 4096))
    assert p[(8, 3)] == (1, 0) and p[(3, 8)] == (0, 1)
    assert p[(64, 37)] == (1, 0) and p[(70, 64)] == (0, 1)
    assert p[(DCT_NMAX, 8)] == (1, 1) and p[(8, DCT_NMAX)] == (1, 1) and not fast(2 * DCT_NMAX)


@gpu_test
@needs_ld
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=ids)
def test_gemm_transform_both_planes(gpu, shape, kind):
    run_transform(shape, kind, 0)


@gpu_test
@needs_ld
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", FAST_SHAPES, ids=ids)
def test_fast_transform_both_planes(gpu, shape, kind):
    run_transform(shape, kind, 1)


@gpu_test
@needs_ld
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=ids)
def test_gemm_zero_plane_comes_back_zero(gpu, shape, kind):
    """The GEMM path runs the second plane through blockIdx.z strides: a zero
    plane in is a zero plane out, exactly."""
    check_zero_planes(shape, kind, 0)


@gpu_test
@needs_ld
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", FAST_SHAPES, ids=ids)
def test_fast_zero_plane_comes_back_zero(gpu, shape, kind):
    """The fast path keeps the planes apart on the bits: each plane of a line
    is its own half-length complex FFT (a real FFT), side by side in LDS.

    Found by this test: the line kernel used to pack the x and y plane as the
    real and imaginary part of ONE complex FFT and separate them through the
    Hermitian symmetry of a real line's spectrum, which the radix-4 passes
    keep to rounding only.  A zeroed plane came back as the other plane's
    rounding error, 1.3e-15 ((3, 8)) to 7.5e-13 ((2048, 16)) absolute, at most
    4.9e-16 of the other plane's max |ref|, in all 32 cases."""
    check_zero_planes(shape, kind, 1)


@gpu_test
@pytest.mark.parametrize("shape", LONG_SHAPES, ids=ids)
def test_long_lines_round_trip_and_single_planes(gpu, shape):
    """REDFT01(REDFT10(a)) = 4 dimx dimy a on the plane pair, and the pair's
    transforms equal the single-plane ones of of2d_dct2d."""
    ax, ay = planes(shape)
    n4 = 4.0 * shape[0] * shape[1]
    fx, fy, paths = prim.curv_dct2d(ax, ay, 10, 1)
    assert paths == (1, 1)
    bx, by, paths = prim.curv_dct2d(fx, fy, 1, 1)
    assert paths == (1, 1)
    for name, a, back in (("x", ax, bx), ("y", ay, by)):
        err, bar = np.abs(back - n4 * a).max(), RTOL * np.abs(a).max() * n4
        print(f"round trip {shape} plane {name}: max err {err:.3e}, bar {bar:.3e}")
        assert err <= bar, name
    ix, iy, _ = prim.curv_dct2d(ax, ay, 1, 1)
    for kind, pair in ((10, (fx, fy)), (1, (ix, iy))):
        for name, a, got in (("x", ax, pair[0]), ("y", ay, pair[1])):
            want, p1 = dct2d(a, kind=kind, method=1)
            assert p1 == (1, 1)
            err, bar = np.abs(got - want).max(), RTOL * np.abs(want).max()
            print(f"pair against single {shape} kind {kind} plane {name}: max err {err:.3e}, "
                  f"bar {bar:.3e}")
            assert err <= bar, (kind, name)


# ------------------------------------------------------------------ eigenvalues
ALPHA_TAU = [(0.5, 0.2), (2.0, 1.0), (1e-3, 3.0), (0.0, 1.0)]


def oracle_eigen(oracle, shape, alpha, tau):
    out = np.zeros(shape[0] * shape[1])
    oracle.lib().oracle_curvature_eigenvalues(shape[0], shape[1], alpha, tau, out)
    return out.reshape(shape)


@gpu_test
@pytest.mark.parametrize("method", (0, 1))
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (5, 4), (37, 64), (64, 37), (130, 96)],
                         ids=ids)
def test_eigenvalue_table(gpu, oracle, shape, method):
    """build_curvature's table against the oracle's export on the fp64 bits:
    both run the reference's expression on the same host libm, so a difference
    is one in the expression (PI = 3.14159265, the float tau * alpha, unsigned
    p and q) or a contraction in host code.  The table does not depend on the
    transforms' path; alpha = 0 gives E = 1."""
    for alpha, tau in ALPHA_TAU:
        got = prim.curv_eigen(shape, alpha, tau, method)
        want = oracle_eigen(oracle, shape, alpha, tau)
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        assert len(bad) == 0, (f"alpha {alpha} tau {tau}: {len(bad)} of {got.size} differ, first "
                               f"at {tuple(bad[0])}: {got[tuple(bad[0])]!r} want "
                               f"{want[tuple(bad[0])]!r}")
        if alpha == 0.0:
            assert np.all(got == 1.0)


FUSED_SHAPES = [(5, 4), (65, 63), (64, 37), (37, 64), (70, 64), (64, 64), (1024, 8)]
# method 1 where an axis takes the fast path (elsewhere it is method 0 again)
FUSED_CASES = [(s, m) for s in FUSED_SHAPES for m in (0, 1) if m == 0 or fast(s[0]) or fast(s[1])]


@gpu_test
@needs_ld
@pytest.mark.parametrize("shape,method", FUSED_CASES, ids=lambda v: ids(v))
def test_fused_eigenvalue_product(gpu, oracle, shape, method):
    """The forward transform with the eigenvalues fused into its axis-x pass
    (the GEMM's epilogue E[m + n*lde], the line kernel's E + off) against the
    longdouble transform times the oracle's table, element by element.  All
    shapes but one are non-square: a transposed read of the table fails."""
    want_paths = (fast(shape[0]), fast(shape[1])) if method else (0, 0)
    ax, ay, rx, ry = transform_case(shape, 10)
    for alpha, tau in ((0.5, 0.2), (2.0, 1.0)):
        E = oracle_eigen(oracle, shape, alpha, tau).astype(LD)
        gx, gy, paths = prim.curv_dct2d(ax, ay, 10, method, eig=(alpha, tau))
        assert paths == want_paths
        for name, got, ref in (("x", gx, rx * E), ("y", gy, ry * E)):
            err, scale = plane_err(got, ref)
            print(f"fused {shape} method {method} alpha {alpha} tau {tau} plane {name}: "
                  f"max err {err:.3e}, bar {RTOL * scale:.3e}")
            assert err <= RTOL * scale, (alpha, tau, name)


def test_fused_product_is_refused_on_the_inverse(of2d_lib):
    """with_eig is the solver's forward pass only; refused before any device work."""
    a = np.zeros((4, 4))
    with pytest.raises(ValueError):
        prim.curv_dct2d(a, a, 1, 0, eig=(1.0, 1.0))
    with pytest.raises(ValueError):
        prim.curv_dct2d(a, a, 7, 0)
    with pytest.raises(ValueError):
        prim.curv_eigen((4, 4), 1.0, 1.0, method=2)


# ------------------------------------------------------------------ rhs
# the block edges of the 64 x 4 launch on both sides of a tile
FIELD_SHAPES = [(1, 1), (63, 3), (64, 4), (65, 5), (130, 7)]
TAUS = (0.0, 1.0, 0.2)
NAN = float("nan")
# planted pixels: (class, {operand: value}); operands ux uy gx gy it
RHS_PLANTS = ([(f"negzero_{k}", {k: -0.0}) for k in ("ux", "uy", "gx", "gy", "it")] +
              [(f"nan_{k}", {k: NAN}) for k in ("ux", "uy", "gx", "gy", "it")] +
              [("subnormal_u", {"ux": 1e-40, "uy": -1e-40}),
               ("subnormal_u_only", {"ux": -1e-40, "uy": 1e-40, "gx": 0.0, "gy": 0.0, "it": 0.0}),
               ("subnormal_g", {"gx": 1e-40, "gy": -3e-41}),
               ("subnormal_it", {"it": 1e-40, "ux": 0.0, "uy": 0.0}),
               ("subnormal_product", {"ux": 1e-20, "gx": 1e-20, "uy": 0.0, "it": 0.0}),
               ("overflow", {"gx": 1e30, "gy": 1e30, "ux": 1e10, "uy": 1e10}),
               ("overflow_cancel", {"gx": 1e30, "gy": -1e30, "ux": 1e10, "uy": 1e10})])


@functools.lru_cache(maxsize=None)
def rhs_inputs(shape):
    """(u, dI, It, classes): smooth mixed-sign fields with RHS_PLANTS spread
    over the pixels (a grid too small for all of them takes the first ones)."""
    dimx, dimy = shape
    rng = np.random.default_rng(500 * dimx + dimy)
    u = (2.0 * rng.standard_normal((dimy, dimx, 2))).astype(F)
    g = (0.3 * rng.standard_normal((dimy, dimx, 2))).astype(F)
    it = (0.5 * rng.standard_normal((dimy, dimx))).astype(F)
    op = {"ux": u[..., 0], "uy": u[..., 1], "gx": g[..., 0], "gy": g[..., 1], "it": it}
    n = dimx * dimy
    step = max(1, n // len(RHS_PLANTS))
    classes = {}
    for k, (name, vals) in enumerate(RHS_PLANTS):
        # the last plant on the last pixel: the corner of the ragged last block
        p = n - 1 if k == len(RHS_PLANTS) - 1 and n > len(RHS_PLANTS) else k * step
        if p >= n or (k and p == 0):
            break
        j, i = divmod(p, dimx)
        for key, v in vals.items():
            op[key][j, i] = F(v)
        classes[name] = (j, i)
    for a in (u, g, it):
        a.setflags(write=False)
    return u, g, it, classes


def rhs_reference(u, g, it, tau):
    """curv_rhs_kernel in numpy float32, in its order; (force, rhs as fp64)."""
    with np.errstate(all="ignore"):
        sc = (it + u[..., 0] * g[..., 0]) + u[..., 1] * g[..., 1]
        f = g * sc[..., None]
        x = u - F(tau) * f
    assert sc.dtype == F and f.dtype == F and x.dtype == F
    return f, np.stack([x[..., 0], x[..., 1]]).astype(np.float64)


def same_bits(got, want, what):
    """Equal bit patterns (uint views of the arrays' own width); NaN by position."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    view = np.uint64 if got.dtype == np.float64 else np.uint32
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.argwhere((gn != wn) | (~wn & (got.view(view) != want.view(view))))
    if len(bad):
        k = tuple(bad[0])
        pytest.fail(f"{what}: {len(bad)} of {got.size} differ, first at {k}: got {got[k]!r} "
                    f"want {want[k]!r}")


def test_rhs_inputs_hold_every_class():
    """Each planted class is in the inputs and does what its name says."""
    sub = lambda v: v != 0 and abs(float(v)) < float(np.finfo(F).tiny)  # noqa: E731
    for shape in FIELD_SHAPES[1:]:
        u, g, it, cl = rhs_inputs(shape)
        assert set(cl) == {name for name, _ in RHS_PLANTS}, shape
        assert len(set(cl.values())) == len(cl), "two plants on one pixel"
        assert cl[RHS_PLANTS[-1][0]] == (shape[1] - 1, shape[0] - 1)
        op = {"ux": u[..., 0], "uy": u[..., 1], "gx": g[..., 0], "gy": g[..., 1], "it": it}
        for k in op:
            v = op[k][cl[f"negzero_{k}"]]
            assert v == 0 and np.signbit(v)
            assert np.isnan(op[k][cl[f"nan_{k}"]])
        assert sub(u[cl["subnormal_u"]][0]) and sub(u[cl["subnormal_u"]][1])
        assert sub(g[cl["subnormal_g"]][0]) and sub(g[cl["subnormal_g"]][1])
        assert sub(it[cl["subnormal_it"]])
        f, x = rhs_reference(u, g, it, 1.0)
        # +-1e-40 motion with no force: the subnormal itself comes through
        assert x[0][cl["subnormal_u_only"]] == float(F(-1e-40))
        p = cl["subnormal_product"]
        assert sub(u[p][0] * g[p][0])
        assert np.isinf(f[cl["overflow"]]).all() and np.isinf(x[(slice(None),) + cl["overflow"]]).all()
        assert np.isnan(f[cl["overflow_cancel"]]).all()       # inf - inf
        _, x0 = rhs_reference(u, g, it, 0.0)
        assert np.isnan(x0[0][cl["overflow"]])                 # 0 * inf
        # NaN in any operand reaches both planes (through sc) or its own plane
        for k in ("gx", "gy", "it"):
            assert np.isnan(x[0][cl[f"nan_{k}"]]) and np.isnan(x[1][cl[f"nan_{k}"]])
    u, g, it, cl = rhs_inputs((1, 1))
    assert list(cl) == ["negzero_ux"]


@gpu_test
@pytest.mark.parametrize("shape", FIELD_SHAPES, ids=ids)
def test_rhs(gpu, oracle, shape):
    """curv_rhs_kernel against its float32 restatement, on the fp64 bits, for
    tau 0, 1 and 0.2; the force part of the restatement against
    oracle_get_force (OpticalFlow.cpp:15-39)."""
    u, g, it, _ = rhs_inputs(shape)
    f, _ = rhs_reference(u, g, it, 1.0)
    fo = np.zeros(u.size, F)
    oracle.lib().oracle_get_force(u.reshape(-1), g.reshape(-1), it.reshape(-1), it.size, fo)
    same_bits(f, fo.reshape(f.shape), f"force restatement against the oracle {shape}")
    for tau in TAUS:
        _, want = rhs_reference(u, g, it, tau)
        same_bits(prim.curv_rhs(u, g, it, tau), want, f"curv_rhs {shape} tau {tau}")


# ------------------------------------------------------------------ construct
CONSTRUCT_SHAPES = FIELD_SHAPES + [(127, 3)]   # 4 n = 1524: no power of two


def midpoint(lo):
    """The double half-way between the float lo and the next float up."""
    lo = F(lo)
    return (float(lo) + float(np.nextafter(lo, F(np.inf)))) / 2


def construct_plants():
    """name -> double, for Z: what the double -> float conversion can get wrong."""
    # neighbouring floats: the lower float's last mantissa bit is 0 for one, 1 for the other
    fmax = float(np.finfo(F).max)
    p = {}
    for name, lo in (("a", F(1.0)), ("b", np.nextafter(F(1.0), F(2.0))), ("c", F(3.0e7)),
                     ("d", np.nextafter(F(3.0e7), F(np.inf)))):
        m = midpoint(lo)
        p[f"mid_{name}"] = m
        p[f"mid_{name}_below"] = float(np.nextafter(m, -np.inf))
        p[f"mid_{name}_above"] = float(np.nextafter(m, np.inf))
        p[f"mid_{name}_neg"] = -m
    p.update(past_max=1e39, past_max_neg=-1e39, huge=1e300,
             max_tie=fmax + 2.0 ** 103,                         # half an ulp past FLT_MAX: inf
             max_tie_below=float(np.nextafter(fmax + 2.0 ** 103, 0.0)),  # FLT_MAX
             sub_quotient=2e-38, sub_quotient_neg=-3e-38, sub_itself=1e-42, vanishing=1e-60,
             negzero=-0.0, nan=NAN, ordinary=1234.5678, ordinary_neg=-0.3)
    return p


@functools.lru_cache(maxsize=None)
def construct_inputs(shape):
    """(z [2, dimy, dimx] fp64, u, classes name -> (plane, j, i))."""
    dimx, dimy = shape
    n = dimx * dimy
    rng = np.random.default_rng(900 * dimx + dimy)
    z = (4.0 * n) * rng.standard_normal((2, dimy, dimx))
    u = rng.standard_normal((dimy, dimx, 2)).astype(F)
    plants = construct_plants()
    classes = {}
    step = max(1, 2 * n // len(plants))
    for k, (name, v) in enumerate(plants.items()):
        p = 2 * n - 1 if k == len(plants) - 1 and 2 * n > len(plants) else k * step
        if p >= 2 * n or (k and p == 0):
            break
        c, (j, i) = p // n, divmod(p % n, dimx)
        z[c, j, i] = v
        classes[name] = (c, j, i)
    z.setflags(write=False)
    u.setflags(write=False)
    return z, u, classes


def construct_reference(z, shape):
    """(float)Z / (4.0f * n) per component, [dimy, dimx, 2] float32."""
    div = F(4.0) * F(shape[0] * shape[1])
    with np.errstate(all="ignore"):
        out = np.stack([z[0].astype(F), z[1].astype(F)], axis=-1) / div
    assert out.dtype == F
    return out, div


def test_construct_inputs_hold_every_class():
    fmax = np.finfo(F).max
    for shape in CONSTRUCT_SHAPES[1:]:
        z, _, cl = construct_inputs(shape)
        assert set(cl) == set(construct_plants()), shape
        assert len(set(cl.values())) == len(cl)
        out, div = construct_reference(z, shape)
        o = {k: out[j, i, c] for k, (c, j, i) in cl.items()}
        with np.errstate(all="ignore"):
            f = {k: F(z[v]) for k, v in cl.items()}
        parities = set()
        for name in "abcd":
            lo = f[f"mid_{name}_below"]
            hi = np.nextafter(lo, F(np.inf))
            assert z[cl[f"mid_{name}"]] == (float(lo) + float(hi)) / 2
            assert f[f"mid_{name}_above"] == hi
            # the tie goes to the even neighbour: down for an even lower float
            odd = int(lo.view(np.uint32) & 1)
            assert f[f"mid_{name}"] == (hi if odd else lo)
            assert f[f"mid_{name}_neg"] == -(hi if odd else lo)
            parities.add(odd)
        assert parities == {0, 1}
        assert np.isposinf(o["past_max"]) and np.isneginf(o["past_max_neg"])
        assert np.isposinf(o["huge"])
        assert np.isposinf(f["max_tie"]) and f["max_tie_below"] == fmax
        tiny = np.finfo(F).tiny
        assert abs(f["sub_quotient"]) >= tiny and 0 < abs(o["sub_quotient"]) < tiny
        assert abs(f["sub_quotient_neg"]) >= tiny and 0 < abs(o["sub_quotient_neg"]) < tiny
        assert 0 < f["sub_itself"] < tiny and o["vanishing"] == 0
        assert o["negzero"] == 0 and np.signbit(o["negzero"]) and np.isnan(o["nan"])
        assert o["ordinary"] == F(1234.5678) / div
    assert F(4.0) * F(127 * 3) == 1524


@gpu_test
@pytest.mark.parametrize("shape", CONSTRUCT_SHAPES, ids=ids)
def test_construct_field(gpu, shape):
    """curv_construct_kernel's field on the float32 bits: the double -> float
    conversion (ties, overflow to inf, subnormals), then the float division."""
    z, u, _ = construct_inputs(shape)
    want, div = construct_reference(z, shape)
    got, _ = prim.curv_construct(z, u, div)
    same_bits(got, want, f"curv_construct {shape}")


def logger_sums(out, u):
    """The oracle's fp64 Logger (Motion::norm's terms): float32 differences,
    squares, sum and root in fp64, summed exactly."""
    e = (out - u).astype(np.float64)
    assert (out - u).dtype == F
    q = u.astype(np.float64)
    return (math.fsum(np.sqrt(e[..., 0] ** 2 + e[..., 1] ** 2).ravel()),
            math.fsum(np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2).ravel()))


@gpu_test
@pytest.mark.parametrize("scale", (1.0, 1e-25, 1e25), ids=("unit", "tiny", "huge"))
@pytest.mark.parametrize("shape", CONSTRUCT_SHAPES, ids=ids)
def test_construct_logger_sums(gpu, shape, scale):
    """The launch's Logger partials, added in block order, against the fp64
    Logger sums at 1e-12 relative (the bound test_gpu_primitives.py holds
    smooth_norm to), on finite fields of magnitude about 1, about 1e-25 and
    about 1e25: the float32 squares of the last two leave the float range
    (0 below ~1e-23, inf above 1.8e19), the fp64 terms do not.

    Found by this test: curv_construct_kernel took the magnitudes as
    sqrtf(ex * ex + ey * ey) in float32 and widened afterwards; the unit field
    came out 4e-8 (one pixel) to 5e-10 (64 x 4) relative off, the tiny field 0
    and the huge field inf; after the change the sums agree to 2e-16.
    The kernel now squares and roots in fp64, as smooth_norm_kernel does."""
    dimx, dimy = shape
    rng = np.random.default_rng(1300 * dimx + dimy)
    div = F(4.0) * F(dimx * dimy)
    z = (float(div) * scale) * rng.standard_normal((2, dimy, dimx))
    u = (scale * rng.standard_normal((dimy, dimx, 2))).astype(F)
    want_out, _ = construct_reference(z, shape)
    got, sums = prim.curv_construct(z, u, div)
    same_bits(got, want_out, f"curv_construct {shape} scale {scale}")
    want = logger_sums(want_out, u)
    for name, g, w in zip(("sum |out - u|", "sum |u|"), sums, want):
        rel = abs(g - w) / w
        print(f"construct sums {shape} scale {scale} {name}: got {g!r} want {w!r} rel {rel:.3e}")
        assert w > 0 and math.isfinite(w)
        assert rel <= 1e-12, name
