"""Curvature's device transforms (of2d_dct2d) against the oracle's naive sums.

Both sides are fp64 evaluations of the same REDFT10 / REDFT01 sums (the fast
path reorders them through an FFT, the GEMM path through MFMA tiles), so the
bar is the one tests/test_oracle.py holds the oracle itself to against scipy:
max |got - want| <= 1e-12 * max |want|, on seeded uniform input as there.

The device array is a[i + j*dimx]; the oracle takes a row-major n0 x n1 array
and transforms axis 1 first, so the [dimx, dimy] array in C order makes it run
axis y then axis x, the order of the device.  Every case asserts which path
each axis took, so a fallback cannot pass as the fast path.

The oracle costs n^2 cosines per line: the two orientations of a long-line
shape ((n, 16) and (16, n)) share one oracle run, on the same numbers
transposed (the separable transform of the transpose is the transpose; only
the order of the two axis passes differs, far inside the bar).

of2d_dct2d transforms one plane: these cases check the x plane of the device's
plane pair next to a y plane of zeros.  Both planes at once, the GEMM path's
ragged tiles and the fused eigenvalue product are in
tests/test_gpu_curvature_prims.py, against an extended-precision reference.
"""
import functools

import numpy as np
import pytest

from opticalflow2d_amd import dct2d
from opticalflow2d_amd.registration import DCT_NMAX, DCT_NMIN

pytestmark = pytest.mark.gpu

RTOL = 1e-12
KINDS = (10, 1)


def fast(n):
    return int(DCT_NMIN <= n <= DCT_NMAX and n & (n - 1) == 0)


@functools.lru_cache(maxsize=None)
def _oracle_case(shape, kind):
    """(input, oracle result) for a [dimx, dimy] array; cached, never modified."""
    from oracle import oracle as O
    a = np.random.default_rng(1000 * shape[0] + shape[1]).random(shape)
    b = np.ascontiguousarray(a.copy())
    O.lib().oracle_dct2d(b, shape[0], shape[1], kind)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def case(shape, kind):
    """Long-line shapes (n, 16) reuse the oracle run of (16, n)."""
    if shape[1] == 16 and shape[0] >= 4096:
        a, b = _oracle_case((shape[1], shape[0]), kind)
        return a.T, b.T
    return _oracle_case(shape, kind)


def check(shape, kind, method, want_paths):
    a, want = case(shape, kind)
    got, paths = dct2d(a, kind=kind, method=method)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print(f"dct2d {shape} kind {kind} method {method}: paths {paths}, "
          f"max err {err:.3e}, bar {RTOL * scale:.3e}")
    assert paths == want_paths
    assert err <= RTOL * scale


SHAPES = [(8, 8), (64, 16), (16, 64), (512, 512), (4096, 16), (16, 4096),
          (64, 37), (70, 64), (4, 16)]
if DCT_NMAX > 4096:
    SHAPES += [(DCT_NMAX, 16), (16, DCT_NMAX)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fast_dct2d_matches_oracle(gpu, oracle, shape, kind):
    check(shape, kind, 1, (fast(shape[0]), fast(shape[1])))


def test_expected_paths_of_the_cases():
    """The cases reach every path: both fast, each axis falling back alone
    (not a power of two, below the minimum), the longest line on each axis."""
    p = {s: (fast(s[0]), fast(s[1])) for s in SHAPES}
    assert p[(8, 8)] == (1, 1) and p[(4096, 16)] == (1, 1) and p[(16, 4096)] == (1, 1)
    assert p[(64, 37)] == (1, 0) and p[(70, 64)] == (0, 1) and p[(4, 16)] == (0, 1)
    assert p[(DCT_NMAX, 16)] == (1, 1) and fast(2 * DCT_NMAX) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_gemm_dct2d_matches_oracle(gpu, oracle, kind):
    """The entry on the existing path: method 0 runs both axes as GEMMs."""
    check((64, 16), kind, 0, (0, 0))
