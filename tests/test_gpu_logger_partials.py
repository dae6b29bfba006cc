"""The summation order of the fp64 Logger sums, on the bits.

Four kernels take the Logger's two sums (sum |new - prev|, sum |prev|) per
block and a one-block launch adds the blocks: smooth_norm_kernel (Demons),
curv_construct_kernel, fluid_step_kernel and logger_kernel (Elastic).  The order
of those additions is the project's contract (DESIGN.md "fixed order"); this
file restates it in numpy and holds the device's sums to it bit for bit:

* a thread adds its own terms in its kernel's row order (THREAD_ROWS below);
* the 64 lanes of a wave are added as a tree, ``v[:off] += v[off:2*off]`` for
  off = 32 ... 1 (lanes outside the image hold 0.0);
* the block's 4 waves are added in order, ((w0 + w1) + w2) + w3;
* the blocks, numbered by * gridx + bx, are added by 1024 threads: thread t
  adds blocks t, t + 1024, ... in order, then the wave tree, then the 16 waves
  in order (reduce_partials_kernel; the Fluid report kernel does the same).
  of2d_prim_curv_construct alone adds its blocks on the host, in block order.

Inputs.  The model takes no root: every magnitude is exact in fp64.  Per pixel
prev = (3, 4) a 2^e and new - prev = (5, 12) b 2^e (components swapped and
signed at random) with integers a, b < 2^16 and e in [-20, 30], so |prev| =
5 a 2^e, |new - prev| = 13 b 2^e, new = prev + (new - prev) is exact in float32
and so is the float32 difference the kernels take.  The terms span some 70
binary digits, more than a double holds, so the sums depend on the order; each
case asserts that on the CPU (np.sum, or the model with the waves reversed,
gives other bits) before it looks at the device.

The Demons smoothing runs with sigma = 0.05, for which the reference's Gaussian
table is exactly the unit impulse (expf(-1 / 0.005) is 0 in float32): the
smoothed field is u_mid itself, which each case asserts, whichever kernel ran
(compile-time width 3, runtime width 4, separable width 3).

The CPU part guards the reason the direct kernels of a compile-time width never
divide by the weight sum: for an odd width it rounds to float 1.
"""
import functools

import numpy as np
import pytest

from opticalflow2d_amd import prim

gpu_test = pytest.mark.gpu
F = np.float32

# 65 x 5, 130 x 9: ragged second block column and row; 64 x 4: one block of
# the 64 x 4 kernel; 2112 x 132: 33 x 33 = 1089 blocks of the 64 x 4 kernel
SHAPES = [(65, 5), (130, 9), (64, 4), (2112, 132)]
# 33 x 33 = 1089 tiles of the 64 x 32 kernels: the only grid here on which the
# 1024-strided loop over the blocks makes a second round
TALL = (2112, 1028)
# the generator's seed per grid: the first for which, for every kernel, each of
# the two sums tells the orders apart (expected() asserts it)
SEEDS = {(65, 5): 11, (130, 9): 5, (64, 4): 15, (2112, 132): 0, TALL: 0}
ids = lambda s: "x".join(str(v) for v in s) if isinstance(s, tuple) else str(s)  # noqa: E731

# tile height and, per thread row ty, the tile rows it adds, in its order
THREAD_ROWS = {
    "smooth_norm": (32, [[8 * ty + k for k in range(8)] for ty in range(4)]),
    "fluid_step": (32, [[4 * k + ty for k in range(8)] for ty in range(4)]),
    "elastic_logger": (32, [[4 * k + ty for k in range(8)] for ty in range(4)]),
    "curv_construct": (4, [[ty] for ty in range(4)]),
}


def bits(x):
    return np.float64(x).view(np.uint64)


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def fields(dimx, dimy):
    """(prev, new, |prev|, |new - prev|): float32 [dimy, dimx, 2] fields and the
    exact fp64 magnitudes, read-only."""
    rng = np.random.default_rng(SEEDS[(dimx, dimy)])
    shape = (dimy, dimx)
    scale = np.ldexp(1.0, rng.integers(-20, 31, shape))
    a = rng.integers(1, 1 << 16, shape).astype(np.float64)
    b = rng.integers(1, 1 << 16, shape).astype(np.float64)

    def pair(p, q, m):
        v = np.stack([p * m, q * m], axis=-1) * rng.choice([-1.0, 1.0], shape + (2,))
        swap = rng.integers(0, 2, shape).astype(bool)
        v[swap] = v[swap][:, ::-1]
        return v * scale[..., None]

    prev64, d64 = pair(3.0, 4.0, a), pair(5.0, 12.0, b)
    prev, new = prev64.astype(F), (prev64 + d64).astype(F)
    # the float32 fields and the float32 difference the kernels take are exact
    assert np.array_equal(prev.astype(np.float64), prev64)
    assert np.array_equal(new.astype(np.float64), prev64 + d64)
    assert np.array_equal((new - prev).astype(np.float64), d64)
    mp, md = 5.0 * a * scale, 13.0 * b * scale
    # ... and so are the squares' sums, whose roots the magnitudes are
    assert np.array_equal(mp * mp, (prev64 ** 2).sum(-1))
    assert np.array_equal(md * md, (d64 ** 2).sum(-1))
    for x in (prev, new, mp, md):
        x.setflags(write=False)
    return prev, new, mp, md


# ------------------------------------------------------------------ the model
def tree(v):
    """Lane 0 of the __shfl_down tree over the last axis (64 lanes)."""
    v = v.copy()
    for off in (32, 16, 8, 4, 2, 1):
        v[..., :off] += v[..., off:2 * off]
    return v[..., 0]


def waves_in_order(w, reverse=False):
    """The last axis (the waves) added first to last."""
    order = range(w.shape[-1])[::-1] if reverse else range(w.shape[-1])
    acc = None
    for k in order:
        acc = w[..., k].copy() if acc is None else acc + w[..., k]
    return acc


def block_partials(terms, kernel, reverse=False):
    """Per-block sums of a [dimy, dimx] array of terms, blocks in by * gx + bx order."""
    th, rows = THREAD_ROWS[kernel]
    dimy, dimx = terms.shape
    gy, gx = -(-dimy // th), -(-dimx // 64)
    t = np.zeros((gy * th, gx * 64))
    t[:dimy, :dimx] = terms
    t = t.reshape(gy, th, gx, 64)
    wave = []
    for mine in rows:  # one wave per thread row
        acc = np.zeros((gy, gx, 64))
        for r in mine:
            acc = acc + t[:, r]
        wave.append(tree(acc))
    return waves_in_order(np.stack(wave, axis=-1), reverse).reshape(-1)


def strided_sum(part, reverse=False):
    """reduce_partials_kernel: 1024 threads over the blocks."""
    n = -(-part.size // 1024) * 1024
    p = np.zeros(n)
    p[:part.size] = part
    acc = np.zeros(1024)
    for row in p.reshape(-1, 1024):
        acc = acc + row
    return float(waves_in_order(tree(acc.reshape(16, 64)), reverse))


def host_sum(part, reverse=False):
    acc = 0.0
    for x in (part[::-1] if reverse else part):
        acc += float(x)
    return acc


def model(terms, kernel, reverse=False):
    final = host_sum if kernel == "curv_construct" else strided_sum
    return final(block_partials(terms, kernel, reverse), reverse)


def expected(kernel, dimx, dimy):
    """The model's (sum |new - prev|, sum |prev|), after the CPU check that
    the input tells orders apart."""
    _, _, mp, md = fields(dimx, dimy)
    want = []
    for t in (md, mp):
        m = model(t, kernel)
        others = (float(np.sum(t)), model(t, kernel, reverse=True))
        assert any(bits(o) != bits(m) for o in others), "the input does not depend on the order"
        want.append(m)
    return tuple(want)


def check(got, kernel, dimx, dimy):
    want = expected(kernel, dimx, dimy)
    print(f"{kernel} {dimx}x{dimy}: got {got[0].hex()} {got[1].hex()} "
          f"want {want[0].hex()} {want[1].hex()}")
    assert (bits(got[0]), bits(got[1])) == (bits(want[0]), bits(want[1]))


# ------------------------------------------------------------------ CPU: the model itself
def test_model_orders():
    """The model's pieces on a case small enough to write out."""
    v = np.arange(64, dtype=np.float64)
    assert tree(v) == v.sum()  # exact integers: any order
    t = np.zeros((4, 64))
    t[0, 0], t[1, 0], t[2, 0], t[3, 0] = 2.0 ** 53, 1.0, 1.0, 2.0
    # curv_construct: rows are waves, ((2^53 + 1) + 1) + 2 loses both ones
    assert model(t, "curv_construct") == 2.0 ** 53 + 2.0
    assert model(t, "curv_construct", reverse=True) == 2.0 ** 53 + 4.0
    # fluid_step: rows 0..3 belong to four different waves, the same sum
    big = np.zeros((32, 64))
    big[:4] = t
    assert model(big, "fluid_step") == 2.0 ** 53 + 2.0
    # smooth_norm: rows 0..7 are one thread's, added in row order
    assert model(big, "smooth_norm") == 2.0 ** 53 + 2.0
    big[:4] = t[::-1]
    assert model(big, "smooth_norm") == 2.0 ** 53 + 4.0


def test_strided_sum_order():
    p = np.zeros(2049)
    p[0], p[1024], p[2048] = 1.0, 1.0, 2.0 ** 53  # one thread's three blocks
    assert strided_sum(p) == 2.0 ** 53 + 2.0
    p[0], p[2048] = p[2048], p[0]
    assert strided_sum(p) == 2.0 ** 53


ODD_WIDTHS = range(1, 16, 2)
# from the smallest sigma whose 2 sigma^2 is not 0 in float32 (below it the
# table is NaN, which is not 1 either: the runtime-width kernel takes it) to
# the largest whose 2 sigma^2 is finite
SIGMA_SWEEP = [1e-20, 1e-10, 1e-3, 0.05, 0.3, 0.5, 0.8, 1.0, 1.5, 2.5, 4.0, 7.3, 10.0, 33.0,
               1e3, 1e6, 1e12, 1e19]


@pytest.mark.parametrize("kw", ODD_WIDTHS)
def test_odd_gaussian_weight_sum_rounds_to_float_one(kw):
    """The direct kernels of a compile-time (odd) width keep the accumulator
    as the result: the reference would divide it by (float) of the fp64 sum of
    the table in its tap order, which is 1.  The host checks the same per call
    and takes the runtime-width kernel, which divides, otherwise."""
    from oracle import oracle as O
    c = (kw - 1) // 2
    for sigma in SIGMA_SWEEP:
        k = np.zeros(kw * kw, np.float64)
        O.lib().oracle_gaussian_kernel(kw, float(sigma), k)
        w = 0.0
        for ii in range(-c, c + 1):  # Field.tpp:242-256, full_weight
            for jj in range(-c, c + 1):
                w += float(k[(ii + c) + (jj + c) * kw])
        assert F(w) == F(1.0), (kw, sigma, w)


# ------------------------------------------------------------------ GPU
DEMONS = [(3, 0), (4, 0), (3, 1)]  # (kw, method): compile-time, runtime, separable


@gpu_test
@pytest.mark.parametrize("kw,method", DEMONS, ids=["kw3", "kw4", "sep3"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_smooth_norm_sums(shape, kw, method):
    dimx, dimy = shape
    prev, new, _, _ = fields(dimx, dimy)
    out, sums, path = prim.smooth_norm(new, prev, kw, 0.05, partials=True, method=method)
    assert path == method
    assert np.array_equal(out.view(np.uint32), new.view(np.uint32))  # the unit impulse
    check(sums, "smooth_norm", dimx, dimy)


@gpu_test
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_curv_construct_sums(shape):
    dimx, dimy = shape
    prev, new, _, _ = fields(dimx, dimy)
    z = np.ascontiguousarray(np.moveaxis(new.astype(np.float64), -1, 0))
    out, sums = prim.curv_construct(z, prev, 1.0)
    assert np.array_equal(out, new)
    check(sums, "curv_construct", dimx, dimy)


@gpu_test
@pytest.mark.parametrize("own_prev", [False, True], ids=["prev-is-u", "prev-given"])
@pytest.mark.parametrize("shape", SHAPES + [TALL], ids=ids)
def test_fluid_step_sums(shape, own_prev):
    """uo = u + R dt with u = prev, R = new - prev, dt = 1; the Logger's prev is
    u itself or a field of its own (the kernel's two instantiations)."""
    dimx, dimy = shape
    prev, new, _, _ = fields(dimx, dimy)
    zero = np.zeros((dimy, dimx, 2), F)
    res = prim.fluid_step(prev, new - prev, zero, zero[..., 0], zero, 1.0,
                          prev=prev.copy() if own_prev else None)
    assert np.array_equal(res["uo"], new)
    check(res["sums"], "fluid_step", dimx, dimy)


@gpu_test
@pytest.mark.parametrize("shape", SHAPES + [TALL], ids=ids)
def test_elastic_logger_sums(shape):
    dimx, dimy = shape
    prev, new, _, _ = fields(dimx, dimy)
    u, pv, sums = prim.elastic_logger(new, prev)
    assert np.array_equal(u, new) and np.array_equal(pv, new)
    check(sums, "elastic_logger", dimx, dimy)
