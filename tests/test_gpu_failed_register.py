"""Failed registrations: one zero denominator among good pixels, and the state
an object holds afterwards.

The only error the reference defines for its solvers is coord2d's "Divide by
zero exception" (coord2d.h:95-100): Horn-Schunck divides by alpha^2 + gx^2 +
gy^2 (OpticalFlowDiffusion.cpp:78), Demons by gx^2 + gy^2 + It^2 si^2 / sx^2
(Demons.cpp:57).  The older tests raise it with images where almost every
pixel is bad and assert only that something was raised.  Here exactly ONE pixel
of a textured pair has the zero denominator, at the places where a detection
mask, a ragged last wave or a tile could lose it, and every path that carries
the flag must report it; the same path on the unedited pair at alpha = 0 (where
the zero-filled pitch padding and the ghost j-lines have a denominator of
exactly 0) must not raise and must give the oracle's bits.  Then the object is
used again and held to the oracle driven through the same calls.

Bar: no tolerance.  Motion, warp and Logger errors on the float32 bits,
iteration counts and printed "Iteration:" lines equal.

Inputs (checked without a GPU by test_hs_inputs_*, test_demons_inputs_*):
  HS      S.texture_pair in float32, alpha = 0; the planted pixel (px, j) has
          the neighbours that gradients.h:9-32 reads made equal in the moving
          image (interior: px - 1 and px + 1; first column: px and px + 1; last
          column: px - 1 and px; the same along y), so partial_x = partial_y =
          0 there on the image warped by the zero motion.  (0 + gx^2) + gy^2 is
          0 at that pixel and nowhere else; the unedited pair has no zero.
  Demons  the same edit and Iref = Imov at the pixel.
  patch   what survives a warm start: register(good) leaves a motion, so the
          next call warps the moving image and a one-pixel edit is smeared
          away.  The state tests that fail after a good call use a 14 x 14
          flat patch in the moving image (HS) or in both images (Demons), whose
          interior stays flat under the warp.  Many zeros, on purpose.
  level0  HS, one pyramid level below: ref = mov + d with d = +-1/8 in a
          checkerboard, all values multiples of 2^-10, so the 2 x 2 box means
          (Field.tpp:75-143) of ref and mov are equal floats, the coarse It is
          0, the coarse motion stays 0 and the planted pixel survives to level
          0: the coarse loop finishes and level 0 throws.

Throws after iteration 0.  Horn-Schunck's denominator does not change inside a
loop.  For Demons ten candidates were run on the oracle with 20 fixed
iterations (a 12, 16 or 20 px square on a 32^2 or 40 x 33 background: 1.0 on 0
in the reference, 0.75 or 0.9 on 0.1, 0.25 or 0.5 in the moving image, shifted
by (2, 1) or (1, 0), so that It != 0 on every pixel at iteration 0; see
AFTER0_CANDIDATES): test_demons_candidates_after_iteration_0 records what they
do.  None of them raises at all (with the square at 1.0 in both images each
raises at iteration 0, where the squares overlap), so there is no such case
below.

Logger modes of the state tests: fixed_iters, the default exact Logger (HS:
the pipelined loop, chunk 1, 7, 32) and logger_fp64.  With fixed_iters and
with logger_fp64 the device sums the norms in fp64 as a tree, the oracle in
pixel order, so in those two modes motion, warp and counts are the oracle's
(oracle_set_logger_fp64 for the second) and the errors and printed lines are
those of a second device object that went through the same calls without the
failing ones (nscales 0, where the reference leaves nothing of a failed call
behind).
"""
import functools
import threading

import numpy as np
import pytest

from opticalflow2d_amd import synthetic as S

F = np.float32
MSG = "Divide by zero exception"
CONV_CAP = 40
G_BIG, G_SMALL, G_GROUP = (130, 97), (67, 50), (130, 100)
SEED = {G_BIG: 31, G_SMALL: 32, G_GROUP: 33, (1, 40): 34, (2, 40): 35, (330, 40): 36,
        (70, 37): 37}
THIRION = [1.0, 0.25, 1.5, 2.5, 5, 0]
DIFFEO = [1.0, 2.0, 1.0, 1.0, 5]


def ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def good(dims, k=0):
    """A textured pair of float32 values as float64 [dimx, dimy]; k picks
    another pair of the same grid."""
    nx, ny = dims
    n = max(nx, 8)
    r, m = S.texture_pair(n, seed=SEED[dims] + 100 * k, sigma=2.0,
                          shift=(0.6 + 0.2 * k, -0.4), ny=max(ny, 8))
    r, m = r[:nx, :ny].astype(F).astype(np.float64), m[:nx, :ny].astype(F).astype(np.float64)
    return ro(np.ascontiguousarray(r), np.ascontiguousarray(m))


def flatten_gradient(mov, px, j):
    """Make partial_x and partial_y of gradients.h zero at (px, j)."""
    nx, ny = mov.shape
    if nx == 1:
        # one column: partial_x's first branch reads idx + 1, the next j-line
        assert 0 < j < ny - 1
        mov[0, j + 1] = mov[0, j]
        mov[0, j - 1] = mov[0, j]
        return
    if px == 0:
        mov[1, j] = mov[0, j]
    elif px == nx - 1:
        mov[nx - 2, j] = mov[nx - 1, j]
    else:
        mov[px + 1, j] = mov[px - 1, j]
    if j == 0:
        mov[px, 1] = mov[px, 0]
    elif j == ny - 1:
        mov[px, ny - 2] = mov[px, ny - 1]
    else:
        mov[px, j + 1] = mov[px, j - 1]


@functools.lru_cache(maxsize=None)
def planted(dims, px, j, demons=False):
    ref, mov = (a.copy() for a in good(dims))
    flatten_gradient(mov, px, j)
    if demons:
        ref[px, j] = mov[px, j]
    return ro(ref, mov)


def hs_positions(dims):
    """The corners; columns 63, 64, 127, 128 and the last on an interior row;
    rows 15, 16 and the last on an interior column."""
    nx, ny = dims
    row, col = ny // 2 + 1, 40
    pos = [(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)]
    pos += [(c, row) for c in (63, 64, 127, 128, nx - 1) if c < nx]
    pos += [(col, r) for r in (15, 16, ny - 1)]
    return pos


HS_CASES = [(d, p) for d in (G_BIG, G_SMALL) for p in hs_positions(d)]
BATCH_POS = [(0, 0), (66, 0), (0, 49), (66, 49), (63, 26), (64, 26)]
# Demons: (330, 40) runs the fused kernel, (70, 37) the unfused ones
DEMONS_CASES = [((70, 37), (0, 0)),     # a corner
                ((70, 37), (30, 31)),   # the last row of a 32-row tile
                ((330, 40), (100, 20)),  # an x-interior tile of the fused kernel
                ((330, 40), (325, 20))]  # its last tile column, whose taps wrap


@functools.lru_cache(maxsize=None)
def patch_pair(dims, demons=False):
    """The good pair k = 1 with a 14 x 14 flat patch."""
    ref, mov = (a.copy() for a in good(dims, 1))
    x0, y0 = dims[0] // 2 - 7, dims[1] // 2 - 7
    mov[x0:x0 + 14, y0:y0 + 14] = 0.5
    if demons:
        ref[x0:x0 + 14, y0:y0 + 14] = 0.5
    return ro(ref, mov)


@functools.lru_cache(maxsize=None)
def level0_pair(dims, px, j):
    """The module docstring's "level0": the coarse level's It is exactly 0."""
    nx, ny = dims
    _, m = good(dims, 2)
    mov = np.round(m * 1024.0) / 1024.0
    flatten_gradient(mov, px, j)
    x, y = np.arange(nx)[:, None], np.arange(ny)[None, :]
    ref = mov + 0.125 * np.where((x + y) % 2 == 0, 1.0, -1.0)
    assert np.array_equal(ref.astype(F), ref) and np.array_equal(mov.astype(F), mov)
    return ro(np.ascontiguousarray(ref), np.ascontiguousarray(mov))


# ------------------------------------------------------------------ oracle side
def derivatives(oracle, ref, mov):
    """The oracle's (gx, gy, It) as [dimx, dimy] float32 arrays."""
    L = oracle.lib()
    nx, ny = ref.shape
    Im = np.ascontiguousarray(mov.reshape(-1, order="F").astype(F))
    Ir = np.ascontiguousarray(ref.reshape(-1, order="F").astype(F))
    dI = np.zeros(2 * nx * ny + 2, F)[:2 * nx * ny]
    It = np.zeros(nx * ny, F)
    L.oracle_spatial_derivative(Im, nx, ny, dI)
    L.oracle_temporal_derivative(Ir, Im, nx * ny, It)
    g = dI.reshape(ny, nx, 2)
    return g[:, :, 0].T.copy(), g[:, :, 1].T.copy(), It.reshape(ny, nx).T.copy()


def hs_zeros(oracle, ref, mov):
    """Pixels where (0 + gx^2) + gy^2 == 0 in float32 (alpha = 0)."""
    gx, gy, _ = derivatives(oracle, ref, mov)
    return np.argwhere(((F(0) + gx * gx) + gy * gy) == 0)


def demons_zeros(oracle, ref, mov, p):
    gx, gy, It = derivatives(oracle, ref, mov)
    si, sx = F(p[0]) * F(p[0]), F(p[1]) * F(p[1])
    den = gx * gx + gy * gy + It * It * si / sx
    # the oracle's own verdict on the same derivatives
    dI = np.ascontiguousarray(np.stack([gx.T, gy.T], axis=2).reshape(-1))
    c = np.zeros_like(dI)
    rc = oracle.lib().oracle_demons_force(dI, np.ascontiguousarray(It.T.reshape(-1)), It.size,
                                          p[0], p[1], c)
    zeros = np.argwhere(den == 0)
    assert (rc != 0) == (len(zeros) > 0)
    return zeros


class Oracle:
    """oracle.Registration with the calls of ImageRegistration below."""

    def __init__(self, O, dims, niter, nscales, reg, params, verbose=0, fixed=False):
        self.O = O
        self.r = O.Registration(dims, niter, nscales, reg, params, 1, verbose, fixed_iters=fixed)

    def register(self, ref, mov):
        self.r.register(ref, mov)

    def state(self, mov=None):
        out = dict(motion=self.r.motion(), iters=self.r.iterations())
        if mov is not None:
            out.update(warp=self.r.warp(mov), errs=self.r.last_errors())
        return out

    def close(self):
        self.r.close()


def oracle_outcome(O, dims, niter, nscales, reg, params, fixed, calls):
    """Drive a fresh oracle through `calls` [(ref, mov)]: per call "ok" or
    "raise", the state after it and the printed Iteration: lines."""
    L = O.lib()
    o = Oracle(O, dims, niter, nscales, reg, params, 1, fixed)
    out = []
    try:
        for ref, mov in calls:
            L.oracle_clear_output()
            try:
                o.register(ref, mov)
                what = "ok"
            except O.OracleError as e:
                assert MSG in str(e)
                what = "raise"
            st = o.state(mov if what == "ok" else None)
            st["what"] = what
            st["lines"] = [l for l in L.oracle_captured_output().decode().splitlines()
                           if l.startswith("Iteration:")]
            out.append(st)
    finally:
        o.close()
    return out


_WANT = {}


def oracle_hs(O, dims, iters, fixed, pair=None):
    """The oracle on the good pair at alpha = 0, once: motion, warp, counts."""
    key = (dims, iters, fixed, pair is None)
    if key not in _WANT or pair is not None:
        ref, mov = pair or good(dims)
        res = oracle_outcome(O, dims, [iters], 0, 0, [0.0], fixed, [(ref, mov)])[0]
        assert res["what"] == "ok"
        if pair is not None:
            return res
        _WANT[key] = res
    return _WANT[key]


# ------------------------------------------------------------------ CPU part
def test_hs_inputs_have_exactly_one_zero_denominator(oracle):
    from opticalflow2d_amd.slab import halo_rows
    for dims in (G_BIG, G_SMALL, G_GROUP, (2, 40)):
        assert len(hs_zeros(oracle, *good(dims))) == 0, dims
        assert oracle_hs(oracle, dims, 3, True)["motion"].any()
    for dims, (px, j) in HS_CASES + [(G_SMALL, p) for p in BATCH_POS] + group_cases() + \
            [((2, 40), (0, 20))]:
        ref, mov = planted(dims, px, j)
        assert hs_zeros(oracle, ref, mov).tolist() == [[px, j]], (dims, px, j)
        res = oracle_outcome(oracle, dims, [3], 0, 0, [0.0], True, [(ref, mov)])[0]
        assert res["what"] == "raise" and not res["motion"].any()
    # the positions the issue names
    assert [p for d, p in HS_CASES if d == G_BIG][4:9] == [(63, 49), (64, 49), (127, 49),
                                                           (128, 49), (129, 49)]
    assert [p for d, p in HS_CASES if d == G_SMALL][4:7] == [(63, 26), (64, 26), (66, 26)]
    assert halo_rows(100, 0, 2) == (0, 54) and halo_rows(100, 1, 2) == (47, 100)
    assert [p for _, p in group_cases()] == [(40, 49), (40, 50)]
    # one column: the denominators of the j-lines whose gradients the
    # reference defines (the last one reads past the array)
    for pair, want in ((good((1, 40)), []), (planted((1, 40), 0, 20), [[0, 20]])):
        gx, gy, _ = derivatives(oracle, *pair)
        den = ((F(0) + gx * gx) + gy * gy)[:, :39]
        assert np.argwhere(den == 0).tolist() == want


def group_cases():
    """Rank 0's last own row and rank 1's first, from halo_rows: a rank's own
    rows start 3 below its first image row and end 4 above its last."""
    from opticalflow2d_amd.slab import halo_rows
    last0 = halo_rows(G_GROUP[1], 0, 2)[1] - 4 - 1
    first1 = halo_rows(G_GROUP[1], 1, 2)[0] + 3
    return [(G_GROUP, (40, last0)), (G_GROUP, (40, first1))]


def test_demons_inputs_have_exactly_one_zero_denominator(oracle):
    for dims in {d for d, _ in DEMONS_CASES} | {G_SMALL}:
        assert len(demons_zeros(oracle, *good(dims), THIRION)) == 0
        assert len(demons_zeros(oracle, *good(dims), DIFFEO)) == 0
    for dims, (px, j) in DEMONS_CASES + [(G_SMALL, p) for p in BATCH_POS]:
        ref, mov = planted(dims, px, j, True)
        for reg, p in ((3, THIRION), (4, DIFFEO)):
            assert demons_zeros(oracle, ref, mov, p).tolist() == [[px, j]], (dims, px, j)
            res = oracle_outcome(oracle, dims, [3], 0, reg, p, True, [(ref, mov)])[0]
            assert res["what"] == "raise"
    for dims in {d for d, _ in DEMONS_CASES}:
        for reg, p in ((3, THIRION), (4, DIFFEO)):
            res = oracle_outcome(oracle, dims, [4], 0, reg, p, True, [good(dims)])[0]
            assert res["what"] == "ok" and res["motion"].any()
    # (330, 40): dimx >= 128, the fused kernel; the last tile column is 320..329
    assert 325 // 64 == (330 - 1) // 64 and 100 // 64 == 1 and 31 % 32 == 31


AFTER0_CANDIDATES = [
    # dims, square side, background and square value of the moving image, shift
    ((32, 32), 16, 0.1, 0.9, (2, 1)), ((32, 32), 16, 0.25, 0.75, (2, 1)),
    ((32, 32), 16, 0.5, 0.75, (2, 1)), ((32, 32), 12, 0.1, 0.9, (1, 0)),
    ((32, 32), 12, 0.5, 0.9, (1, 0)), ((32, 32), 20, 0.25, 0.9, (2, 1)),
    ((40, 33), 16, 0.1, 0.9, (2, 1)), ((40, 33), 16, 0.5, 0.75, (1, 0)),
    ((40, 33), 12, 0.25, 0.75, (2, 1)), ((40, 33), 20, 0.5, 0.9, (2, 1)),
]


def after0_pair(dims, side, bg, top, shift):
    nx, ny = dims
    x0, y0 = (nx - side) // 2, (ny - side) // 2
    ref = np.zeros(dims)
    ref[x0:x0 + side, y0:y0 + side] = 1.0
    mov = np.full(dims, bg)
    mov[x0 + shift[0]:x0 + shift[0] + side, y0 + shift[1]:y0 + shift[1] + side] = top
    return ref, mov


def first_raise(oracle, dims, pair, cap=20):
    """The iteration at which Thirion's Demons raises on the oracle, or None."""
    res = oracle_outcome(oracle, dims, [cap], 0, 3, THIRION, True, [pair])[0]
    if res["what"] == "ok":
        return None
    for n in range(1, cap + 1):  # the first count that raises: its last iteration
        if oracle_outcome(oracle, dims, [n], 0, 3, THIRION, True, [pair])[0]["what"] == "raise":
            return n - 1
    raise AssertionError("raises with the cap and with no smaller count")


def test_demons_candidates_after_iteration_0(oracle):
    """The module docstring's record: none of the ten raises."""
    got = [first_raise(oracle, c[0], after0_pair(*c)) for c in AFTER0_CANDIDATES]
    assert len(AFTER0_CANDIDATES) == 10
    assert got == [None] * 10, got


# what the state tests drive: name -> (dims, niter, nscales, reg, params, calls)
def sequences(reg):
    demons = reg == 3
    p = THIRION if demons else [0.0]
    d = G_BIG
    g1, g2 = good(d), good(d, 1)
    pixel = planted(d, 64, 49, demons)
    patch = patch_pair(d, demons)
    seq = {
        "good-fail-good": (0, [g1, patch, g2]),
        "fresh-fail-good": (0, [pixel, g2]),
        "fail-twice-good": (0, [pixel, pixel, g2]),
        "good-fail-fail-good": (0, [g1, patch, patch, g2]),
    }
    if not demons:
        lv = level0_pair(d, 64, 49)
        seq["pyramid good-fail-good"] = (1, [g1, patch, g2])
        seq["pyramid fresh-fail-good"] = (1, [lv, g2])
    want = {k: ["raise" if c is patch or c is pixel or (not demons and c is lv) else "ok"
                for c in calls] for k, (_, calls) in seq.items()}
    return d, p, seq, want


NITER = {0: [CONV_CAP, 12], 3: [8, 8]}


@pytest.mark.parametrize("reg", [0, 3])
def test_oracle_sequences_fail_where_planned(oracle, reg):
    d, p, seq, want = sequences(reg)
    for name, (nscales, calls) in seq.items():
        for fixed in (True, False):
            res = oracle_outcome(oracle, d, NITER[reg], nscales, reg, p, fixed, calls)
            assert [r["what"] for r in res] == want[name], (name, fixed)
            assert res[-1]["motion"].any()
            if name == "pyramid fresh-fail-good":
                # the coarse loop finished, level 0 threw
                assert len(res[0]["iters"]) == 1 and res[0]["iters"][0] >= 1
            if name == "pyramid good-fail-good":
                assert res[1]["motion"].any()


# ------------------------------------------------------------------ GPU: detection
def gpu_raises(fn):
    from opticalflow2d_amd import Of2dError, _lib
    with pytest.raises(Of2dError, match=MSG) as e:
        fn()
    assert e.value.status == _lib.OF2D_ERR_RUNTIME


def reg_modes():
    return [dict(fixed_iters=1, hs_gradients_from_image=gi, _iters=n)
            for n in (1, 2, 3, 13) for gi in (0, 1)] + [dict(_iters=CONV_CAP)]


def registration_run(dims, pair, alpha, mode):
    from opticalflow2d_amd import ImageRegistration
    opt = {k: v for k, v in mode.items() if k[0] != "_"}
    with ImageRegistration(dims, [mode["_iters"]], 0, 0, [alpha], **opt) as r:
        r.register(*pair)
        return dict(motion=r.motion(), warp=r.warp(pair[1]), iters=r.iterations())


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [G_BIG, G_SMALL])
def test_registration_good_pair_alpha_zero(gpu, oracle, dims):
    """alpha = 0 where every pixel has a gradient: the padding's and the ghost
    j-lines' 0 / 0 must neither raise nor reach a pixel."""
    for mode in reg_modes():
        fixed = "fixed_iters" in mode
        want = oracle_hs(oracle, dims, mode["_iters"], fixed)
        got = registration_run(dims, good(dims), 0.0, mode)
        assert got["iters"] == want["iters"], mode
        assert same_bits(got["motion"], want["motion"]), mode
        assert same_bits(got["warp"], want["warp"]), mode


@pytest.mark.gpu
@pytest.mark.parametrize("dims, pos", HS_CASES)
def test_registration_detects_one_pixel(gpu, dims, pos):
    """The precheck (every count; it also covers the triple, which has no test
    of its own), the single step and the pair behind it, stored gradients and
    gradients from the image, fixed counts and the exact Logger's loop."""
    pair = planted(dims, *pos)
    for mode in reg_modes():
        gpu_raises(lambda: registration_run(dims, pair, 0.0, mode))


def slab_run(dims, pair, iters, quads):
    from opticalflow2d_amd import SlabSolver
    s = SlabSolver(dims[0], dims[1], 0.0)
    try:
        s.set_option("hs_fixed_quads", quads)
        s.set_images(*pair)
        assert s.info()["iterations_per_launch"] == (4 if quads else 3)
        assert s.run(iters, fixed_iters=True) == iters
        return s.motion()
    finally:
        s.close()


SLAB_MODES = [(q, n) for q in (1, 0) for n in (3, 4, 13)]


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [G_BIG, G_SMALL])
def test_slab_good_pair_alpha_zero(gpu, oracle, dims):
    for quads, iters in SLAB_MODES:
        want = oracle_hs(oracle, dims, iters, True)
        assert same_bits(slab_run(dims, good(dims), iters, quads), want["motion"]), (quads, iters)


@pytest.mark.gpu
@pytest.mark.parametrize("dims, pos", HS_CASES)
def test_slab_detects_one_pixel(gpu, dims, pos):
    """The slab's precheck runs over a field with two ghost j-lines."""
    pair = planted(dims, *pos)
    for quads, iters in SLAB_MODES:
        gpu_raises(lambda: slab_run(dims, pair, iters, quads))


def group_run(dims, calls, iters, split, fixed=True):
    """run_group's pattern (tests/test_gpu_slab_local.py) for calls that may
    fail: per call every rank's exception (or None), and the assembled motion
    of the calls where no rank failed."""
    from opticalflow2d_amd import SlabGroup, SlabSolver
    from opticalflow2d_amd.slab import halo_rows
    from test_gpu_slab_local import can_split
    n = 2
    g = SlabGroup(n)
    slabs = [SlabSolver(dims[0], dims[1], 0.0, r, n, group=g) for r in range(n)]
    out = []
    try:
        for ref, mov in calls:
            for s in slabs:
                s.set_option("split", split)
                lo, hi = halo_rows(dims[1], s.rank, n)
                s.set_images(ref[:, lo:hi], mov[:, lo:hi])
            want = 1 if (split == 1 and can_split(dims[1], n)) else 0
            assert [s.info()["split"] for s in slabs] == [want] * n
            done, errs = [None] * n, [None] * n

            def work(r):
                try:
                    done[r] = slabs[r].run(iters, fixed_iters=fixed)
                except Exception as e:  # compared by the caller
                    errs[r] = e

            th = [threading.Thread(target=work, args=(r,)) for r in range(n)]
            for t in th:
                t.start()
            for t in th:
                t.join(timeout=180)
            assert not any(t.is_alive() for t in th), "a rank did not finish"
            motion = None
            if errs == [None] * n:
                motion = np.concatenate([s.motion() for s in slabs], axis=1)
            out.append((errs, done, motion))
        return out
    finally:
        for s in slabs:
            s.close()
        g.close()


def all_ranks_raised(errs):
    from opticalflow2d_amd import Of2dError, _lib
    for e in errs:
        assert isinstance(e, Of2dError) and MSG in str(e) and e.status == _lib.OF2D_ERR_RUNTIME, errs


@pytest.mark.gpu
@pytest.mark.parametrize("dims, split", [(G_GROUP, 1), (G_GROUP, -1), (G_BIG, -1)])
def test_two_rank_group_every_rank_raises(gpu, oracle, dims, split):
    """A zero on rank 0's last own row or rank 1's first: both ranks raise (the
    vote of slab.cpp), and the good pair runs through.  (130, 100) splits into
    interior and edge launches, (130, 97) cannot."""
    from opticalflow2d_amd.slab import slab_bounds
    rows = [slab_bounds(dims[1], 0, 2)[1] - 1, slab_bounds(dims[1], 1, 2)[0]]
    assert rows[1] == rows[0] + 1
    for iters in (3, 13):
        (errs, done, m), = group_run(dims, [good(dims)], iters, split)
        assert errs == [None, None] and done == [iters, iters]
        assert same_bits(m, oracle_hs(oracle, dims, iters, True)["motion"])
        for j in rows:
            pair = planted(dims, 40, j)
            if iters == 3:
                assert hs_zeros(oracle, *pair).tolist() == [[40, j]]
            (errs, _, _), = group_run(dims, [pair], iters, split)
            all_ranks_raised(errs)


@pytest.mark.gpu
@pytest.mark.parametrize("nx", [1, 2])
def test_narrow_grids(gpu, oracle, nx):
    """(1, 40): single steps only and no precheck, so the single step's own
    test reports; (2, 40): the narrowest grid with the precheck.  On one
    column the reference's gradient of the last j-line reads past the array
    (test_width_one_grid_high_gradients): after k iterations the j-lines below
    40 - k are compared."""
    from opticalflow2d_amd import ImageRegistration
    dims = (nx, 40)
    for iters in (1, 3):
        keep = 40 - iters if nx == 1 else 40
        want = oracle_hs(oracle, dims, iters, True)
        with ImageRegistration(dims, [iters], 0, 0, [0.0], fixed_iters=1) as r:
            r.register(*good(dims))
            got = r.motion()
        # one column at alpha = 0: every update points outside the image and
        # the composition onto the zero motion returns 0 (Motion.cpp:113-178),
        # so there the comparison only says that nothing was raised
        assert want["motion"][:, :keep].any() == (nx == 2)
        assert same_bits(got[:, :keep], want["motion"][:, :keep]), iters
        pair = planted(dims, 0, 20)
        gpu_raises(lambda: registration_run(dims, pair, 0.0, dict(fixed_iters=1, _iters=iters)))


def batch_stack(pos, demons, B=5):
    """Five pairs of (67, 50), the planted one in the middle."""
    refs = np.stack([good(G_SMALL, k)[0] for k in range(B)])
    movs = np.stack([good(G_SMALL, k)[1] for k in range(B)])
    if pos is not None:
        refs[B // 2], movs[B // 2] = planted(G_SMALL, *pos, demons)
    return refs, movs


def batch_oracle(oracle, reg, p, ref, mov, iters):
    res = oracle_outcome(oracle, G_SMALL, [iters], 0, reg, p, True, [(ref, mov)])[0]
    assert res["what"] == "ok"
    return res


def check_batch(oracle, b, reg, p, refs, movs, iters, bad):
    from opticalflow2d_amd import _lib
    B = len(movs)
    want = [_lib.OF2D_OK] * B
    if bad is not None:
        want[bad] = _lib.OF2D_ERR_RUNTIME
    assert b.status().tolist() == want
    if bad is None:
        assert b.last_error() == ""
    else:
        assert MSG in b.last_error() and f"pair {bad}" in b.last_error()
    assert b.info()["threads"] == [1024]
    motion, warp = b.motion(), b.warp(movs)
    for k in range(B):
        if k == bad:
            assert not motion[k].any()
            continue
        key = (reg, k, iters)
        if key not in _WANT:
            _WANT[key] = batch_oracle(oracle, reg, p, refs[k], movs[k], iters)
        assert same_bits(motion[k], _WANT[key]["motion"]), f"pair {k}"
        assert same_bits(warp[k], _WANT[key]["warp"]), f"pair {k}"


@pytest.mark.gpu
@pytest.mark.parametrize("reg", [0, 3])
def test_batch_flags_the_planted_pair_alone_and_recovers(gpu, oracle, reg):
    """A pair's workgroup walks pixels t, t + 1024, ...: the corners and
    columns 63 / 64.  Then the same object registers five good pairs: every
    pair, the one that failed included, is the oracle's and no status is left."""
    from opticalflow2d_amd import BatchRegistration
    demons = reg == 3
    p, iters = (THIRION if demons else 0.0), 5
    op = THIRION if demons else [0.0]
    with BatchRegistration(5, G_SMALL, [iters], 0, p, 1, reg=reg, device=0, fixed_iters=1) as b:
        for pos in BATCH_POS:
            refs, movs = batch_stack(pos, demons)
            b.register(refs, movs)
            check_batch(oracle, b, reg, op, refs, movs, iters, 2)
            refs, movs = batch_stack(None, demons)
            b.register(refs, movs)
            check_batch(oracle, b, reg, op, refs, movs, iters, None)
            assert b.iterations().tolist() == [[iters]] * 5


def demons_run(dims, pair, reg, p, iters, sep):
    from opticalflow2d_amd import ImageRegistration
    with ImageRegistration(dims, [iters], 0, reg, p, fixed_iters=1, demons_separable=sep) as r:
        try:
            r.register(*pair)
            return dict(motion=r.motion(), warp=r.warp(pair[1]), iters=r.iterations())
        finally:
            assert r.demons_paths() == [(dims[0], dims[1], 5, sep)]


@pytest.mark.gpu
@pytest.mark.parametrize("reg, sep", [(3, 0), (3, 1), (4, 0)])
@pytest.mark.parametrize("dims, pos", DEMONS_CASES)
def test_demons_detects_one_pixel(gpu, oracle, dims, pos, reg, sep):
    """The unfused force kernel ((70, 37)) and the fused kernel ((330, 40)),
    with the path record of the loop that ran."""
    p = THIRION if reg == 3 else DIFFEO
    for iters in (1, 4):
        gpu_raises(lambda: demons_run(dims, planted(dims, *pos, True), reg, p, iters, sep))
    if sep == 0:  # the separable form rounds differently by design
        want = oracle_outcome(oracle, dims, [4], 0, reg, p, True, [good(dims)])[0]
        got = demons_run(dims, good(dims), reg, p, 4, sep)
        assert got["iters"] == want["iters"]
        assert same_bits(got["motion"], want["motion"]) and same_bits(got["warp"], want["warp"])


# ------------------------------------------------------------------ GPU: state
def device_outcome(gpu, dims, niter, nscales, reg, params, calls, skip=(), **opt):
    """ImageRegistration through `calls` (but those in `skip`), as oracle_outcome."""
    from opticalflow2d_amd import ImageRegistration, Of2dError
    out = []
    with ImageRegistration(dims, niter, nscales, reg, params, 1, 1, **opt) as r:
        for n, (ref, mov) in enumerate(calls):
            if n in skip:
                out.append(None)
                continue
            gpu.clear()
            try:
                r.register(ref, mov)
                what = "ok"
            except Of2dError as e:
                assert MSG in str(e)
                what = "raise"
            st = dict(what=what, motion=r.motion(), iters=r.iterations())
            if what == "ok":
                st.update(warp=r.warp(mov), errs=r.last_errors())
            st["lines"] = [l for l in "".join(gpu).splitlines() if l.startswith("Iteration:")]
            out.append(st)
    return out


STATE_MODES = [("fixed", dict(fixed_iters=1)), ("exact", {}), ("chunk1", dict(chunk=1)),
               ("chunk7", dict(chunk=7)), ("chunk32", dict(chunk=32)),
               ("fp64", dict(logger_fp64=1))]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [m for m, _ in STATE_MODES])
@pytest.mark.parametrize("reg", [0, 3])
def test_state_after_a_failed_register(gpu, oracle, reg, mode):
    """ImageRegistration.cpp:133-156: the accumulate comes after the loop, so
    the level that threw keeps its motion, the levels that finished before it
    stay accumulated and upsampled, and iterations() holds the loops that
    finished.  The object and the oracle go through the same calls; after each
    one motion and counts are compared, after each good one warp, errors and
    the printed lines too."""
    opt = dict(STATE_MODES)[mode]
    fixed, fp64 = mode == "fixed", mode == "fp64"
    tree = fixed or fp64  # the Logger sums are the device's fp64 tree
    d, p, seq, want = sequences(reg)
    L = oracle.lib()
    for name, (nscales, calls) in seq.items():
        L.oracle_set_logger_fp64(1 if fp64 else 0)
        try:
            exp = oracle_outcome(oracle, d, NITER[reg], nscales, reg, p, fixed, calls)
        finally:
            L.oracle_set_logger_fp64(0)
        got = device_outcome(gpu, d, NITER[reg], nscales, reg, p, calls, **opt)
        clean = None
        if tree and nscales == 0:
            bad = [n for n, w in enumerate(want[name]) if w == "raise"]
            clean = device_outcome(gpu, d, NITER[reg], nscales, reg, p, calls, skip=bad, **opt)
        for n, (g, e) in enumerate(zip(got, exp)):
            at = f"{name}, call {n}"
            assert g["what"] == e["what"] == want[name][n], at
            assert g["iters"] == e["iters"], at
            assert same_bits(g["motion"], e["motion"]), at
            if g["what"] == "raise":
                continue
            assert same_bits(g["warp"], e["warp"]), at
            if not tree:
                assert same_bits(g["errs"], e["errs"]), at
                assert g["lines"] == e["lines"] and len(g["lines"]) >= 1, at
            elif clean is not None:
                assert same_bits(g["errs"], clean[n]["errs"]), at
                assert g["lines"] == clean[n]["lines"], at
                assert same_bits(g["motion"], clean[n]["motion"]), at


@pytest.mark.gpu
def test_slab_after_a_failed_run(gpu, oracle):
    """set_images(planted), run raises; set_images(good), run on the same slab
    is a fresh slab's run (and the oracle's), fixed and with the Logger."""
    from opticalflow2d_amd import SlabSolver
    d = G_BIG
    s, fresh = SlabSolver(d[0], d[1], 0.0), SlabSolver(d[0], d[1], 0.0)
    try:
        for fixed, iters in ((True, 13), (False, CONV_CAP)):
            for pos in ((64, 49), (129, 96)):
                s.set_images(*planted(d, *pos))
                gpu_raises(lambda: s.run(iters, fixed_iters=fixed))
            s.set_images(*good(d))
            fresh.set_images(*good(d))
            want = oracle_hs(oracle, d, iters, fixed)
            assert [s.run(iters, fixed_iters=fixed)] == want["iters"]
            assert fresh.run(iters, fixed_iters=fixed) == want["iters"][0]
            assert same_bits(s.motion(), want["motion"])
            assert same_bits(fresh.motion(), want["motion"])
            if not fixed:
                assert same_bits(s.errors(), fresh.errors())
                assert same_bits(s.errors(), want["errs"])
    finally:
        s.close()
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fixed, iters", [(True, 13), (False, CONV_CAP)])
def test_group_after_a_failed_run(gpu, oracle, fixed, iters):
    """The same on two ranks that split: fail, fail on the other rank's row,
    then the good pair on the same slabs."""
    d = G_GROUP
    (_, p0), (_, p1) = group_cases()
    res = group_run(d, [planted(d, *p0), planted(d, *p1), good(d)], iters, 1, fixed)
    all_ranks_raised(res[0][0])
    all_ranks_raised(res[1][0])
    errs, done, m = res[2]
    want = oracle_hs(oracle, d, iters, fixed)
    assert errs == [None, None] and done == want["iters"] * 2
    assert same_bits(m, want["motion"])


@pytest.mark.gpu
def test_gateway_handle_survives_a_failed_call(gpu, oracle):
    """of2d_gateway: the failing register returns OF2D_ERR_RUNTIME with the
    reference's string, the singleton's next calls succeed and are the
    oracle's after the same calls."""
    from opticalflow2d_amd import OpticalFlow2d
    d = G_BIG
    bad, ok = planted(d, 64, 49), good(d, 1)
    exp = oracle_outcome(oracle, d, [CONV_CAP], 0, 0, [0.0], False, [bad, ok])
    assert [e["what"] for e in exp] == ["raise", "ok"]
    OpticalFlow2d(list(d), [CONV_CAP], 0, 0, [0.0], 1, 1, 0)
    try:
        gpu_raises(lambda: OpticalFlow2d(*bad))
        assert same_bits(OpticalFlow2d(nargout=1), exp[0]["motion"])
        OpticalFlow2d(*ok)
        assert same_bits(OpticalFlow2d(nargout=1), exp[1]["motion"])
        assert same_bits(OpticalFlow2d(ok[1], nargout=1), exp[1]["warp"])
    finally:
        OpticalFlow2d()
