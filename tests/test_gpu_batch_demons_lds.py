"""The batch option "conv_lds" on the device (BatchRegistration reg=3 with
conv_lds=1): the Demons loop with the field its two
convolutions read in one LDS plane.  Every result is held, with
np.array_equal, to the oracle, to the one-pair ImageRegistration and to the
same batch with conv_lds=0: fixed iterations at the sizes where the kernel
takes another path, a pyramid with refines and one with mixed placement, the
diffeomorphic loop, convergence per pair (counts and errors on their bits), a
divide-by-zero pair, a NaN pixel, more pairs than workgroup slots, the option
switched on one handle, a warm start and device tensors.
info()["placement"] is exactly what the fit rule predicts."""
import numpy as np
import pytest

from opticalflow2d_amd import synthetic as S

pytestmark = pytest.mark.gpu

REG = 3       # the batch's method
ONE_PAIR_DIFFEO = 4  # DemonsDiffeomorphic, the one-pair method of diffeomorphic=1

# [sigma_i, sigma_x, sigma_diffusion, sigma_fluid, kernel_width] of
# test_gpu_batch_diffeo.py: QUIET takes no squaring in any iteration, LIVE 0, 1
# or 2
QUIET = [1.0, 0.25, 1.5, 2.5, 5]
LIVE = [1.0, 2.0, 1.0, 1.0, 5]


def params(kw=5, accum=0, sigma_x=0.25):
    return [1.0, sigma_x, 1.5, 2.5, kw, accum]


def level_dims(dims, nscales):
    """ImageRegistration.cpp:56-61: dim / scale with a float scale, per level."""
    return [(int(np.float32(dims[0]) / np.float32(2.0 ** s)),
             int(np.float32(dims[1]) / np.float32(2.0 ** s))) for s in range(nscales + 1)]


def fits(dx, dy):
    """The fit rule of batch_plan.h (conv_lds_fits), restated: the dense plane
    and its dx + 1 elements of slack plus 1 KiB of static LDS within the CU's
    160 KiB, and at most 16 pixels for each of the 1024 threads."""
    return (dx * dy + dx + 1) * 8 + 1024 <= 160 * 1024 and dx * dy <= 16 * 1024


def placement_of(dims, nscales):
    return [1 if fits(dx, dy) else 0 for dx, dy in level_dims(dims, nscales)]


def test_the_fit_rule_restated():
    assert fits(128, 128) and fits(9, 300) and fits(130, 17) and fits(64, 64)
    assert not fits(129, 128) and not fits(150, 120) and not fits(256, 256)
    assert (128 * 128 + 128 + 1) * 8 == 132104
    assert placement_of((200, 180), 2) == [0, 1, 1]


def make_pairs(dims, B, shared=False, seed0=10, extra=0.0):
    """B different textured pairs with different shifts; shared: one reference."""
    dimx, dimy = dims
    refs, movs = [], []
    for k in range(B):
        shift = (0.4 + 0.35 * k + extra, (-0.3 - 0.2 * k if k % 2 else 0.25 + 0.15 * k) - extra)
        r, m = S.texture_pair(dimx, seed=seed0 if shared else seed0 + k, sigma=2.0, shift=shift,
                              ny=dimy)
        refs.append(r)
        movs.append(m)
    return (refs[0] if shared else np.stack(refs)), np.stack(movs)


def ref_of(refs, k):
    return refs if refs.ndim == 2 else refs[k]


def one_pair_method(p, diffeo):
    """The one-pair method and parameters of a batch with parameters p."""
    return (ONE_PAIR_DIFFEO, list(p[:5])) if diffeo else (REG, list(p))


def oracle_pair(O, dims, niter, nscales, p, nrefine, ref, mov, diffeo=False):
    reg, q = one_pair_method(p, diffeo)
    o = O.Registration(dims, niter, nscales, reg, q, nrefine, fixed_iters=True)
    o.register(ref, mov)
    out = o.motion(), o.warp(mov), o.iterations()
    o.close()
    return out


def run_batch(dims, niter, nscales, p, nrefine, refs, movs, **opt):
    from opticalflow2d_amd import BatchRegistration
    with BatchRegistration(len(movs), dims, niter, nscales, p, nrefine, reg=REG, device=0,
                           **opt) as b:
        b.register(refs, movs)
        return {"motion": b.motion(), "warp": b.warp(movs), "iters": b.iterations(),
                "status": b.status(), "info": b.info(), "error": b.last_error(),
                "errs": [b.last_errors(k) for k in range(len(movs))]}


def launches_formula(nscales, nrefine):
    """warp, loop and accumulate per loop; a motion downsample
    per level strictly between the coarsest and level 0, an upsample per level
    above 0; the pass that zeroes failed pairs.  The option adds none."""
    return 3 * (nscales + 1) * nrefine + max(nscales - 1, 0) + nscales + 1


def both(dims, niter, nscales, p, nrefine, refs, movs, **opt):
    """The batch with conv_lds 1 and 0; the placement is the fit rule's."""
    got = run_batch(dims, niter, nscales, p, nrefine, refs, movs, conv_lds=1, **opt)
    glob = run_batch(dims, niter, nscales, p, nrefine, refs, movs, conv_lds=0, **opt)
    assert got["info"]["placement"] == placement_of(dims, nscales)
    assert glob["info"]["placement"] == [0] * (nscales + 1)
    assert got["info"]["threads"] == glob["info"]["threads"] == [1024] * (nscales + 1)
    assert got["info"]["launches"] == glob["info"]["launches"] == launches_formula(nscales, nrefine)
    return got, glob


def check_fixed(oracle, dims, niter, nscales, nrefine, p, refs, movs, got, glob, diffeo=False):
    """got against conv_lds=0, the oracle and the one-pair path."""
    from opticalflow2d_amd import ImageRegistration
    B = len(movs)
    want_iters = [n for n in reversed(niter[: nscales + 1]) for _ in range(nrefine)]
    assert got["status"].tolist() == [0] * B and got["error"] == ""
    assert got["iters"].tolist() == glob["iters"].tolist() == [want_iters] * B
    assert np.array_equal(got["motion"], glob["motion"]), "differs from conv_lds=0"
    assert np.array_equal(got["warp"], glob["warp"])
    reg, q = one_pair_method(p, diffeo)
    for k in range(B):
        m, w, it = oracle_pair(oracle, dims, niter, nscales, p, nrefine, ref_of(refs, k), movs[k],
                               diffeo)
        assert it == want_iters
        # any other accumulation value applies no correction: the motion stays zero
        assert m.any() == (p[5] in (0, 1))
        assert np.array_equal(got["motion"][k], m), f"pair {k}: motion differs from the oracle"
        assert np.array_equal(got["warp"][k], w), f"pair {k}: warp differs from the oracle"
        with ImageRegistration(dims, niter, nscales, reg, q, nrefine, fixed_iters=1,
                               device=0) as r:
            r.register(ref_of(refs, k), movs[k])
            assert np.array_equal(got["motion"][k], r.motion()), f"pair {k}: one-pair path"
            assert np.array_equal(got["warp"][k], r.warp(movs[k]))
        assert got["errs"][k].size == 0  # fixed_iters: no errors recorded


# ------------------------------------------------------------ 1. fixed iterations
FIXED_CASES = [
    # dims, B, niter, nscales, shared reference, parameters
    ((31, 29), 1, [7], 0, False, params()),   # 899 pixels: one per thread at most
    ((31, 29), 3, [7], 0, False, params()),
    ((40, 33), 1, [7], 0, False, params()),   # 1320: up to 4, no multiple of the wave
    ((40, 33), 3, [7], 0, False, params()),
    ((90, 70), 2, [5], 0, False, params()),   # 6300: up to 16, partly filled
    ((128, 128), 2, [3], 0, False, params()),  # the limit: 16 each, the largest plane
    # level 1 is (65, 8); a shared reference; Addition
    ((130, 17), 3, [6, 9], 1, True, params(accum=1)),
    # a kernel wider than the grid: level 1 is (4, 150), its taps wrap twice
    ((9, 300), 2, [5, 6], 1, False, params(kw=15)),
    ((40, 33), 2, [7], 0, False, params(kw=1)),
    # an even width sums a 3 x 3 corner of the 4 x 4 table: the weight sum is
    # not 1 and the interior division is live
    ((40, 33), 2, [7], 0, False, params(kw=4)),
    ((40, 33), 2, [7], 0, False, params(kw=7)),
    ((40, 33), 2, [7], 0, False, params(kw=9)),  # a width that is not compiled in
    ((40, 33), 2, [7], 0, False, params(sigma_x=0.3)),  # sigma_x^2 no power of two
    ((40, 33), 2, [7], 0, False, params(accum=2)),      # neither Composition nor Addition
]


@pytest.mark.parametrize("dims, B, niter, nscales, shared, p", FIXED_CASES)
def test_fixed_iterations_bit_for_bit(gpu, oracle, dims, B, niter, nscales, shared, p):
    refs, movs = make_pairs(dims, B, shared)
    got, glob = both(dims, niter, nscales, p, 1, refs, movs, fixed_iters=1)
    assert got["info"]["placement"] == [1] * (nscales + 1)
    check_fixed(oracle, dims, niter, nscales, 1, p, refs, movs, got, glob)


# ------------------------------------------------------------ 2. pyramids
PYR = dict(dims=(67, 50), niter=[5, 6, 7], nscales=2, nrefine=2)
_cache = {}


def pyramid_case(B=7):
    if B not in _cache:
        refs, movs = make_pairs(PYR["dims"], 7)
        _cache.setdefault("in", (refs, movs))
        _cache[B] = both(PYR["dims"], PYR["niter"], PYR["nscales"], params(), PYR["nrefine"],
                         refs[:B], movs[:B], fixed_iters=1)
    return _cache["in"], _cache[B]


def test_pyramid_two_refines(gpu, oracle):
    (refs, movs), (got, glob) = pyramid_case(7)
    assert got["info"]["placement"] == [1, 1, 1]
    check_fixed(oracle, PYR["dims"], PYR["niter"], PYR["nscales"], PYR["nrefine"], params(), refs,
                movs, got, glob)


def test_pyramid_mixed_placement(gpu, oracle):
    """Level 0 (200, 180) does not fit and runs the global-memory kernel; levels
    1 and 2 run the new one and hand their motion up to it."""
    dims, niter, nscales = (200, 180), [3, 4, 5], 2
    refs, movs = make_pairs(dims, 2)
    got, glob = both(dims, niter, nscales, params(), 1, refs, movs, fixed_iters=1)
    assert got["info"]["placement"] == [0, 1, 1]
    check_fixed(oracle, dims, niter, nscales, 1, params(), refs, movs, got, glob)


def test_launch_count_depends_on_neither_batch_size_nor_option(gpu):
    _, (one, one0) = pyramid_case(1)
    _, (all7, all70) = pyramid_case(7)
    want = launches_formula(PYR["nscales"], PYR["nrefine"])
    assert [r["info"]["launches"] for r in (one, one0, all7, all70)] == [want] * 4 and want == 22
    assert one["info"]["loops"] == all7["info"]["loops"] == 6
    assert np.array_equal(one["motion"][0], all7["motion"][0])  # pairs do not see each other


# ------------------------------------------------------------ 3. diffeomorphic
DIFFEO_CASES = [
    ((40, 33), 3, [7], LIVE),
    ((40, 33), 3, [7], QUIET),  # no squaring in any iteration
    # the last pixels' squaring gathers read the slack past the plane
    ((128, 128), 2, [3], LIVE),
]


@pytest.mark.parametrize("dims, B, niter, p5", DIFFEO_CASES)
def test_diffeomorphic_bit_for_bit(gpu, oracle, dims, B, niter, p5):
    p = list(p5) + [0]
    refs, movs = make_pairs(dims, B)
    got, glob = both(dims, niter, 0, p, 1, refs, movs, fixed_iters=1, diffeomorphic=1)
    assert got["info"]["placement"] == [1]
    check_fixed(oracle, dims, niter, 0, 1, p, refs, movs, got, glob, diffeo=True)
    if p5 is LIVE:  # the squarings ran: Thirion's loop on the same input differs
        thirion = run_batch(dims, niter, 0, p, 1, refs, movs, fixed_iters=1, conv_lds=1)
        assert thirion["info"]["placement"] == [1]
        assert not np.array_equal(thirion["motion"], got["motion"])


# ------------------------------------------------------------ 4. convergence
CONV_INPUTS = [(40, (0.3, 0.2)), (41, (1.1, -0.6)), (43, (0.7, 0.9)), (45, (1.4, 0.8))]


def conv_pairs(dims):
    dimx, dimy = dims
    out = [S.texture_pair(dimx, seed=seed, sigma=2.5, shift=sh, ny=dimy)
           for seed, sh in CONV_INPUTS]
    return np.stack([r for r, _ in out]), np.stack([m for _, m in out])


@pytest.mark.parametrize("dims, niter, nscales", [((48, 40), [200], 0),
                                                  ((67, 50), [200, 200, 200], 2)])
def test_convergence_per_pair(gpu, oracle, dims, niter, nscales):
    """The pixel-to-thread mapping and the reduction tree are conv_lds=0's, so
    the counts and the errors (on their float32 bits) are too; every pair stops
    on its own iteration, and its motion is the oracle's run of those counts."""
    p = params()
    refs, movs = conv_pairs(dims)
    B = len(movs)
    got, glob = both(dims, niter, nscales, p, 1, refs, movs)
    assert got["info"]["placement"] == [1] * (nscales + 1)
    assert got["status"].tolist() == glob["status"].tolist() == [0] * B
    assert np.array_equal(got["iters"], glob["iters"])
    counts = got["iters"].tolist()
    assert len({tuple(c) for c in counts}) == B, counts
    assert all(2 < n < 200 for c in counts for n in c), counts
    for k in range(B):
        assert got["errs"][k].size == counts[k][-1]
        assert np.array_equal(got["errs"][k].view(np.uint32), glob["errs"][k].view(np.uint32)), k
        # the oracle's fixed run with the pair's counts (niter is finest level first)
        m, w, _ = oracle_pair(oracle, dims, counts[k][::-1], nscales, p, 1, refs[k], movs[k])
        assert np.array_equal(got["motion"][k], m), f"pair {k}"
        assert np.array_equal(got["warp"][k], w), f"pair {k}"
    assert np.array_equal(got["motion"], glob["motion"])


# ------------------------------------------------------------ 5. divide by zero
def test_divide_by_zero_is_per_pair(gpu, oracle):
    from opticalflow2d_amd import BatchRegistration, _lib
    dims, niter, p = (40, 33), [5], params()
    good_refs, good_movs = make_pairs(dims, 4)
    refs, movs = good_refs.copy(), good_movs.copy()
    bad = 2
    refs[bad] = 0.5  # no gradient, and Iref = Imov
    movs[bad] = 0.5
    with BatchRegistration(4, dims, niter, 0, p, 1, reg=REG, device=0, fixed_iters=1,
                           conv_lds=1) as b:
        b.register(refs, movs)
        status, error, motion, warped = b.status().tolist(), b.last_error(), b.motion(), b.warp(movs)
        assert b.info()["placement"] == [1]
        iters = b.iterations().tolist()
        # the next estimate on the handle is clean
        b.register(good_refs, good_movs)
        assert b.status().tolist() == [0] * 4 and b.last_error() == ""
        again = b.motion()
    want = [_lib.OF2D_OK] * 4
    want[bad] = _lib.OF2D_ERR_RUNTIME
    assert status == want
    assert "Divide by zero exception" in error and f"pair {bad}" in error
    assert not motion[bad].any()
    assert iters == [[5], [5], [0], [5]]
    for k in range(4):
        m, w, _ = oracle_pair(oracle, dims, niter, 0, p, 1, good_refs[k], good_movs[k])
        assert np.array_equal(again[k], m), f"pair {k}: the estimate after the failure"
        if k != bad:
            assert np.array_equal(motion[k], m), f"pair {k}"
            assert np.array_equal(warped[k], w), f"pair {k}"


# ------------------------------------------------------------ 6. a NaN pixel
def same_bits_and_nans(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na],
                                                     b.view(np.uint64)[~nb])


@pytest.mark.parametrize("diffeo", [0, 1])
def test_nan_pixel_as_conv_lds_0(gpu, diffeo):
    dims, niter = (40, 33), [4]
    p = (LIVE + [0]) if diffeo else params()
    refs, movs = make_pairs(dims, 3)
    bad = 1
    movs_nan = movs.copy()
    movs_nan[bad, 17, 12] = np.nan
    got, glob = both(dims, niter, 0, p, 1, refs, movs_nan, fixed_iters=1, diffeomorphic=diffeo)
    assert got["status"].tolist() == glob["status"].tolist() == [0, 0, 0]
    assert np.isnan(glob["warp"][bad]).any() and not np.isnan(glob["warp"][bad]).all()
    for k in range(3):
        assert same_bits_and_nans(got["motion"][k], glob["motion"][k]), k
        assert same_bits_and_nans(got["warp"][k], glob["warp"][k]), k
    clean = run_batch(dims, niter, 0, p, 1, refs, movs, fixed_iters=1, diffeomorphic=diffeo,
                      conv_lds=1)
    assert not same_bits_and_nans(clean["motion"][bad], got["motion"][bad])
    for k in (0, 2):
        assert np.array_equal(got["motion"][k], clean["motion"][k])


# ------------------------------------------------------------ 7. many pairs
MANY_SHIFTS = [(0.5, 0.25), (-0.75, 0.5), (1.25, -0.9), (0.1, 0.9), (0.6, -0.4), (-0.3, 0.8),
               (0.9, 1.1), (-1.1, -0.2)]


def test_more_pairs_than_workgroup_slots(gpu, oracle):
    """600 workgroups of 1024 threads: a CU holds 32 waves, two such
    workgroups, so the 256 CUs hold 512 at a time and the grid takes a second
    round of blocks."""
    dims, niter, B, p = (40, 33), [3], 600, params()
    eight = [S.texture_pair(40, seed=7 + k // 4, sigma=2.0, shift=sh, ny=33)
             for k, sh in enumerate(MANY_SHIFTS)]
    # on the CPU first: the oracle takes every one of the eight
    want = [oracle_pair(oracle, dims, niter, 0, p, 1, r, m) for r, m in eight]
    which = (np.arange(B) * 5 + np.arange(B) // 256) % 8
    assert which[0] == 0 and len(set(which.tolist())) == 8
    refs = np.stack([eight[w][0] for w in which])
    movs = np.stack([eight[w][1] for w in which])
    got = run_batch(dims, niter, 0, p, 1, refs, movs, fixed_iters=1, conv_lds=1)
    assert not got["status"].any()
    assert got["info"]["placement"] == [1] and got["info"]["threads"] == [1024]
    assert got["info"]["launches"] == launches_formula(0, 1)
    for w in range(8):
        sel = np.flatnonzero(which == w)
        assert sel.size > 50
        m, wimg, _ = want[w]
        assert m.any()
        assert np.array_equal(got["motion"][sel], np.broadcast_to(m, (sel.size,) + m.shape))
        assert np.array_equal(got["warp"][sel], np.broadcast_to(wimg, (sel.size,) + wimg.shape))


# ------------------------------------------------------------ 8. options on one handle
def test_switching_on_one_handle(gpu, oracle):
    from opticalflow2d_amd import BatchRegistration
    dims, niter, nscales, p = (130, 17), [6, 9], 1, params()
    refs, movs = make_pairs(dims, 3)
    with BatchRegistration(3, dims, niter, nscales, p, 1, reg=REG, device=0, fixed_iters=1,
                           conv_lds=1) as b:
        b.register(refs, movs)
        first, p1 = b.motion(), b.info()["placement"]
        b.set_option("conv_lds", 0)
        b.register(refs, movs)
        second, p2 = b.motion(), b.info()["placement"]
        b.set_option("conv_lds", 1)
        b.register(refs, movs)
        third, p3 = b.motion(), b.info()["placement"]
    assert (p1, p2, p3) == ([1, 1], [0, 0], [1, 1])
    assert np.array_equal(first, second) and np.array_equal(first, third)
    m, _, _ = oracle_pair(oracle, dims, niter, nscales, p, 1, refs[1], movs[1])
    assert np.array_equal(first[1], m)


def test_warm_start_two_frames(gpu):
    from opticalflow2d_amd import BatchRegistration
    dims, niter, p = (40, 33), [7], params()
    refs, movs1 = make_pairs(dims, 3)
    _, movs2 = make_pairs(dims, 3, extra=0.3)
    out = {}
    for conv_lds in (1, 0):
        with BatchRegistration(3, dims, niter, 0, p, 1, reg=REG, device=0, fixed_iters=1,
                               warm_start=1, conv_lds=conv_lds) as b:
            b.register(refs, movs1)
            one = b.motion()
            assert b.status().tolist() == [0, 0, 0]
            b.register(refs, movs2)
            assert b.status().tolist() == [0, 0, 0]
            out[conv_lds] = (one, b.motion(), b.info()["placement"])
    assert out[1][2] == [1] and out[0][2] == [0]
    assert np.array_equal(out[1][0], out[0][0])
    assert np.array_equal(out[1][1], out[0][1])
    # the warm start is live: the second frame moved on from the first
    assert not np.array_equal(out[1][0], out[1][1])


def test_device_tensors_give_the_host_path_bits(gpu):
    import torch
    from opticalflow2d_amd import BatchRegistration
    dims, niter, p, B = (40, 33), [6], params(), 3
    refs, movs = make_pairs(dims, B)
    refs, movs = refs.astype(np.float32), movs.astype(np.float32)
    host = run_batch(dims, niter, 0, p, 1, refs.astype(np.float64), movs.astype(np.float64),
                     fixed_iters=1, conv_lds=1)

    def strided(a):
        # [B, dimy, dimx] in memory, seen as [B, dimx, dimy]: not contiguous
        t = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 1))).to("cuda")
        t = t.transpose(1, 2)
        assert not t.is_contiguous()
        return t

    with BatchRegistration(B, dims, niter, 0, p, reg=REG, device=0, fixed_iters=1,
                           conv_lds=1) as b:
        b.register(strided(refs), strided(movs))
        motion = b.motion_device().cpu().numpy()
        warped = b.warp(strided(movs)).cpu().numpy()
        assert b.status().tolist() == [0] * B and b.info()["placement"] == [1]
    assert motion.dtype == np.float32 and warped.dtype == np.float32
    assert host["motion"].any()
    assert np.array_equal(motion.astype(np.float64), host["motion"])
    assert np.array_equal(warped.astype(np.float64), host["warp"])
