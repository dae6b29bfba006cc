"""Batched Diffeomorphic Demons on the device (BatchRegistration reg=3 with
diffeomorphic=1) against the oracle's reg=4 run and the
one-pair reg=4 path: every pair of a batch bit for bit, squaring counts that
are live and differ between the pairs of a batch, pairs independent of each
other, per-pair convergence and divide-by-zero, a launch count independent of
the batch size, more pairs than block slots, device tensors and non-finite
input."""
import numpy as np
import pytest

from opticalflow2d_amd import synthetic as S

pytestmark = pytest.mark.gpu

REG = 3       # the batch's method; the option makes it the one-pair method 4
ONE_PAIR = 4  # DemonsDiffeomorphic

# [sigma_i, sigma_x, sigma_diffusion, sigma_fluid, kernel_width]
# sigma_x < sigma_i / 2: |c| <= sigma_x / (2 sigma_i) = 0.125, maxabs <= 0.18,
# so nsq = max(0, ceil(1 + log2(maxabs))) = 0 in every iteration
QUIET = [1.0, 0.25, 1.5, 2.5, 5]
# sigma_x > sigma_i: |c| up to 1, maxabs up to sqrt(2): 0, 1 or 2 squarings
LIVE = [1.0, 2.0, 1.0, 1.0, 5]


def with_kw(p, kw):
    return p[:4] + [kw]


def batch_params(p):
    """The batch's six parameters: the one-pair five and Composition."""
    return list(p) + [0]


def make_pairs(dims, B, shared=False, seed0=10):
    """B different textured pairs with different shifts; shared: one reference."""
    dimx, dimy = dims
    refs, movs = [], []
    for k in range(B):
        shift = (0.4 + 0.35 * k, -0.3 - 0.2 * k if k % 2 else 0.25 + 0.15 * k)
        r, m = S.texture_pair(dimx, seed=seed0 if shared else seed0 + k, sigma=2.0, shift=shift,
                              ny=dimy)
        refs.append(r)
        movs.append(m)
    return (refs[0] if shared else np.stack(refs)), np.stack(movs)


def ref_of(refs, k):
    return refs if refs.ndim == 2 else refs[k]


def oracle_pair(O, dims, niter, nscales, p, nrefine, ref, mov, fixed=True):
    o = O.Registration(dims, niter, nscales, ONE_PAIR, p, nrefine, fixed_iters=fixed)
    o.register(ref, mov)
    out = o.motion(), o.warp(mov), o.iterations(), o.last_errors()
    o.close()
    return out


def run_batch(dims, niter, nscales, p, nrefine, refs, movs, **opt):
    from opticalflow2d_amd import BatchRegistration
    opt.setdefault("diffeomorphic", 1)
    with BatchRegistration(len(movs), dims, niter, nscales, batch_params(p), nrefine, reg=REG,
                           device=0, **opt) as b:
        b.register(refs, movs)
        return {"motion": b.motion(), "warp": b.warp(movs), "iters": b.iterations(),
                "status": b.status(), "info": b.info(), "error": b.last_error(),
                "errs": [b.last_errors(k) for k in range(len(movs))]}


def launches_formula(nscales, nrefine):
    """warp, loop and accumulate per loop; a motion downsample
    per level strictly between the coarsest and level 0, an upsample per level
    above 0; the pass that zeroes failed pairs.  The option adds none."""
    return 3 * (nscales + 1) * nrefine + max(nscales - 1, 0) + nscales + 1


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def squarings(maxabs):
    """Motion::exp's count (Motion.cpp:253-261) from Motion::maxabs's value."""
    with np.errstate(divide="ignore"):
        c = np.ceil(np.float32(1.0) + np.log2(np.float32(maxabs)))
    return max(int(c), 0) if np.isfinite(c) else 0


def restate_on_cpu(O, dims, niter, nscales, p, ref, mov, fixed):
    """The pyramid (nrefine 1) of DemonsDiffeomorphic::get_update from the
    oracle's primitives with the reference's Logger (Motion::norm's sequential
    float sums): per loop the iteration count, every error and every
    iteration's squaring count, and the motion."""
    L = O.lib()
    dimx, dimy = dims
    kw = int(p[4])
    kdiff, kfluid = np.zeros(kw * kw), np.zeros(kw * kw)
    L.oracle_gaussian_kernel(kw, p[2], kdiff)
    L.oracle_gaussian_kernel(kw, p[3], kfluid)
    ldim = []
    for s in range(nscales + 1):
        scale = np.float32(2.0 ** s)
        ldim.append((int(np.float32(dimx) / scale), int(np.float32(dimy) / scale)))
    Iref = [f32(np.asarray(ref).T)]
    Imov = [f32(np.asarray(mov).T)]
    for s in range(1, nscales + 1):
        for stack in (Iref, Imov):
            out = np.zeros((ldim[s][1], ldim[s][0]), np.float32)
            L.oracle_downsample_image(stack[0], dimx, dimy, out, ldim[s][0], ldim[s][1])
            stack.append(out)
    motion = [np.zeros((dy, dx, 2), np.float32) for dx, dy in ldim]
    counts, errors, nsq = [], [], []
    for s in range(nscales, -1, -1):
        dx, dy = ldim[s]
        n = dx * dy
        if 0 < s < nscales:
            L.oracle_downsample_motion(motion[0].reshape(-1), dimx, dimy, motion[s].reshape(-1),
                                       dx, dy)
        Iaux = Imov[s].copy()
        L.oracle_warp2d(Iaux, motion[s].reshape(-1), dx, dy)
        u = np.zeros((dy, dx, 2), np.float32)
        prev = u.copy()
        dI = np.zeros((dy, dx, 2), np.float32)
        It = np.zeros((dy, dx), np.float32)
        c = np.zeros((dy, dx, 2), np.float32)
        errs, sq = [], []
        for it in range(niter[s]):
            W = Iaux.copy()
            L.oracle_warp2d(W, u.reshape(-1), dx, dy)
            L.oracle_spatial_derivative(W, dx, dy, dI.reshape(-1))
            L.oracle_temporal_derivative(Iref[s], W, n, It)
            assert L.oracle_demons_force(dI.reshape(-1), It, n, p[0], p[1], c.reshape(-1)) == 0
            L.oracle_convolute_motion(c.reshape(-1), dx, dy, kfluid, kw)
            # DemonsDiffeomorphic.cpp: correspondence->exp()
            sq.append(squarings(L.oracle_motion_maxabs(c.reshape(-1), n)))
            L.oracle_motion_exp(c.reshape(-1), dx, dy)
            L.oracle_accumulate(u.reshape(-1), c.reshape(-1), dx, dy)
            L.oracle_convolute_motion(u.reshape(-1), dx, dy, kdiff, kw)
            # Logger::update_error (Logger.cpp:32-51)
            pn = np.float32(L.oracle_motion_norm(prev.reshape(-1), n))
            dn = np.float32(L.oracle_motion_norm(f32(u - prev).reshape(-1), n))
            errs.append(np.float32(0.0) if pn == 0 else np.float32(dn / pn))
            prev = u.copy()
            if not fixed and errs[-1] < np.float32(0.001) and it > 1:
                break
        counts.append(len(errs))
        errors.append(np.array(errs, np.float32))
        nsq.append(sq)
        L.oracle_accumulate(motion[s].reshape(-1), u.reshape(-1), dx, dy)
        if s > 0:
            L.oracle_upsample_motion(motion[s].reshape(-1), dx, dy, motion[0].reshape(-1), dimx,
                                     dimy)
    return counts, errors, motion[0].astype(np.float64).transpose(1, 0, 2), nsq


# the (67, 50) pyramid with two refines: shared by the bit-for-bit, independence
# and launch-count tests
PYR = dict(dims=(67, 50), niter=[5, 6, 7], nscales=2, nrefine=2)
_cache = {}


def pyramid_case(B=7):
    if B not in _cache:
        refs, movs = make_pairs(PYR["dims"], 7)
        _cache.setdefault("in", (refs, movs))
        _cache[B] = run_batch(PYR["dims"], PYR["niter"], PYR["nscales"], LIVE, PYR["nrefine"],
                              refs[:B], movs[:B], fixed_iters=1)
    return _cache["in"], _cache[B]


FIXED_CASES = [
    # dims, B, niter, nscales, shared reference, parameters
    ((40, 33), 1, [7], 0, False, LIVE),  # a width that is no multiple of the wave
    ((40, 33), 3, [7], 0, False, LIVE),
    ((40, 33), 3, [7], 0, False, QUIET),  # no squaring in any iteration
    # dimx >= 128: the one-pair path takes its fused mode-3 kernel at level 0
    # and the unfused pair at level 1 (65, 8)
    ((130, 17), 5, [6, 9], 1, True, LIVE),
    # a kernel wider than the grid: level 1 is (4, 150), its taps wrap twice
    ((9, 300), 2, [5, 6], 1, False, with_kw(LIVE, 15)),
    ((9, 300), 2, [5, 6], 1, False, with_kw(LIVE, 1)),
    # an even width sums a 3 x 3 corner of the 4 x 4 table: the weight sum is
    # not 1 and the interior division is live
    ((9, 300), 2, [5, 6], 1, False, with_kw(LIVE, 4)),
]


def check_against_oracle_and_one_pair(oracle, dims, niter, nscales, nrefine, p, refs, movs, got):
    from opticalflow2d_amd import ImageRegistration
    B = len(movs)
    want_iters = [n for n in reversed(niter[: nscales + 1]) for _ in range(nrefine)]
    assert got["status"].tolist() == [0] * B and got["error"] == ""
    assert got["info"]["threads"] == [1024] * (nscales + 1)
    assert got["info"]["placement"] == [0] * (nscales + 1)
    assert got["iters"].tolist() == [want_iters] * B
    for k in range(B):
        m, w, it, _ = oracle_pair(oracle, dims, niter, nscales, p, nrefine, ref_of(refs, k),
                                  movs[k])
        assert it == want_iters and m.any()
        assert np.array_equal(got["motion"][k], m), f"pair {k}: motion differs from the oracle"
        assert np.array_equal(got["warp"][k], w), f"pair {k}: warp differs from the oracle"
        with ImageRegistration(dims, niter, nscales, ONE_PAIR, p, nrefine, fixed_iters=1,
                               device=0) as r:
            r.register(ref_of(refs, k), movs[k])
            assert r.iterations() == want_iters
            assert np.array_equal(got["motion"][k], r.motion()), f"pair {k}: one-pair path"
            assert np.array_equal(got["warp"][k], r.warp(movs[k]))
        assert got["errs"][k].size == 0  # fixed_iters: no errors recorded


@pytest.mark.parametrize("dims, B, niter, nscales, shared, p", FIXED_CASES)
def test_fixed_iterations_bit_for_bit(gpu, oracle, dims, B, niter, nscales, shared, p):
    refs, movs = make_pairs(dims, B, shared)
    if p is QUIET:  # the bound argument, on this input
        for k in range(B):
            sq = restate_on_cpu(oracle, dims, niter, nscales, p, ref_of(refs, k), movs[k], True)[3]
            assert not np.any(np.concatenate(sq))
    got = run_batch(dims, niter, nscales, p, 1, refs, movs, fixed_iters=1)
    check_against_oracle_and_one_pair(oracle, dims, niter, nscales, 1, p, refs, movs, got)


def test_fixed_iterations_pyramid_two_refines(gpu, oracle):
    (refs, movs), got = pyramid_case(7)
    check_against_oracle_and_one_pair(oracle, PYR["dims"], PYR["niter"], PYR["nscales"],
                                      PYR["nrefine"], LIVE, refs, movs, got)


# ------------------------------------------------------------ live squarings
LIVE_CASE = dict(dims=(40, 33), niter=[8], B=5)


def test_squarings_are_live_and_differ_between_pairs(gpu, oracle):
    """A condition on the inputs, established on the CPU before the device
    runs: the iteration restated from the oracle's primitives is the oracle's
    whole run bit for bit, so its squaring counts are the run's; the batch
    holds iterations with 0, 1 and 2 squarings, and in at least one iteration
    two pairs take different counts (the kernel's count is the pair's own, not
    the batch's).  Then the batch equals the oracle per pair."""
    dims, niter, B = LIVE_CASE["dims"], LIVE_CASE["niter"], LIVE_CASE["B"]
    refs, movs = make_pairs(dims, B)
    seqs, want = [], []
    for k in range(B):
        m, w, it, _ = oracle_pair(oracle, dims, niter, 0, LIVE, 1, refs[k], movs[k])
        rc, _, rmotion, sq = restate_on_cpu(oracle, dims, niter, 0, LIVE, refs[k], movs[k], True)
        assert rc == it == niter
        assert np.array_equal(rmotion, m), f"pair {k}: the restatement is not the oracle's run"
        seqs.append(sq[0])
        want.append((m, w))
    seqs = np.array(seqs)  # [pair, iteration]
    assert {0, 1, 2} <= set(seqs.reshape(-1).tolist()), seqs
    assert any(len(set(col.tolist())) > 1 for col in seqs.T), seqs
    got = run_batch(dims, niter, 0, LIVE, 1, refs, movs, fixed_iters=1)
    assert got["status"].tolist() == [0] * B
    for k, (m, w) in enumerate(want):
        assert np.array_equal(got["motion"][k], m), f"pair {k}: squarings {seqs[k].tolist()}"
        assert np.array_equal(got["warp"][k], w), f"pair {k}"


# ------------------------------------------------------------ independence
def test_pairs_do_not_see_each_other(gpu):
    (refs, movs), all7 = pyramid_case(7)
    for k in (0, 3, 6):
        one = run_batch(PYR["dims"], PYR["niter"], PYR["nscales"], LIVE, PYR["nrefine"],
                        refs[k:k + 1], movs[k:k + 1], fixed_iters=1)
        assert np.array_equal(one["motion"][0], all7["motion"][k])
        assert np.array_equal(one["warp"][0], all7["warp"][k])
    # the same object registered twice, then with the option off and on again
    from opticalflow2d_amd import BatchRegistration
    thirion = run_batch(PYR["dims"], PYR["niter"], PYR["nscales"], LIVE, PYR["nrefine"], refs,
                        movs, fixed_iters=1, diffeomorphic=0)
    with BatchRegistration(7, PYR["dims"], PYR["niter"], PYR["nscales"], batch_params(LIVE),
                           PYR["nrefine"], reg=REG, device=0, fixed_iters=1) as b:
        b.register(refs, movs)
        plain = b.motion()  # the default is the existing path
        b.set_option("diffeomorphic", 1)
        b.register(refs, movs)
        first = b.motion()
        b.register(refs, movs)
        second = b.motion()
        b.set_option("diffeomorphic", 0)
        b.register(refs, movs)
        middle = b.motion()
        b.set_option("diffeomorphic", 1)
        b.register(refs, movs)
        third = b.motion()
    assert np.array_equal(first, all7["motion"]) and np.array_equal(second, all7["motion"])
    assert np.array_equal(third, all7["motion"])
    assert np.array_equal(plain, thirion["motion"]) and np.array_equal(middle, thirion["motion"])
    assert not np.array_equal(thirion["motion"], all7["motion"])  # the squarings matter here


# ------------------------------------------------------------ convergence
# Chosen on the CPU: with LIVE's sigma_x = 2 most of these loops oscillate past
# 200 iterations whatever sigma_diffusion is; sigma_x = 1.5 (|c| up to 0.75,
# one squaring at most) with sigma_diffusion 2.5 converges on these inputs
# while the second pair still takes squarings inside its loops
CONV_P = [1.0, 1.5, 2.5, 1.0, 5]
CONV_INPUTS = [(40, (0.3, 0.2)), (43, (1.4, 0.8)), (45, (0.5, 0.6)), (46, (0.3, 0.2))]
# the oracle's convergence-on counts, run on the CPU (coarsest level first)
CONV_CASES = [
    ((48, 40), [200], 0, [[30], [41], [26], [27]]),
    ((67, 50), [200, 200, 200], 2, [[18, 19, 25], [13, 16, 27], [14, 20, 32], [24, 25, 33]]),
]


def conv_pairs(dims):
    dimx, dimy = dims
    out = [S.texture_pair(dimx, seed=seed, sigma=2.5, shift=sh, ny=dimy)
           for seed, sh in CONV_INPUTS]
    return np.stack([r for r, _ in out]), np.stack([m for _, m in out])


@pytest.mark.parametrize("dims, niter, nscales, recorded", CONV_CASES)
def test_convergence_per_pair(gpu, oracle, dims, niter, nscales, recorded):
    """Each pair stops on its own iteration: the oracle's (the reference's
    sequential float Logger), because no oracle error of any loop lies within
    1e-3 relative of the threshold (asserted on the CPU first; the nearest is
    0.50 % away at (48, 40) and 1.2 % in the pyramid) and the fp64 and float
    sums of at most 3350 terms differ by far less.  At least one pair
    takes a squaring inside its loop.  The motion is the oracle's fixed_iters
    run with the pair's counts, bit for bit, and counts, motion and errors are
    the one-pair logger_fp64 reg=4 path's (errors within one float32 ulp: its
    fp64 sums are a tree over blocks, the batch's run in the batch's fixed
    order)."""
    from opticalflow2d_amd import ImageRegistration
    p = CONV_P
    refs, movs = conv_pairs(dims)
    B = len(movs)
    assert B >= 3
    want, live = [], False
    for k in range(B):
        m, w, counts, last = oracle_pair(oracle, dims, niter, nscales, p, 1, refs[k], movs[k],
                                         fixed=False)
        rc, rerrs, rmotion, sq = restate_on_cpu(oracle, dims, niter, nscales, p, refs[k], movs[k],
                                                False)
        # the restatement is the oracle's loop: its errors are the oracle's
        assert rc == counts and np.array_equal(rerrs[-1], last)
        assert np.array_equal(rmotion, m)
        assert counts == recorded[k]
        for s, (c, e) in enumerate(zip(counts, rerrs)):
            assert 2 < c < niter[nscales - s]
            assert np.all(np.abs(e.astype(np.float64) - 0.001) > 1e-3 * 0.001)
        live |= any(np.any(q) for q in sq)
        want.append(counts)
    assert len({tuple(c) for c in want}) == B, want
    assert live, "no pair takes a squaring inside its loop"
    got = run_batch(dims, niter, nscales, p, 1, refs, movs)
    assert got["status"].tolist() == [0] * B
    assert got["info"]["threads"] == [1024] * (nscales + 1)
    for k in range(B):
        assert got["iters"][k].tolist() == want[k], f"pair {k}: break not on the oracle's iteration"
        # the oracle's fixed run with the pair's counts (niter is finest level first)
        m, w, _, _ = oracle_pair(oracle, dims, want[k][::-1], nscales, p, 1, refs[k], movs[k])
        assert np.array_equal(got["motion"][k], m), f"pair {k}"
        assert np.array_equal(got["warp"][k], w), f"pair {k}"
        with ImageRegistration(dims, niter, nscales, ONE_PAIR, p, 1, logger_fp64=1,
                               device=0) as r:
            r.register(refs[k], movs[k])
            assert r.iterations() == want[k], f"pair {k}: one-pair logger_fp64 counts"
            assert np.array_equal(got["motion"][k], r.motion()), f"pair {k}: one-pair path"
            one = r.last_errors()
        e = got["errs"][k]
        assert e.shape == one.shape == (want[k][-1],)
        assert np.all(np.abs(e.astype(np.float64) - one.astype(np.float64))
                      <= np.spacing(one).astype(np.float64)), f"pair {k}"


# ------------------------------------------------------------ divide by zero
def test_divide_by_zero_is_per_pair(gpu, oracle):
    from opticalflow2d_amd import _lib
    dims, niter, p = (40, 33), [5], LIVE
    refs, movs = make_pairs(dims, 4)
    bad = 2
    refs[bad] = 0.5
    movs[bad] = 0.5
    with pytest.raises(oracle.OracleError, match="Divide by zero exception"):
        oracle_pair(oracle, dims, niter, 0, p, 1, refs[bad], movs[bad])
    got = run_batch(dims, niter, 0, p, 1, refs, movs, fixed_iters=1)
    want = [_lib.OF2D_OK] * 4
    want[bad] = _lib.OF2D_ERR_RUNTIME
    assert got["status"].tolist() == want
    assert "Divide by zero exception" in got["error"] and f"pair {bad}" in got["error"]
    assert not got["motion"][bad].any()
    keep = [k for k in range(4) if k != bad]
    clean = run_batch(dims, niter, 0, p, 1, refs[keep], movs[keep], fixed_iters=1)
    assert clean["status"].tolist() == [0, 0, 0] and clean["error"] == ""
    for n, k in enumerate(keep):
        assert clean["motion"][n].any()
        assert np.array_equal(got["motion"][k], clean["motion"][n]), f"pair {k}"
        assert np.array_equal(got["warp"][k], clean["warp"][n]), f"pair {k}"


# ------------------------------------------------------------ launches, many pairs
def test_launch_count_does_not_depend_on_batch_size(gpu):
    _, one = pyramid_case(1)
    _, all7 = pyramid_case(7)
    want = launches_formula(PYR["nscales"], PYR["nrefine"])
    assert one["info"]["launches"] == all7["info"]["launches"] == want == 22
    assert one["info"]["loops"] == all7["info"]["loops"] == 6
    assert all7["info"]["placement"] == [0, 0, 0]
    assert all7["info"]["threads"] == [1024, 1024, 1024]


MANY_SHIFTS = [(0.5, 0.25), (-0.75, 0.5), (1.25, -0.9), (0.1, 0.9), (0.6, -0.4), (-0.3, 0.8),
               (0.9, 1.1), (-1.1, -0.2)]


def many_eight():
    return [S.texture_pair(16, seed=7 + k // 4, sigma=1.5, shift=sh, ny=12)
            for k, sh in enumerate(MANY_SHIFTS)]


def test_more_pairs_than_block_slots(gpu, oracle):
    """600 workgroups of 1024 threads: a CU holds 32 waves, two such
    workgroups, so the 256 CUs hold 512 at a time and the grid takes a second
    round of blocks.  (16, 12) has fewer pixels than threads: most threads
    bring 0 to the block maximum.  The eight pairs take squarings (asserted on
    the CPU)."""
    dims, niter, B, p = (16, 12), [3], 600, LIVE
    eight = many_eight()
    # on the CPU first: the oracle takes every one of the eight
    want = [oracle_pair(oracle, dims, niter, 0, p, 1, r, m) for r, m in eight]
    sq = [restate_on_cpu(oracle, dims, niter, 0, p, r, m, True)[3][0] for r, m in eight]
    assert np.any(sq) and len({tuple(q) for q in sq}) > 1, sq
    which = (np.arange(B) * 5 + np.arange(B) // 256) % 8
    assert which[0] == 0 and len(set(which.tolist())) == 8
    refs = np.stack([eight[w][0] for w in which])
    movs = np.stack([eight[w][1] for w in which])
    got = run_batch(dims, niter, 0, p, 1, refs, movs, fixed_iters=1)
    assert not got["status"].any()
    assert got["info"]["threads"] == [1024]
    for w in range(8):
        sel = np.flatnonzero(which == w)
        assert sel.size > 50
        first = sel[0]
        assert np.array_equal(got["motion"][sel], np.broadcast_to(got["motion"][first],
                                                                  (sel.size,) + dims + (2,)))
        assert np.array_equal(got["warp"][sel], np.broadcast_to(got["warp"][first],
                                                                (sel.size,) + dims))
    for k in (0, B - 1):
        m, wimg, _, _ = want[which[k]]
        assert m.any()
        assert np.array_equal(got["motion"][k], m) and np.array_equal(got["warp"][k], wimg)


# ------------------------------------------------------------ device tensors
def test_device_tensors_give_the_host_path_bits(gpu):
    import torch
    from opticalflow2d_amd import BatchRegistration
    dims, niter, p, B = (40, 33), [6], LIVE, 3
    refs, movs = make_pairs(dims, B)
    refs, movs = refs.astype(np.float32), movs.astype(np.float32)
    host = run_batch(dims, niter, 0, p, 1, refs.astype(np.float64), movs.astype(np.float64),
                     fixed_iters=1)

    def strided(a):
        # [B, dimy, dimx] in memory, seen as [B, dimx, dimy]: not contiguous
        t = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 1))).to("cuda")
        t = t.transpose(1, 2)
        assert not t.is_contiguous()
        return t

    with BatchRegistration(B, dims, niter, 0, batch_params(p), reg=REG, device=0, fixed_iters=1,
                           diffeomorphic=1) as b:
        b.register(strided(refs), strided(movs))
        motion = b.motion_device().cpu().numpy()
        warped = b.warp(strided(movs)).cpu().numpy()
        assert b.status().tolist() == [0] * B
    assert motion.dtype == np.float32 and warped.dtype == np.float32
    assert host["motion"].any()
    assert np.array_equal(motion.astype(np.float64), host["motion"])
    assert np.array_equal(warped.astype(np.float64), host["warp"])


# ------------------------------------------------------------ non-finite input
def same_bits_and_nans(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na],
                                                     b.view(np.uint64)[~nb])


def test_nan_pixel_as_the_one_pair_path(gpu):
    """Pins the NaN arithmetic of the exp stages as the Thirion test pins the
    loop's: the maximum drops a NaN term, a squaring keeps a pixel whose
    sampling coordinate is NaN."""
    from opticalflow2d_amd import ImageRegistration
    dims, niter, p = (40, 33), [4], LIVE
    refs, movs = make_pairs(dims, 3)
    clean = run_batch(dims, niter, 0, p, 1, refs, movs, fixed_iters=1)
    bad = 1
    movs_nan = movs.copy()
    movs_nan[bad, 17, 12] = np.nan
    got = run_batch(dims, niter, 0, p, 1, refs, movs_nan, fixed_iters=1)
    assert got["status"].tolist() == [0, 0, 0]
    with ImageRegistration(dims, niter, 0, ONE_PAIR, p, 1, fixed_iters=1, device=0) as r:
        r.register(refs[bad], movs_nan[bad])
        one_m, one_w = r.motion(), r.warp(movs_nan[bad])
    assert np.isnan(one_w).any() and not np.isnan(one_w).all()
    assert not same_bits_and_nans(one_m, clean["motion"][bad])
    assert same_bits_and_nans(got["motion"][bad], one_m)
    assert same_bits_and_nans(got["warp"][bad], one_w)
    for k in (0, 2):
        assert np.array_equal(got["motion"][k], clean["motion"][k])
        assert np.array_equal(got["warp"][k], clean["warp"][k])
