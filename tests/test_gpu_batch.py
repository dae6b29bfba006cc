"""Batched Horn-Schunck on the device (BatchRegistration)
against the oracle and the one-pair path: every pair of a batch bit for bit,
pairs independent of each other, per-pair convergence and divide-by-zero, a
launch count independent of the batch size, and more pairs than block slots."""
import math

import numpy as np
import pytest

from opticalflow2d_amd import synthetic as S

pytestmark = pytest.mark.gpu

ALPHA = 0.1


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


def oracle_pair(O, dims, niter, nscales, alpha, nrefine, ref, mov):
    o = O.Registration(dims, niter, nscales, 0, [alpha], nrefine, fixed_iters=True)
    o.register(ref, mov)
    out = o.motion(), o.warp(mov), o.iterations()
    o.close()
    return out


def run_batch(dims, niter, nscales, alpha, nrefine, refs, movs, **opt):
    from opticalflow2d_amd import BatchRegistration
    with BatchRegistration(len(movs), dims, niter, nscales, alpha, nrefine, device=0, **opt) as b:
        b.register(refs, movs)
        return {"motion": b.motion(), "warp": b.warp(movs), "iters": b.iterations(),
                "status": b.status(), "info": b.info(), "error": b.last_error(),
                "errs": [b.last_errors(k) for k in range(len(movs))]}


# the (67, 50) pyramid with two refines: shared by the bit-for-bit, independence
# and launch-count tests
PYR = dict(dims=(67, 50), niter=[5, 6, 7], nscales=2, nrefine=2)
_cache = {}


def pyramid_case(B=7):
    if B not in _cache:
        refs, movs = make_pairs(PYR["dims"], 7)
        _cache.setdefault("in", (refs, movs))
        _cache[B] = run_batch(PYR["dims"], PYR["niter"], PYR["nscales"], ALPHA, PYR["nrefine"],
                              refs[:B], movs[:B], fixed_iters=1)
    return _cache["in"], _cache[B]


FIXED_CASES = [
    # dims, B, niter, nscales, nrefine, shared reference
    # a pair's workgroup has 1024 threads at every level (asserted below)
    ((40, 33), 1, [7], 0, 1, False),   # a width that is no multiple of the wave
    ((40, 33), 3, [7], 0, 1, False),
    # wider than the pitch unit; level 1 is (65, 8): fewer pixels than threads
    ((130, 17), 5, [6, 9], 1, 1, True),
    # one round of the threads covers 113 rows of 9 pixels: 300 rows take three
    ((9, 300), 2, [5, 6], 1, 1, False),
]


def check_against_oracle_and_one_pair(oracle, dims, niter, nscales, nrefine, refs, movs, got):
    from opticalflow2d_amd import ImageRegistration
    B = len(movs)
    loops = (nscales + 1) * nrefine
    want_iters = [n for n in reversed(niter[: nscales + 1]) for _ in range(nrefine)]
    assert got["status"].tolist() == [0] * B and got["error"] == ""
    assert got["info"]["threads"] == [1024] * (nscales + 1)
    assert got["iters"].tolist() == [want_iters] * B and len(want_iters) == loops
    for k in range(B):
        m, w, it = oracle_pair(oracle, dims, niter, nscales, ALPHA, nrefine, ref_of(refs, k),
                               movs[k])
        assert it == want_iters
        assert np.array_equal(got["motion"][k], m), f"pair {k}: motion differs from the oracle"
        assert np.array_equal(got["warp"][k], w), f"pair {k}: warp differs from the oracle"
        with ImageRegistration(dims, niter, nscales, 0, [ALPHA], nrefine, fixed_iters=1,
                               device=0) as r:
            r.register(ref_of(refs, k), movs[k])
            assert np.array_equal(got["motion"][k], r.motion()), f"pair {k}: one-pair path"
            assert np.array_equal(got["warp"][k], r.warp(movs[k]))
        assert got["errs"][k].size == 0  # fixed_iters: no errors recorded


@pytest.mark.parametrize("dims, B, niter, nscales, nrefine, shared", FIXED_CASES)
def test_fixed_iterations_bit_for_bit(gpu, oracle, dims, B, niter, nscales, nrefine, shared):
    refs, movs = make_pairs(dims, B, shared)
    got = run_batch(dims, niter, nscales, ALPHA, nrefine, refs, movs, fixed_iters=1)
    check_against_oracle_and_one_pair(oracle, dims, niter, nscales, nrefine, refs, movs, got)


def test_fixed_iterations_pyramid_two_refines(gpu, oracle):
    (refs, movs), got = pyramid_case(7)
    check_against_oracle_and_one_pair(oracle, PYR["dims"], PYR["niter"], PYR["nscales"],
                                      PYR["nrefine"], refs, movs, got)


def test_pairs_do_not_see_each_other(gpu):
    (refs, movs), all7 = pyramid_case(7)
    for k in (0, 3, 6):
        one = run_batch(PYR["dims"], PYR["niter"], PYR["nscales"], ALPHA, PYR["nrefine"],
                        refs[k:k + 1], movs[k:k + 1], fixed_iters=1)
        assert np.array_equal(one["motion"][0], all7["motion"][k])
        assert np.array_equal(one["warp"][0], all7["warp"][k])
    # two identical calls: a new object, and the same object registered twice
    from opticalflow2d_amd import BatchRegistration
    with BatchRegistration(7, PYR["dims"], PYR["niter"], PYR["nscales"], ALPHA, PYR["nrefine"],
                           device=0, fixed_iters=1) as b:
        b.register(refs, movs)
        first = b.motion()
        b.register(refs, movs)
        second = b.motion()
    assert np.array_equal(first, all7["motion"]) and np.array_equal(second, all7["motion"])


# ------------------------------------------------------------ convergence
def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def logger_error_restated(u_new, u_old):
    """Motion::norm's terms summed exactly (math.fsum), then logger_error's
    float arithmetic."""
    d = (u_new - u_old).astype(np.float32).astype(np.float64).reshape(-1, 2)
    p = u_old.astype(np.float64).reshape(-1, 2)
    sd = math.fsum(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).tolist())
    sp = math.fsum(np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]).tolist())
    n = np.float32(d.shape[0])
    prevnorm = np.float32(sp) / n
    diffnorm = np.float32(sd) / n
    return np.float32(0.0) if prevnorm == 0 else np.float32(diffnorm / prevnorm)


def restate_on_cpu(O, dims, niter, nscales, alpha, ref, mov):
    """The pyramid (nrefine 1) from the oracle's primitives with exactly summed
    Logger errors: per loop the iteration count and the errors, and the motion."""
    L = O.lib()
    dimx, dimy = dims
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
    counts, errors = [], []
    for s in range(nscales, -1, -1):
        dx, dy = ldim[s]
        if 0 < s < nscales:
            L.oracle_downsample_motion(motion[0].reshape(-1), dimx, dimy, motion[s].reshape(-1),
                                       dx, dy)
        Iaux = Imov[s].copy()
        L.oracle_warp2d(Iaux, motion[s].reshape(-1), dx, dy)
        dI = np.zeros((dy, dx, 2), np.float32)
        It = np.zeros((dy, dx), np.float32)
        L.oracle_spatial_derivative(Iaux, dx, dy, dI.reshape(-1))
        L.oracle_temporal_derivative(Iref[s], Iaux, dx * dy, It)
        u = np.zeros((dy, dx, 2), np.float32)
        errs = []
        for it in range(niter[s]):
            prev = u.copy()
            assert L.oracle_hs_update(u.reshape(-1), dI.reshape(-1), It, dx, dy, alpha) == 0
            errs.append(logger_error_restated(u, prev))
            if errs[-1] < np.float32(0.001) and it > 1:
                break
        counts.append(len(errs))
        errors.append(np.array(errs, np.float32))
        L.oracle_accumulate(motion[s].reshape(-1), u.reshape(-1), dx, dy)
        if s > 0:
            L.oracle_upsample_motion(motion[s].reshape(-1), dx, dy, motion[0].reshape(-1), dimx,
                                     dimy)
    return counts, errors, motion[0]


# alpha 0.3: every loop of these sizes breaks below the 200-iteration cap
CONV_ALPHA = 0.3
CONV_SHIFTS = [(0.3, 0.2), (1.1, -0.6), (2.0, 1.3), (0.7, 0.9)]


def conv_pairs(dims):
    dimx, dimy = dims
    out = [S.texture_pair(dimx, seed=40 + k, sigma=2.5, shift=sh, ny=dimy)
           for k, sh in enumerate(CONV_SHIFTS)]
    return np.stack([r for r, _ in out]), np.stack([m for _, m in out])


@pytest.mark.parametrize("dims, niter, nscales", [((48, 40), [200], 0),
                                                  ((67, 50), [200, 200, 200], 2)])
def test_convergence_per_pair(gpu, oracle, dims, niter, nscales):
    """Each pair stops on its own iteration; its motion is the oracle's
    fixed_iters run with the pair's reported counts, bit for bit; the errors
    are the exactly summed ones within one float32 ulp and the break falls on
    the restated iteration.

    The oracle's own convergence-on run (the reference's sequential float sum)
    is not asserted against.  Recorded on the CPU for these inputs: it breaks on
    the same iterations, (48, 40): 160, 182, 173, 175 for the four pairs;
    (67, 50): [52, 79, 149], [56, 69, 145], [58, 107, 186], [50, 89, 153]
    (coarsest level first); the exactly summed error nearest to the threshold
    is 1.3e-4 relative away from it."""
    refs, movs = conv_pairs(dims)
    B = len(movs)
    # on the CPU first: the inputs break at different iterations, below the cap,
    # and no exactly summed error is within 1e-5 relative of the threshold
    restated = [restate_on_cpu(oracle, dims, niter, nscales, CONV_ALPHA, refs[k], movs[k])
                for k in range(B)]
    last_counts = [r[0][-1] for r in restated]
    assert len(set(last_counts)) == B, last_counts
    for counts, errors, _ in restated:
        for s, (c, e) in enumerate(zip(counts, errors)):
            assert 2 < c < niter[nscales - s]
            assert np.all(np.abs(e.astype(np.float64) - 0.001) > 1e-5 * 0.001)
    got = run_batch(dims, niter, nscales, CONV_ALPHA, 1, refs, movs)
    assert got["status"].tolist() == [0] * B
    assert got["info"]["threads"] == [1024] * (nscales + 1)
    for k in range(B):
        counts, errors, motion = restated[k]
        assert got["iters"][k].tolist() == counts, f"pair {k}: break not on the restated iteration"
        # the oracle's fixed run with the pair's counts (niter is finest level first)
        m, w, _ = oracle_pair(oracle, dims, counts[::-1], nscales, CONV_ALPHA, 1, refs[k], movs[k])
        assert np.array_equal(got["motion"][k], m), f"pair {k}"
        assert np.array_equal(got["warp"][k], w), f"pair {k}"
        assert np.array_equal(motion.astype(np.float64).transpose(1, 0, 2), m)
        # the last loop's errors (level 0), against the exactly summed ones
        e = got["errs"][k]
        assert e.shape == errors[-1].shape
        if nscales == 0:
            assert np.all(np.abs(e.astype(np.float64) - errors[-1].astype(np.float64))
                          <= np.spacing(errors[-1]).astype(np.float64)), f"pair {k}"


# ------------------------------------------------------------ divide by zero
def test_divide_by_zero_is_per_pair(gpu, oracle):
    dims, niter = (40, 33), [5]
    refs, movs = make_pairs(dims, 4)
    bad = 2
    refs[bad] = 0.5
    movs[bad] = 0.5
    with pytest.raises(oracle.OracleError, match="Divide by zero exception"):
        oracle_pair(oracle, dims, niter, 0, 0.0, 1, refs[bad], movs[bad])
    got = run_batch(dims, niter, 0, 0.0, 1, refs, movs, fixed_iters=1)
    from opticalflow2d_amd import _lib
    want = [_lib.OF2D_OK] * 4
    want[bad] = _lib.OF2D_ERR_RUNTIME
    assert got["status"].tolist() == want
    assert "Divide by zero exception" in got["error"] and f"pair {bad}" in got["error"]
    assert not got["motion"][bad].any()
    for k in range(4):
        if k == bad:
            continue
        m, w, _ = oracle_pair(oracle, dims, niter, 0, 0.0, 1, refs[k], movs[k])
        assert np.array_equal(got["motion"][k], m), f"pair {k}"
        assert np.array_equal(got["warp"][k], w), f"pair {k}"


# ------------------------------------------------------------ launches, many pairs
def test_launch_count_does_not_depend_on_batch_size(gpu):
    _, one = pyramid_case(1)
    _, all7 = pyramid_case(7)
    assert one["info"]["launches"] == all7["info"]["launches"] > 0
    assert one["info"]["loops"] == all7["info"]["loops"] == 6
    assert all7["info"]["placement"] == [0, 0, 0]
    assert all7["info"]["threads"] == [1024, 1024, 1024]


def test_more_pairs_than_block_slots(gpu, oracle):
    """1100 workgroups of 1024 threads: a CU holds 32 waves, two such
    workgroups, so the 256 CUs hold 512 at a time and the grid takes a second
    and a third round of blocks.  (16, 12) has fewer pixels than threads."""
    dims, niter, B = (16, 12), [3], 1100
    # one seed: the same reference, shifted four ways
    both = [S.texture_pair(16, seed=7, sigma=1.5, shift=sh, ny=12)
            for sh in [(0.5, 0.25), (-0.75, 0.5), (1.25, -1.0), (0.1, 0.9)]]
    ref, four = both[0][0], [m for _, m in both]
    which = (np.arange(B) * 7 + np.arange(B) // 256) % 4
    movs = np.stack([four[w] for w in which])
    got = run_batch(dims, niter, 0, ALPHA, 1, ref, movs, fixed_iters=1)
    assert not got["status"].any()
    assert got["info"]["threads"] == [1024]
    for w in range(4):
        m, wimg, _ = oracle_pair(oracle, dims, niter, 0, ALPHA, 1, ref, four[w])
        sel = which == w
        assert sel.sum() > 200
        assert np.array_equal(got["motion"][sel], np.broadcast_to(m, (sel.sum(),) + m.shape))
        assert np.array_equal(got["warp"][sel], np.broadcast_to(wimg, (sel.sum(),) + wimg.shape))
