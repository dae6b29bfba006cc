"""The yardstick of the warm-start tests, on the CPU:
``estimate_from`` restates ImageRegistration::estimate_motion for Diffusion
from the oracle's primitives, starting from given per-level motions.  Before
anything is measured against it, it is held to ``oracle.Registration`` on the
bits: from zero, and from a reused start (the second and third ``register`` of
one oracle object, which never resets ``motion[]``)."""
import numpy as np
import pytest

from opticalflow2d_amd import synthetic as S


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def level_dims(dims, nscales):
    """ImageRegistration.cpp:56-61: dim(dimin.x / scale, dimin.y / scale), float scale."""
    out = []
    for s in range(nscales + 1):
        scale = np.float32(2.0 ** s)
        out.append((int(np.float32(dims[0]) / scale), int(np.float32(dims[1]) / scale)))
    return out


def zero_levels(dims, nscales):
    return [np.zeros((dy, dx, 2), np.float32) for dx, dy in level_dims(dims, nscales)]


def downsample_motion(O, m, dims_out):
    """Motion::downSample of a level-0 field ``[dimy, dimx, 2]``."""
    dy, dx = m.shape[:2]
    out = np.zeros((dims_out[1], dims_out[0], 2), np.float32)
    O.lib().oracle_downsample_motion(f32(m).reshape(-1), dx, dy, out.reshape(-1), dims_out[0],
                                     dims_out[1])
    return out


def field_of(m):
    """``[dimx, dimy, 2]`` float64 (the classes' motion) -> ``[dimy, dimx, 2]`` float32."""
    return f32(np.asarray(m).transpose(1, 0, 2))


def motion_of(field):
    """The reverse, as ``motion()`` returns it."""
    return np.ascontiguousarray(field.astype(np.float64).transpose(1, 0, 2))


def estimate_from(O, levels, Iref, Imov, niter, nscales, nrefine, alpha, fixed=True):
    """estimate_motion (ImageRegistration.cpp:133-156) with Diffusion, started
    from ``levels`` (per level from 0 a ``[dy, dx, 2]`` float32 motion).
    Returns (the levels afterwards, the iteration counts in execution order,
    the last loop's errors); ``levels`` is not modified."""
    L = O.lib()
    dimx, dimy = Iref.shape
    ldim = level_dims((dimx, dimy), nscales)
    motion = [f32(m).copy() for m in levels]
    assert [m.shape for m in motion] == [(dy, dx, 2) for dx, dy in ldim]
    ref = [f32(np.asarray(Iref, np.float64).T)]
    mov = [f32(np.asarray(Imov, np.float64).T)]
    for s in range(1, nscales + 1):
        for stack in (ref, mov):
            out = np.zeros((ldim[s][1], ldim[s][0]), np.float32)
            L.oracle_downsample_image(stack[0], dimx, dimy, out, ldim[s][0], ldim[s][1])
            stack.append(out)
    counts, errs = [], np.zeros(0, np.float32)
    for s in range(nscales, -1, -1):
        dx, dy = ldim[s]
        n = dx * dy
        if 0 < s < nscales:
            L.oracle_downsample_motion(motion[0].reshape(-1), dimx, dimy, motion[s].reshape(-1),
                                       dx, dy)
        for _ in range(nrefine):
            Iaux = mov[s].copy()
            L.oracle_warp2d(Iaux, motion[s].reshape(-1), dx, dy)
            dI = np.zeros((dy, dx, 2), np.float32)
            It = np.zeros((dy, dx), np.float32)
            L.oracle_spatial_derivative(Iaux, dx, dy, dI.reshape(-1))
            L.oracle_temporal_derivative(ref[s], Iaux, n, It)
            est = np.zeros((dy, dx, 2), np.float32)
            e = np.zeros(max(niter[s], 1), np.float32)
            it = L.oracle_hs_loop(est.reshape(-1), dI.reshape(-1), It, dx, dy, alpha, niter[s],
                                  int(fixed), e)
            assert it >= 0, "divide by zero in the restatement"
            counts.append(it)
            errs = e[:it].copy()
            L.oracle_accumulate(motion[s].reshape(-1), est.reshape(-1), dx, dy)
        if s > 0:
            L.oracle_upsample_motion(motion[s].reshape(-1), dx, dy, motion[0].reshape(-1), dimx,
                                     dimy)
    return motion, counts, errs


# three different pairs of one size: one reference each, a moving image per call
def warm_pairs(dims, ncalls=3, B=3, sigma=2.0, step=0.5):
    """``refs[k]``, ``movs[call][k]``: the same reference, the shift growing by
    ``step`` times the pair's direction per call (a slowly moving series),
    different textures per pair."""
    dimx, dimy = dims
    refs, movs = [], [[] for _ in range(ncalls)]
    for k in range(B):
        for c in range(ncalls):
            g, q = step * (c + 1), k % 5
            shift = (g * (0.5 + 0.3 * q), g * (-0.4 + 0.35 * q))
            r, m = S.texture_pair(dimx, seed=20 + k, sigma=sigma, shift=shift, ny=dimy)
            movs[c].append(m)
        refs.append(r)
    return np.stack(refs), [np.stack(m) for m in movs]


ALPHA = 0.1
CASES = [((40, 24), [6], 0, 1), ((40, 24), [4, 5, 6], 2, 2), ((19, 13), [4, 5, 6], 2, 2)]


@pytest.mark.parametrize("dims, niter, nscales, nrefine", CASES)
def test_restatement_is_the_oracle_from_zero_and_reused(oracle, dims, niter, nscales, nrefine):
    refs, movs = warm_pairs(dims)
    for k in range(2):
        o = oracle.Registration(dims, niter, nscales, 0, [ALPHA], nrefine, fixed_iters=True)
        levels = zero_levels(dims, nscales)
        seen = []
        for call in range(3):  # the first from zero, then the reused object
            o.register(refs[k], movs[call][k])
            levels, counts, _ = estimate_from(oracle, levels, refs[k], movs[call][k], niter,
                                              nscales, nrefine, ALPHA)
            assert counts == o.iterations()
            want = o.motion()
            assert want.any()
            assert np.array_equal(motion_of(levels[0]), want), f"pair {k}, call {call}"
            seen.append(want)
        o.close()
        # the reuse is live: a fresh object on the last call's images differs
        fresh = oracle.Registration(dims, niter, nscales, 0, [ALPHA], nrefine, fixed_iters=True)
        fresh.register(refs[k], movs[2][k])
        assert not np.array_equal(fresh.motion(), seen[2])
        fresh.close()


def test_restatement_with_convergence_on(oracle):
    """The Logger's break and errors are the oracle's too (its sequential
    float sums), from zero and on the reused object."""
    dims, niter = (40, 24), [200]
    refs, movs = warm_pairs(dims)
    o = oracle.Registration(dims, niter, 0, 0, [ALPHA], 1)
    levels = zero_levels(dims, 0)
    for call in range(3):
        o.register(refs[0], movs[call][0])
        levels, counts, errs = estimate_from(oracle, levels, refs[0], movs[call][0], niter, 0, 1,
                                             ALPHA, fixed=False)
        assert counts == o.iterations() and 2 < counts[0] < 200
        assert np.array_equal(errs, o.last_errors())
        assert np.array_equal(motion_of(levels[0]), o.motion())
    o.close()


def test_downsampled_start_is_what_set_motion_builds(oracle):
    """The start of check 4: {m, downSample(m)} at levels 0 and nscales, the
    levels between overwritten by the estimate itself, whatever they hold."""
    dims, niter, nscales = (40, 24), [4, 5, 6], 2
    refs, movs = warm_pairs(dims)
    o = oracle.Registration(dims, [6], 0, 0, [ALPHA], 1, fixed_iters=True)
    o.register(refs[1], movs[0][1])
    m = field_of(o.motion())
    o.close()
    ldim = level_dims(dims, nscales)
    a = zero_levels(dims, nscales)
    a[0], a[2] = m, downsample_motion(oracle, m, ldim[2])
    b = [x.copy() for x in a]
    b[1][:] = 7.0  # never read: downsampled into before its loop
    ra = estimate_from(oracle, a, refs[1], movs[1][1], niter, nscales, 2, ALPHA)[0]
    rb = estimate_from(oracle, b, refs[1], movs[1][1], niter, nscales, 2, ALPHA)[0]
    assert np.array_equal(ra[0], rb[0]) and ra[0].any()
    zero = estimate_from(oracle, zero_levels(dims, nscales), refs[1], movs[1][1], niter, nscales,
                         2, ALPHA)[0]
    assert not np.array_equal(ra[0], zero[0])
