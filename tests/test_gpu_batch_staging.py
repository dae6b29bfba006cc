"""A batch whose host forms need more than one staging round (batch.cpp: the
loops over rounds in set_images, get_motion, set_motion, warp, jacobian,
invert_motion and quality).  The staging buffer holds 8 Mi doubles, a motion
field of ``8 Mi / (2 * dimx * dimy)`` pairs; every other GPU test fits one
round.  Here 35 pairs of (512, 509), the largest ragged size the batch takes,
go through rounds of 16, 16 and 3; a shared reference through one.

Every pair differs from every other: three textured pairs tiled, the moving
image of pair k offset by ``OFFSET * k`` (asserted below), so a pair that lands
in another pair's slot, at whatever distance, gives other bits.  Expected values
come from a one-pair ImageRegistration with the same options on each distinct
input, registered once and cached; tests/test_gpu_batch.py holds the two paths
to each other and to the oracle at small shapes.  Everything is compared bit
for bit but the reordered fp64 sums (the Jacobian mean, MSE and NCC), whose
bounds are derived where they are used.
"""
import time

import numpy as np
import pytest

from test_gpu_batch import ALPHA, make_pairs
from test_gpu_batch_analysis import image32, numpy_similarity

pytestmark = pytest.mark.gpu

DIMS = (512, 509)
B = 35
NITER, NSCALES = [2], 0
OFFSET = 0.002       # pair k's moving image is its texture's + OFFSET * k
INVERT_ITERS = 3
U = 2.0 ** -53

_cache = {}


def stage_pairs(dimx, dimy):
    """batch_plan.h stage_chunk_pairs, before the cap at nbatch."""
    return max(1, (8 << 20) // (2 * dimx * dimy))


def inputs():
    """``(refs [3], movs [B], which, M [B])``: the three references, every
    pair's moving image, the reference of pair k is ``refs[which[k]]``; M: a
    motion per pair to supply, float32 values."""
    if "in" not in _cache:
        refs, base = make_pairs(DIMS, 3)
        which = np.arange(B) % 3
        movs = base[which] + OFFSET * np.arange(B)[:, None, None]
        rng = np.random.default_rng(31)
        m3 = rng.standard_normal((3,) + DIMS + (2,)).astype(np.float32)
        M = m3[which] + (0.125 * np.arange(B, dtype=np.float32))[:, None, None, None]
        assert M.dtype == np.float32
        # no two pairs' inputs are equal, three pairs apart or otherwise: equal
        # arrays would have equal sums
        for a in (movs, M):
            sums = a.reshape(B, -1).sum(axis=1, dtype=np.float64)
            assert len(set(sums.tolist())) == B, sums
        for a in (refs, movs, M):
            a.flags.writeable = False
        _cache["in"] = refs, movs, which, M
    return _cache["in"]


def one_pair(keys, full=True):
    """The one-pair results of ``(reference index, pair)`` inputs, each input
    registered once: the cold estimate's motion and, with ``full``, its warp
    and analysis, then the estimate continued from the supplied M[pair]."""
    from opticalflow2d_amd import ImageRegistration
    refs, movs, _, M = inputs()
    todo = [k for k in keys if (k, full) not in _cache and (k, True) not in _cache]
    t0 = time.perf_counter()
    if todo:
        with ImageRegistration(DIMS, NITER, NSCALES, 0, [ALPHA], 1, fixed_iters=1, device=0) as r:
            for key in todo:
                ri, k = key
                r.reset_motion()
                r.register(refs[ri], movs[k])
                res = {"motion": r.motion()}
                if full:
                    res["warp"] = r.warp(movs[k])
                    res["jac"], res["jst"] = r.jacobian()
                    res["inv"], res["info"] = r.inverse_motion(max_iter=INVERT_ITERS)
                    res["q"] = r.quality(refs[ri], movs[k])
                    r.set_motion(M[k])
                    res["set"] = r.motion()
                    r.register(refs[ri], movs[k])
                    res["warm"] = r.motion()
                _cache[key, full] = res
        print(f"one-pair reference: {len(todo)} inputs at {DIMS}, full={full}: "
              f"{time.perf_counter() - t0:.2f} s")
    return [_cache.get((k, True)) or _cache[k, full] for k in keys]


def batch():
    from opticalflow2d_amd import BatchRegistration
    return BatchRegistration(B, DIMS, NITER, NSCALES, ALPHA, 1, fixed_iters=1, device=0)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, what
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), what


def test_the_case_needs_three_rounds():
    """On the CPU: the round arithmetic this module relies on."""
    from opticalflow2d_amd.batch import BATCH_MAXPX
    dimx, dimy = DIMS
    assert dimx * dimy <= BATCH_MAXPX < dimx * (dimy + 4) and dimy % 64 and dimy % 4
    stage = stage_pairs(dimx, dimy)
    assert stage == 16
    assert B > 2 * stage and B % stage == 3 and -(-B // stage) == 3


def test_register_motion_warp_set_motion(gpu):
    refs, movs, which, M = inputs()
    t0 = time.perf_counter()
    want = one_pair([(int(which[k]), k) for k in range(B)])
    t1 = time.perf_counter()
    assert all(w["motion"].any() for w in want)
    for k in range(1, B):  # a pair in another's slot would show
        assert not np.array_equal(want[k]["motion"], want[k - 1]["motion"])
        assert not np.array_equal(want[k]["motion"], want[k - 3 if k >= 3 else 0]["motion"])
    with batch() as b:
        b.register(refs[which], movs)
        assert b.status().tolist() == [0] * B and b.last_error() == ""
        assert b.iterations().tolist() == [NITER] * B
        got_m, got_w = b.motion(), b.warp(movs)
        for k in range(B):
            same_bits(got_m[k], want[k]["motion"], f"pair {k}: motion")
            same_bits(got_w[k], want[k]["warp"], f"pair {k}: warp")
        # a supplied motion, distinct per pair, comes back as it went in
        b.set_motion(M)
        back = b.motion()
        assert np.array_equal(back.astype(np.float32).view(np.uint32), M.view(np.uint32))
        assert np.array_equal(back, M.astype(np.float64))
        for k in range(B):
            same_bits(back[k], want[k]["set"], f"pair {k}: set_motion")
        # and the estimate continues from it as the one-pair path's does
        b.set_option("warm_start", 1)
        b.register(refs[which], movs)
        assert b.status().tolist() == [0] * B
        got = b.motion()
        for k in range(B):
            same_bits(got[k], want[k]["warm"], f"pair {k}: warm estimate")
            assert not np.array_equal(got[k], want[k]["motion"])
    print(f"staging test: one-pair references {t1 - t0:.2f} s, batch part "
          f"{time.perf_counter() - t1:.2f} s")


def test_analysis_host_forms(gpu):
    from opticalflow2d_amd.prims import prim
    refs, movs, which, _ = inputs()
    want = one_pair([(int(which[k]), k) for k in range(B)])
    n = DIMS[0] * DIMS[1]
    with batch() as b:
        b.register(refs[which], movs)
        jac, st = b.jacobian()
        none, st2 = b.jacobian(jac=False)
        inv, info = b.inverse_motion(max_iter=INVERT_ITERS)
        q = b.quality(refs[which], movs)
        qs = b.quality(refs[0], movs)
        warped = b.warp(movs)
        assert b.status().tolist() == [0] * B
    assert none is None and st2 == st
    r32 = np.stack([image32(refs[i]) for i in range(3)])
    m32 = np.stack([image32(movs[k]) for k in range(B)])
    w32 = np.stack([image32(warped[k]) for k in range(B)])
    # the batch's own kernel on the same float images, one launch, no rounds:
    # a pair's sums are taken in a fixed order, so the words are the same
    before = prim.batch_similarity(r32[which], m32)
    after = prim.batch_similarity(r32[which], w32)
    shared_before = prim.batch_similarity(r32[0], m32)
    for k in range(B):
        w, what = want[k], f"pair {k}"
        same_bits(jac[k], w["jac"], f"{what}: jacobian map")
        for key in ("min", "max", "folded", "below_half"):
            assert st[k][key] == w["jst"][key], (what, key)
        # an fp64 sum of n terms taken in another order: 2 n 2^-53 mean|J|
        mean = w["jac"].mean()
        bound = 2 * n * U * np.abs(w["jac"]).mean()
        print(f"{what}: mean {st[k]['mean']!r} one-pair {w['jst']['mean']!r} numpy {mean!r} "
              f"bound {bound:.3e}")
        assert abs(st[k]["mean"] - mean) <= bound, what
        same_bits(inv[k], w["inv"], f"{what}: inverse")
        assert info[k] == w["info"], what
        assert (q[k]["mse_before"], q[k]["ncc_before"]) == tuple(before[k]), what
        assert (q[k]["mse_after"], q[k]["ncc_after"]) == tuple(after[k]), what
        assert (qs[k]["mse_before"], qs[k]["ncc_before"]) == tuple(shared_before[k]), what
        # against the one-pair entry: both take the six sums of the covariance
        # form over n non-negative terms each, in different orders.  Each sum
        # is within n u of exact, two orders within 2 n u of each other, so
        # MSE agrees to 2 n u (and a division's rounding).  A variance or the
        # covariance, s2 - s0^2 / n, moves by at most 6 n u E[x^2]; relative
        # to sqrt(va vb) that is 6 n u kappa with kappa = max E[x^2] / Var x
        # over the two images, and NCC = cab / sqrt(va vb) moves by at most
        # 6 n u kappa (1 + |NCC|) <= 12 n u kappa.
        ref = r32[which[k]].astype(np.float64)
        for tag, img in (("before", m32[k]), ("after", w32[k])):
            x = img.astype(np.float64)
            kappa = max((ref * ref).mean() / ref.var(), (x * x).mean() / x.var())
            gm, gn = q[k][f"mse_{tag}"], q[k][f"ncc_{tag}"]
            wm, wn = w["q"][f"mse_{tag}"], w["q"][f"ncc_{tag}"]
            print(f"{what} {tag}: mse {gm!r} one-pair {wm!r}; ncc {gn!r} one-pair {wn!r}; "
                  f"numpy {numpy_similarity(ref, x)}; kappa {kappa:.2f}")
            assert abs(gm - wm) <= (2 * n + 2) * U * wm, (what, tag)
            assert abs(gn - wn) <= 12 * n * U * kappa, (what, tag)
    # pairs three apart are told apart by the analysis too
    assert all(q[k]["mse_before"] != q[k - 3]["mse_before"] for k in range(3, B))


def test_shared_reference(gpu):
    """One round of one image for the reference, three for the moving stack."""
    refs, movs, _, _ = inputs()
    want = one_pair([(0, k) for k in range(B)], full=False)
    with batch() as b:
        b.register(refs[0], movs)
        assert b.status().tolist() == [0] * B
        got = b.motion()
    for k in range(B):
        same_bits(got[k], want[k]["motion"], f"pair {k}")
