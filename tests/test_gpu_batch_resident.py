"""The batch option "resident" on the device (BatchRegistration resident=1,
DESIGN.md §4.6.5): the Horn-Schunck loop with the pair's iterate in LDS and
dI, It in registers.  Every result is held, with np.array_equal, to the oracle,
to the one-pair ImageRegistration and to the same batch with resident=0:
fixed iterations at the sizes where the kernel takes another path, convergence
per pair (counts and errors on their bits), a divide-by-zero pair, more pairs
than resident workgroups, the option switched on one handle, and a warm
start.  info()["placement"] is exactly what the fit rule predicts."""
import numpy as np
import pytest

from opticalflow2d_amd import synthetic as S

pytestmark = pytest.mark.gpu

ALPHA = 0.1


def level_dims(dims, nscales):
    """ImageRegistration.cpp:56-61: dim / scale with a float scale, per level."""
    return [(int(np.float32(dims[0]) / np.float32(2.0 ** s)),
             int(np.float32(dims[1]) / np.float32(2.0 ** s))) for s in range(nscales + 1)]


def fits(dx, dy):
    """The fit rule of batch_plan.h (resident_fits), restated: the iterate's one
    LDS copy with its ghost ring plus 1 KiB of reduction scratch within the
    CU's 160 KiB, and at most 16 pixels for each of the 1024 threads."""
    return (dx + 2) * (dy + 2) * 8 + 1024 <= 160 * 1024 and dx * dy <= 16 * 1024


def placement_of(dims, nscales):
    return [1 if fits(dx, dy) else 0 for dx, dy in level_dims(dims, nscales)]


def test_the_fit_rule_restated():
    assert fits(128, 128) and fits(3, 5) and fits(9, 300) and fits(130, 17) and fits(65, 8)
    assert fits(64, 64) and not fits(256, 256) and not fits(129, 128)
    assert not fits(150, 120)  # the bytes fit, the pixels per thread do not
    assert not fits(2, 6000)   # the pixels fit, the bytes do not
    assert placement_of((256, 256), 2) == [0, 1, 1]


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


# ------------------------------------------------------------ 1. fixed iterations
FIXED_CASES = [
    # dims, B, niter, nscales, nrefine, shared reference
    ((3, 5), 2, [4], 0, 1, False),      # fewer pixels than threads, all on the border
    ((40, 33), 3, [7], 0, 1, False),    # no multiple of a wave; the result in est[1]
    ((40, 33), 3, [8], 0, 1, False),    # ... and in est[0]
    ((128, 128), 2, [5], 0, 1, False),  # the largest level of the rule: 16 pixels per thread
    ((130, 17), 5, [6, 9], 1, 1, True),  # wider than the pitch unit; level 1 is (65, 8)
    ((256, 256), 2, [3, 4, 5], 2, 2, False),  # placement [0, 1, 1], two refines
    ((9, 300), 2, [5], 0, 1, False),    # tall and narrow: many short rows
]


@pytest.mark.parametrize("dims, B, niter, nscales, nrefine, shared", FIXED_CASES)
def test_fixed_iterations_bit_for_bit(gpu, oracle, dims, B, niter, nscales, nrefine, shared):
    from opticalflow2d_amd import ImageRegistration
    refs, movs = make_pairs(dims, B, shared)
    got = run_batch(dims, niter, nscales, ALPHA, nrefine, refs, movs, fixed_iters=1, resident=1)
    glob = run_batch(dims, niter, nscales, ALPHA, nrefine, refs, movs, fixed_iters=1, resident=0)
    want_place = placement_of(dims, nscales)
    assert any(want_place)
    assert got["info"]["placement"] == want_place
    assert glob["info"]["placement"] == [0] * (nscales + 1)
    assert got["info"]["threads"] == glob["info"]["threads"] == [1024] * (nscales + 1)
    assert got["info"]["launches"] == glob["info"]["launches"]
    want_iters = [n for n in reversed(niter[: nscales + 1]) for _ in range(nrefine)]
    assert got["status"].tolist() == [0] * B and got["error"] == ""
    assert got["iters"].tolist() == [want_iters] * B
    # against placement 0
    assert np.array_equal(got["motion"], glob["motion"])
    assert np.array_equal(got["warp"], glob["warp"])
    for k in range(B):
        # against the oracle
        m, w, it = oracle_pair(oracle, dims, niter, nscales, ALPHA, nrefine, ref_of(refs, k),
                               movs[k])
        assert it == want_iters
        assert m.any()
        assert np.array_equal(got["motion"][k], m), f"pair {k}: motion differs from the oracle"
        assert np.array_equal(got["warp"][k], w), f"pair {k}: warp differs from the oracle"
        # against the one-pair path
        with ImageRegistration(dims, niter, nscales, 0, [ALPHA], nrefine, fixed_iters=1,
                               device=0) as r:
            r.register(ref_of(refs, k), movs[k])
            assert np.array_equal(got["motion"][k], r.motion()), f"pair {k}: one-pair path"
            assert np.array_equal(got["warp"][k], r.warp(movs[k]))
        assert got["errs"][k].size == 0  # fixed_iters: no errors recorded


# ------------------------------------------------------------ 2. convergence
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
def test_convergence_equals_placement_0(gpu, dims, niter, nscales):
    """The pixel-to-thread mapping and the reduction tree are placement 0's, so
    the errors (on their float32 bits), the counts and the fields are too."""
    refs, movs = conv_pairs(dims)
    B = len(movs)
    got = run_batch(dims, niter, nscales, CONV_ALPHA, 1, refs, movs, resident=1)
    glob = run_batch(dims, niter, nscales, CONV_ALPHA, 1, refs, movs, resident=0)
    assert got["info"]["placement"] == [1] * (nscales + 1)
    assert glob["info"]["placement"] == [0] * (nscales + 1)
    assert got["info"]["threads"] == [1024] * (nscales + 1)
    assert got["status"].tolist() == glob["status"].tolist() == [0] * B
    assert np.array_equal(got["iters"], glob["iters"])
    # the per-pair break is exercised: four different counts below the cap
    last = got["iters"][:, -1].tolist()
    assert len(set(last)) == B and all(2 < n < niter[0] for n in last), last
    for k in range(B):
        assert got["errs"][k].size == last[k]
        assert np.array_equal(got["errs"][k].view(np.uint32), glob["errs"][k].view(np.uint32)), k
    assert np.array_equal(got["motion"], glob["motion"])
    assert np.array_equal(got["warp"], glob["warp"])


# ------------------------------------------------------------ 3. divide by zero
def test_divide_by_zero_is_per_pair(gpu, oracle):
    dims, niter = (40, 33), [5]
    refs, movs = make_pairs(dims, 4)
    bad = 2
    refs[bad] = 0.5
    movs[bad] = 0.5
    got = run_batch(dims, niter, 0, 0.0, 1, refs, movs, fixed_iters=1, resident=1)
    glob = run_batch(dims, niter, 0, 0.0, 1, refs, movs, fixed_iters=1, resident=0)
    assert got["info"]["placement"] == [1]
    from opticalflow2d_amd import _lib
    want = [_lib.OF2D_OK] * 4
    want[bad] = _lib.OF2D_ERR_RUNTIME
    assert got["status"].tolist() == glob["status"].tolist() == want
    assert got["error"] == glob["error"]
    assert "Divide by zero exception" in got["error"] and f"pair {bad}" in got["error"]
    assert not got["motion"][bad].any() and not glob["motion"][bad].any()
    assert np.array_equal(got["iters"], glob["iters"])
    for k in range(4):
        if k == bad:
            continue
        m, w, _ = oracle_pair(oracle, dims, niter, 0, 0.0, 1, refs[k], movs[k])
        assert np.array_equal(got["motion"][k], m), f"pair {k}"
        assert np.array_equal(got["warp"][k], w), f"pair {k}"


# ------------------------------------------------------------ 4. many pairs
def test_more_pairs_than_resident_workgroups(gpu, oracle):
    """600 workgroups of 66 * 66 * 8 B = 34 848 B of LDS each: a CU's 160 KiB
    hold four of them and its 32 wave slots two, so the 256 CUs hold 512 at a
    time and the grid takes a second round of blocks."""
    dims, niter, B = (64, 64), [3], 600
    both = [S.texture_pair(64, seed=7, sigma=2.0, shift=sh, ny=64)
            for sh in [(0.5, 0.25), (-0.75, 0.5), (1.25, -1.0), (0.1, 0.9)]]
    ref, four = both[0][0], [m for _, m in both]
    which = (np.arange(B) * 7 + np.arange(B) // 256) % 4
    movs = np.stack([four[w] for w in which])
    got = run_batch(dims, niter, 0, ALPHA, 1, ref, movs, fixed_iters=1, resident=1)
    assert not got["status"].any()
    assert got["info"]["placement"] == [1] and got["info"]["threads"] == [1024]
    assert got["iters"].tolist() == [[3]] * B
    for w in range(4):
        m, wimg, _ = oracle_pair(oracle, dims, niter, 0, ALPHA, 1, ref, four[w])
        sel = which == w
        assert sel.sum() > 100
        assert np.array_equal(got["motion"][sel], np.broadcast_to(m, (sel.sum(),) + m.shape))
        assert np.array_equal(got["warp"][sel], np.broadcast_to(wimg, (sel.sum(),) + wimg.shape))


# ------------------------------------------------------------ 5. switching
def test_switching_on_one_handle(gpu, oracle):
    from opticalflow2d_amd import BatchRegistration
    dims, niter, nscales = (130, 17), [6, 9], 1
    refs, movs = make_pairs(dims, 3)
    with BatchRegistration(3, dims, niter, nscales, ALPHA, 1, device=0, fixed_iters=1,
                           resident=1) as b:
        b.register(refs, movs)
        first, p1 = b.motion(), b.info()["placement"]
        b.set_option("resident", 0)
        b.register(refs, movs)
        second, p2 = b.motion(), b.info()["placement"]
        b.set_option("resident", 1)
        b.register(refs, movs)
        third, p3 = b.motion(), b.info()["placement"]
    assert (p1, p2, p3) == ([1, 1], [0, 0], [1, 1])
    assert np.array_equal(first, second) and np.array_equal(first, third)
    m, _, _ = oracle_pair(oracle, dims, niter, nscales, ALPHA, 1, refs[1], movs[1])
    assert np.array_equal(first[1], m)


# ------------------------------------------------------------ 6. warm start
def test_warm_start_two_frames(gpu):
    from opticalflow2d_amd import BatchRegistration
    dims, niter = (40, 33), [7]
    refs, movs1 = make_pairs(dims, 3)
    _, movs2 = make_pairs(dims, 3, extra=0.6)
    out = {}
    for resident in (1, 0):
        with BatchRegistration(3, dims, niter, 0, ALPHA, 1, device=0, fixed_iters=1,
                               warm_start=1, resident=resident) as b:
            b.register(refs, movs1)
            one = b.motion()
            b.register(refs, movs2)
            out[resident] = (one, b.motion(), b.info()["placement"])
    assert out[1][2] == [1] and out[0][2] == [0]
    assert np.array_equal(out[1][0], out[0][0])
    assert np.array_equal(out[1][1], out[0][1])
    # the warm start is live: the second frame moved on from the first
    assert not np.array_equal(out[1][0], out[1][1])
    with BatchRegistration(3, dims, niter, 0, ALPHA, 1, device=0, fixed_iters=1,
                           resident=1) as b:
        b.register(refs, movs2)
        assert not np.array_equal(b.motion(), out[1][1])
