"""Batched Elastic on the device (BatchRegistration(reg=2)):
every pair of a batch bit for bit the one-pair Elastic registration and the
oracle, at the sizes where the in-workgroup sweep can go wrong; pairs
independent of each other, per-pair convergence, warm start, a launch count
independent of the batch size, more pairs than block slots, and what surrounds
the loop (device I/O, set_motion, the batched analysis)."""
import numpy as np
import pytest

from opticalflow2d_amd import synthetic as S
from test_gpu_batch import make_pairs, ref_of

pytestmark = pytest.mark.gpu

PARAMS = [0.5, 0.25, 0.9]  # lambda != 0, omega not the default


def threads(dx):
    return min((dx + 63) // 64 * 64, 512)


def level_threads(dims, nscales):
    return [threads(int(np.float32(dims[0]) / np.float32(2 ** s))) for s in range(nscales + 1)]


def run_batch(dims, niter, nscales, params, nrefine, refs, movs, **opt):
    from opticalflow2d_amd import BatchRegistration
    with BatchRegistration(len(movs), dims, niter, nscales, params, nrefine, reg=2, device=0,
                           **opt) as b:
        b.register(refs, movs)
        return {"motion": b.motion(), "warp": b.warp(movs), "iters": b.iterations(),
                "status": b.status(), "info": b.info(), "error": b.last_error(),
                "errs": [b.last_errors(k) for k in range(len(movs))]}


def one_pair(dims, niter, nscales, params, nrefine, ref, mov, **opt):
    from opticalflow2d_amd import ImageRegistration
    with ImageRegistration(dims, niter, nscales, 2, params, nrefine, device=0, **opt) as r:
        r.register(ref, mov)
        return {"motion": r.motion(), "warp": r.warp(mov), "iters": r.iterations(),
                "errs": r.last_errors()}


def oracle_pair(O, dims, niter, nscales, params, nrefine, ref, mov, fixed=True):
    o = O.Registration(dims, niter, nscales, 2, params, nrefine, 0, fixed_iters=fixed)
    o.register(ref, mov)
    out = {"motion": o.motion(), "warp": o.warp(mov), "iters": o.iterations(),
           "errs": np.asarray(o.last_errors())}
    o.close()
    return out


def want_iters(niter, nscales, nrefine):
    return [n for n in reversed(niter[: nscales + 1]) for _ in range(nrefine)]


def check(oracle, dims, niter, nscales, params, nrefine, refs, movs, got, one_params=None):
    """got, a fixed_iters batch: every pair against the one-pair path (with
    one_params where the batch's were completed by the class) and the oracle."""
    B = len(movs)
    want = want_iters(niter, nscales, nrefine)
    one_params = params if one_params is None else one_params
    assert got["status"].tolist() == [0] * B and got["error"] == ""
    assert got["info"]["threads"] == level_threads(dims, nscales)
    assert got["info"]["placement"] == [0] * (nscales + 1)
    assert got["iters"].tolist() == [want] * B
    for k in range(B):
        one = one_pair(dims, niter, nscales, one_params, nrefine, ref_of(refs, k), movs[k],
                       fixed_iters=1)
        assert one["iters"] == want
        assert np.array_equal(got["motion"][k], one["motion"]), f"pair {k}: one-pair path"
        assert np.array_equal(got["warp"][k], one["warp"]), f"pair {k}: one-pair warp"
        assert got["errs"][k].size == 0  # fixed_iters: no errors recorded
        o = oracle_pair(oracle, dims, niter, nscales, one_params, nrefine, ref_of(refs, k),
                        movs[k])
        assert o["iters"] == want
        assert np.array_equal(got["motion"][k], o["motion"]), f"pair {k}: oracle"
        assert np.array_equal(got["warp"][k], o["warp"]), f"pair {k}: oracle's warp"


FIXED_CASES = [
    # dims, B, niter, shared reference
    ((3, 3), 2, [5], False),       # one interior pixel
    ((5, 4), 3, [5], False),
    ((63, 9), 2, [4], False),      # the one-pair strip's width
    ((64, 9), 2, [4], True),       # one wave, no barrier
    ((65, 9), 2, [4], False),      # two waves
    ((130, 20), 2, [4], False),    # three waves, barriers
    ((9, 200), 2, [4], False),     # tall: the wavefront longer than wide
    ((1024, 16), 2, [3], False),   # more columns than threads
    ((512, 512), 2, [2], False),   # the largest
]


@pytest.mark.parametrize("dims, B, niter, shared", FIXED_CASES)
def test_fixed_iterations_bit_for_bit(gpu, oracle, dims, B, niter, shared):
    refs, movs = make_pairs(dims, B, shared)
    got = run_batch(dims, niter, 0, PARAMS, 1, refs, movs, fixed_iters=1)
    assert got["motion"].any() or dims == (3, 3)
    check(oracle, dims, niter, 0, PARAMS, 1, refs, movs, got)


@pytest.mark.parametrize("dims", [(2, 7), (7, 2)])
def test_no_interior(gpu, oracle, dims):
    """A level with a side below 3: the sweep relaxes nothing, the motion is +0
    on the bits after the loop's accumulate, as the one-pair path's."""
    refs, movs = make_pairs(dims, 2)
    got = run_batch(dims, [4], 0, PARAMS, 1, refs, movs, fixed_iters=1)
    assert got["motion"].tobytes() == np.zeros_like(got["motion"]).tobytes()
    check(oracle, dims, [4], 0, PARAMS, 1, refs, movs, got)


def test_default_omega_through_the_class(gpu, oracle):
    """[mu, lambda]: the class appends omega = 0.66f, the one-pair path's and
    the reference's default."""
    dims = (40, 33)
    refs, movs = make_pairs(dims, 2)
    got = run_batch(dims, [6], 0, [0.3, 0.1], 1, refs, movs, fixed_iters=1)
    assert got["motion"].any()
    check(oracle, dims, [6], 0, [0.3, 0.1], 1, refs, movs, got)
    other = run_batch(dims, [6], 0, [0.3, 0.1, 0.9], 1, refs, movs, fixed_iters=1)
    assert not np.array_equal(got["motion"], other["motion"])


# the (64, 36) pyramid with two refines: shared by the pyramid, independence
# and launch-count tests
PYR = dict(dims=(64, 36), niter=[5, 6, 7], nscales=2, nrefine=2)
_cache = {}


def pyramid_case(B=7):
    if B not in _cache:
        refs, movs = make_pairs(PYR["dims"], 7)
        _cache.setdefault("in", (refs, movs))
        _cache[B] = run_batch(PYR["dims"], PYR["niter"], PYR["nscales"], PARAMS, PYR["nrefine"],
                              refs[:B], movs[:B], fixed_iters=1)
    return _cache["in"], _cache[B]


def test_pyramid_two_refines(gpu, oracle):
    (refs, movs), got = pyramid_case(7)
    sel = {k: v[:5] if k in ("motion", "warp", "iters", "status", "errs") else v
           for k, v in got.items()}
    check(oracle, PYR["dims"], PYR["niter"], PYR["nscales"], PARAMS, PYR["nrefine"], refs[:5],
          movs[:5], sel)


def test_pairs_do_not_see_each_other(gpu):
    (refs, movs), all7 = pyramid_case(7)
    for k in (0, 3, 6):
        one = run_batch(PYR["dims"], PYR["niter"], PYR["nscales"], PARAMS, PYR["nrefine"],
                        refs[k:k + 1], movs[k:k + 1], fixed_iters=1)
        assert np.array_equal(one["motion"][0], all7["motion"][k])
        assert np.array_equal(one["warp"][0], all7["warp"][k])


def test_launch_count_does_not_depend_on_batch_size(gpu):
    _, one = pyramid_case(1)
    _, five = pyramid_case(5)
    nscales, loops = PYR["nscales"], 6
    # max(nscales - 1, 0) downsamples + 4 per loop + nscales upsamples + 1 zeroing
    formula = max(nscales - 1, 0) + 4 * loops + nscales + 1
    assert one["info"]["launches"] == five["info"]["launches"] == formula
    assert one["info"]["loops"] == five["info"]["loops"] == loops
    assert five["info"]["placement"] == [0, 0, 0]
    assert five["info"]["threads"] == [64, 64, 64]


def test_more_pairs_than_block_slots(gpu):
    """1100 workgroups (the count tests/test_gpu_batch.py uses): more than the
    device holds at a time, so the grid takes further rounds of blocks."""
    dims, niter, B = (8, 8), [2], 1100
    both = [S.texture_pair(8, seed=7, sigma=1.5, shift=sh, ny=8)
            for sh in [(0.5, 0.25), (-0.75, 0.5), (1.25, -1.0), (0.1, 0.9)]]
    ref, four = both[0][0], [m for _, m in both]
    which = (np.arange(B) * 7 + np.arange(B) // 256) % 4
    movs = np.stack([four[w] for w in which])
    got = run_batch(dims, niter, 0, PARAMS, 1, ref, movs, fixed_iters=1)
    assert not got["status"].any()
    assert got["iters"].tolist() == [[2]] * B
    for k in (0, B // 2, B - 1):
        one = run_batch(dims, niter, 0, PARAMS, 1, ref, movs[k:k + 1], fixed_iters=1)
        assert one["motion"].any()
        assert np.array_equal(got["motion"][k], one["motion"][0])
        assert np.array_equal(got["warp"][k], one["warp"][0])
    # every pair with the same moving image has the same bits
    for w in range(4):
        sel = which == w
        assert np.array_equal(got["motion"][sel],
                              np.broadcast_to(got["motion"][sel][0], got["motion"][sel].shape))


def test_zero_in_zero_out(gpu):
    dims = (16, 32)
    refs, _ = make_pairs(dims, 3)
    got = run_batch(dims, [4], 0, PARAMS, 1, refs, refs.copy(), fixed_iters=1)
    assert got["motion"].tobytes() == np.zeros_like(got["motion"]).tobytes()  # +0 on the bits


# ------------------------------------------------------------ convergence
CONV_DIMS = (48, 32)
CONV_PARAMS = [0.05, 0.02, 1.5]
CONV_CAP = 400
CONV_INPUTS = [(41, (1.1, -0.6)), (50, (2.0, 1.3)), (71, (1.1, -0.6)), (75, (2.0, 1.3))]
CONV_COUNTS = [94, 82, 68, 78]


def test_convergence_per_pair(gpu, oracle):
    """Each pair stops on its own iteration: the oracle's and the one-pair
    path's (``logger_fp64=1``).

    The inputs were chosen on the CPU with the oracle (seeds 40 to 89 of
    texture_pair(48, sigma=2.5, ny=32), the shift by seed % 5 from (2.0, 1.3),
    (1.1, -0.6), (0.3, 0.2), (0.7, 0.9), (1.5, -0.75), a cap of 400) so that the
    oracle's error keeps at least 1e-5 from 0.001 at the breaking iteration and
    at the one before it; an equal count is therefore not luck (the fp64 sums
    and the oracle's float sum differ in an error's last bits).  With
    tests/test_gpu_fluid.py's [0.1, 0.0] and omega 0.66 the error falls by
    about 7e-6 an iteration where it crosses 0.001 (after some 300
    iterations), so no input keeps that distance on both sides; mu 0.05,
    lambda 0.02 and omega 1.5 cross it after 60 to 110 iterations in steps of
    4e-5 to 7e-5, and 24 of the 50 seeds qualify.  Recorded, error - 0.001
    before / at the break:
      seed 41, shift (1.1, -0.6): 94 iterations, +2.23e-5 / -1.70e-5
      seed 50, shift (2.0, 1.3):  82 iterations, +2.16e-5 / -2.43e-5
      seed 71, shift (1.1, -0.6): 68 iterations, +2.61e-5 / -3.03e-5
      seed 75, shift (2.0, 1.3):  78 iterations, +3.08e-5 / -1.95e-5
    The test asserts the margins again on the oracle's own errors."""
    pairs = [S.texture_pair(CONV_DIMS[0], seed=s, sigma=2.5, shift=sh, ny=CONV_DIMS[1])
             for s, sh in CONV_INPUTS]
    refs, movs = np.stack([r for r, _ in pairs]), np.stack([m for _, m in pairs])
    B = len(movs)
    got = run_batch(CONV_DIMS, [CONV_CAP], 0, CONV_PARAMS, 1, refs, movs)
    assert got["status"].tolist() == [0] * B
    assert len(set(CONV_COUNTS)) == B == 4
    for k in range(B):
        o = oracle_pair(oracle, CONV_DIMS, [CONV_CAP], 0, CONV_PARAMS, 1, refs[k], movs[k],
                        fixed=False)
        n = CONV_COUNTS[k]
        assert o["iters"] == [n]
        e = o["errs"].astype(np.float64)
        assert e[n - 2] - 0.001 >= 1e-5 and 0.001 - e[n - 1] >= 1e-5
        one = one_pair(CONV_DIMS, [CONV_CAP], 0, CONV_PARAMS, 1, refs[k], movs[k], logger_fp64=1)
        assert one["iters"] == [n]
        assert got["iters"][k].tolist() == [n], f"pair {k}"
        assert np.array_equal(got["motion"][k], one["motion"]), f"pair {k}"
        # the bar tests/test_gpu_batch.py applies to Diffusion's errors: one float32 ulp
        eb, e1 = got["errs"][k], np.asarray(one["errs"], np.float32)
        assert eb.shape == e1.shape == (n,)
        assert np.all(np.abs(eb.astype(np.float64) - e1.astype(np.float64))
                      <= np.spacing(e1).astype(np.float64)), f"pair {k}"
    # two calls give the same bits
    again = run_batch(CONV_DIMS, [CONV_CAP], 0, CONV_PARAMS, 1, refs, movs)
    assert np.array_equal(again["motion"], got["motion"])
    assert all(np.array_equal(a, b) for a, b in zip(again["errs"], got["errs"]))


# ------------------------------------------------------------ warm start, surroundings
def test_warm_start_is_a_reused_one_pair_object(gpu):
    from opticalflow2d_amd import BatchRegistration, ImageRegistration
    dims, niter = (70, 20), [5]
    refs, movs = make_pairs(dims, 3)
    with BatchRegistration(3, dims, niter, 0, PARAMS, reg=2, device=0, fixed_iters=1,
                           warm_start=1) as b:
        b.register(refs, movs)
        first = b.motion()
        b.register(refs, movs)
        second = b.motion()
        assert b.info()["launches"] == 4 + 1
    assert not np.array_equal(first, second)
    for k in range(3):
        with ImageRegistration(dims, niter, 0, 2, PARAMS, fixed_iters=1, device=0) as r:
            r.register(refs[k], movs[k])
            assert np.array_equal(first[k], r.motion())
            r.register(refs[k], movs[k])
            assert np.array_equal(second[k], r.motion()), f"pair {k}"


def test_device_io(gpu):
    import torch
    from opticalflow2d_amd import BatchRegistration
    dims, niter = (37, 29), [4]
    refs, movs = make_pairs(dims, 3)
    host = run_batch(dims, niter, 0, PARAMS, 1, refs, movs, fixed_iters=1)
    with BatchRegistration(3, dims, niter, 0, PARAMS, reg=2, device=0, fixed_iters=1) as b:
        b.register(torch.as_tensor(refs, device="cuda:0"), torch.as_tensor(movs, device="cuda:0"))
        torch.cuda.synchronize()
        assert np.array_equal(b.motion(), host["motion"])
        md = b.motion_device()
        assert md.is_cuda
        assert np.array_equal(md.cpu().numpy().astype(np.float64), host["motion"])
        wd = b.warp(torch.as_tensor(movs, device="cuda:0"))
        assert np.array_equal(wd.cpu().numpy(), host["warp"])


def test_set_motion_of_get_motion_is_the_identity(gpu):
    from opticalflow2d_amd import BatchRegistration
    dims, niter = (37, 29), [4]
    refs, movs = make_pairs(dims, 3)
    with BatchRegistration(3, dims, niter, 0, PARAMS, reg=2, device=0, fixed_iters=1) as b:
        b.register(refs, movs)
        m, w = b.motion(), b.warp(movs)
        assert m.any()
        b.reset_motion()
        assert b.motion().tobytes() == np.zeros_like(m).tobytes()
        b.set_motion(m)
        assert np.array_equal(b.motion(), m) and np.array_equal(b.warp(movs), w)


def test_analysis_agrees_with_the_one_pair_entries(gpu):
    from opticalflow2d_amd import BatchRegistration, ImageRegistration
    dims, niter = (37, 29), [6]
    refs, movs = make_pairs(dims, 3)
    n = dims[0] * dims[1]
    with BatchRegistration(3, dims, niter, 0, PARAMS, reg=2, device=0, fixed_iters=1) as b:
        b.register(refs, movs)
        m0 = b.motion()
        jac, st = b.jacobian()
        inv, info = b.inverse_motion()
        q = b.quality(refs, movs)
        assert np.array_equal(b.motion(), m0)  # the analysis leaves the motion alone
    k = 1
    with ImageRegistration(dims, niter, 0, 2, PARAMS, 1, fixed_iters=1, device=0) as r:
        r.register(refs[k], movs[k])
        wjac, wst = r.jacobian()
        winv, winfo = r.inverse_motion()
        wq = r.quality(refs[k], movs[k])
    assert np.array_equal(np.asarray(jac[k], np.float64).view(np.uint64), wjac.view(np.uint64))
    for key in ("min", "max", "folded", "below_half"):
        assert st[k][key] == wst[key], key
    # a mean of n float32 values summed in fp64 in two orders (test_gpu_batch_analysis.py)
    assert abs(st[k]["mean"] - wst["mean"]) <= 4 * n * 2.0 ** -53 * np.abs(wjac).mean()
    assert np.array_equal(np.asarray(inv[k], np.float64).view(np.uint64), winv.view(np.uint64))
    assert info[k] == winfo
    # each within 1e-11 of the exact value (test_gpu_batch_analysis.py), so 2e-11 apart
    for key, want in wq.items():
        assert abs(q[k][key] - want) <= 2e-11 * abs(want), key
