"""Batched Curvature on the device (BatchRegistration(reg=1), DESIGN.md
§4.6.7): every pair of a batch bit for bit the one-pair ``curvature_dct=1``
registration and within the project's Curvature bar of the oracle (max |du| <=
1e-5 px, tests/test_gpu_curvature.py), pairs independent of each other,
per-pair convergence, warm start, a launch count independent of the batch
size, more pairs than block slots, and device I/O."""
import numpy as np
import pytest

from opticalflow2d_amd import synthetic as S
from test_gpu_batch import make_pairs, ref_of

pytestmark = pytest.mark.gpu

PARAMS = [0.5, 0.2]
TOL = 1e-5
THREADS = 512


def run_batch(dims, niter, nscales, params, nrefine, refs, movs, **opt):
    from opticalflow2d_amd import BatchRegistration
    with BatchRegistration(len(movs), dims, niter, nscales, params, nrefine, reg=1, device=0,
                           **opt) as b:
        b.register(refs, movs)
        return {"motion": b.motion(), "warp": b.warp(movs), "iters": b.iterations(),
                "status": b.status(), "info": b.info(), "error": b.last_error(),
                "errs": [b.last_errors(k) for k in range(len(movs))]}


def one_pair(dims, niter, nscales, params, nrefine, ref, mov, **opt):
    from opticalflow2d_amd import ImageRegistration
    with ImageRegistration(dims, niter, nscales, 1, params, nrefine, curvature_dct=1, device=0,
                           **opt) as r:
        r.register(ref, mov)
        paths = r.curvature_paths()
        assert paths and all(p[2] == 1 and p[3] == 1 for p in paths), paths  # fast on both axes
        return {"motion": r.motion(), "warp": r.warp(mov), "iters": r.iterations(),
                "errs": r.last_errors()}


def oracle_pair(O, dims, niter, nscales, params, nrefine, ref, mov, fixed=True):
    o = O.Registration(dims, niter, nscales, 1, params, nrefine, 0, fixed_iters=fixed)
    o.register(ref, mov)
    out = {"motion": o.motion(), "iters": o.iterations(), "errs": np.asarray(o.last_errors())}
    o.close()
    return out


def want_iters(niter, nscales, nrefine):
    return [n for n in reversed(niter[: nscales + 1]) for _ in range(nrefine)]


def check(oracle, dims, niter, nscales, params, nrefine, refs, movs, got, with_oracle=True):
    B = len(movs)
    want = want_iters(niter, nscales, nrefine)
    assert got["status"].tolist() == [0] * B and got["error"] == ""
    assert got["info"]["threads"] == [THREADS] * (nscales + 1)
    assert got["info"]["placement"] == [0] * (nscales + 1)
    assert got["iters"].tolist() == [want] * B
    for k in range(B):
        one = one_pair(dims, niter, nscales, params, nrefine, ref_of(refs, k), movs[k],
                       fixed_iters=1)
        assert one["iters"] == want
        assert np.array_equal(got["motion"][k], one["motion"]), f"pair {k}: one-pair path"
        assert np.array_equal(got["warp"][k], one["warp"]), f"pair {k}: one-pair warp"
        assert got["errs"][k].size == 0  # fixed_iters: no errors recorded
        if with_oracle:
            o = oracle_pair(oracle, dims, niter, nscales, params, nrefine, ref_of(refs, k), movs[k])
            assert o["iters"] == want
            d = np.abs(got["motion"][k] - o["motion"]).max()
            assert d <= TOL, f"pair {k}: {d} px from the oracle"


FIXED_CASES = [
    # dims, B, niter, shared reference, against the oracle too
    ((8, 8), 1, [5], False, True),       # one radix-4 pass, fewer pixels than threads
    ((16, 8), 3, [5], False, True),      # a trailing radix-2 pass along x
    ((32, 64), 3, [4], False, True),
    ((128, 16), 4, [4], True, True),     # a y pass in eight chunks of columns
    # the longest line and the largest scratch; the oracle's naive sums are too
    # slow here: the one-pair path only
    ((512, 512), 2, [3], False, False),
]


@pytest.mark.parametrize("dims, B, niter, shared, with_oracle", FIXED_CASES)
def test_fixed_iterations_bit_for_bit(gpu, oracle, dims, B, niter, shared, with_oracle):
    refs, movs = make_pairs(dims, B, shared)
    got = run_batch(dims, niter, 0, PARAMS, 1, refs, movs, fixed_iters=1)
    check(oracle, dims, niter, 0, PARAMS, 1, refs, movs, got, with_oracle)


# the (64, 32) pyramid with two refines: shared by the pyramid, independence
# and launch-count tests
PYR = dict(dims=(64, 32), niter=[5, 6, 7], nscales=2, nrefine=2)
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


def test_default_tau_is_one(gpu):
    dims = (16, 8)
    refs, movs = make_pairs(dims, 2)
    a = run_batch(dims, [4], 0, [0.5], 1, refs, movs, fixed_iters=1)
    b = run_batch(dims, [4], 0, [0.5, 1.0], 1, refs, movs, fixed_iters=1)
    c = run_batch(dims, [4], 0, [0.5, 0.5], 1, refs, movs, fixed_iters=1)
    assert np.array_equal(a["motion"], b["motion"]) and a["motion"].any()
    assert not np.array_equal(a["motion"], c["motion"])
    one = one_pair(dims, [4], 0, [0.5], 1, refs[1], movs[1], fixed_iters=1)
    assert np.array_equal(a["motion"][1], one["motion"])


def test_pairs_do_not_see_each_other(gpu):
    (refs, movs), all7 = pyramid_case(7)
    for k in (0, 3, 6):
        one = run_batch(PYR["dims"], PYR["niter"], PYR["nscales"], PARAMS, PYR["nrefine"],
                        refs[k:k + 1], movs[k:k + 1], fixed_iters=1)
        assert np.array_equal(one["motion"][0], all7["motion"][k])
        assert np.array_equal(one["warp"][0], all7["warp"][k])


def test_launch_count_does_not_depend_on_batch_size(gpu):
    _, one = pyramid_case(1)
    _, all7 = pyramid_case(7)
    nscales, loops = PYR["nscales"], 6
    # max(nscales - 1, 0) downsamples + 4 per loop + nscales upsamples + 1 zeroing
    formula = max(nscales - 1, 0) + 4 * loops + nscales + 1
    assert one["info"]["launches"] == all7["info"]["launches"] == formula
    assert one["info"]["loops"] == all7["info"]["loops"] == loops
    assert all7["info"]["placement"] == [0, 0, 0]
    assert all7["info"]["threads"] == [THREADS] * 3


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
CONV_DIMS = (32, 16)
CONV_PARAMS = [0.02, 100.0]
CONV_INPUTS = [(42, (2.0, 1.3)), (49, (1.1, -0.6)), (60, (0.3, 0.2)), (75, (0.7, 0.9))]
CONV_COUNTS = [94, 123, 88, 91]


def test_convergence_per_pair(gpu, oracle):
    """Each pair stops on its own iteration: the oracle's and the one-pair
    path's (``curvature_dct=1, logger_fp64=1``).

    The inputs were chosen on the CPU with the oracle (seeds 40 to 79 of
    texture_pair(32, sigma=2.5, ny=16) at alpha 0.02, tau 100 and a cap of 200)
    so that the oracle's error keeps at least 1e-5 from 0.001 at the breaking
    iteration and at the one before it; an equal count is therefore not luck
    (the fp64 sums and the oracle's float sum differ in an error's last bits,
    about 1e-10 here).  Recorded, error - 0.001 before / at the break:
      seed 42, shift (2.0, 1.3):  94 iterations, +2.00e-5 / -1.10e-5
      seed 49, shift (1.1, -0.6): 123 iterations, +1.36e-5 / -1.66e-5
      seed 60, shift (0.3, 0.2):  88 iterations, +1.99e-5 / -1.09e-5
      seed 75, shift (0.7, 0.9):  91 iterations, +1.49e-5 / -1.52e-5
    The test asserts the margins again on the oracle's own errors."""
    pairs = [S.texture_pair(CONV_DIMS[0], seed=s, sigma=2.5, shift=sh, ny=CONV_DIMS[1])
             for s, sh in CONV_INPUTS]
    refs, movs = np.stack([r for r, _ in pairs]), np.stack([m for _, m in pairs])
    B = len(movs)
    got = run_batch(CONV_DIMS, [200], 0, CONV_PARAMS, 1, refs, movs)
    assert got["status"].tolist() == [0] * B
    assert len(set(CONV_COUNTS)) == B
    for k in range(B):
        o = oracle_pair(oracle, CONV_DIMS, [200], 0, CONV_PARAMS, 1, refs[k], movs[k], fixed=False)
        n = CONV_COUNTS[k]
        assert o["iters"] == [n]
        e = o["errs"].astype(np.float64)
        assert e[n - 2] - 0.001 >= 1e-5 and 0.001 - e[n - 1] >= 1e-5
        one = one_pair(CONV_DIMS, [200], 0, CONV_PARAMS, 1, refs[k], movs[k], logger_fp64=1)
        assert one["iters"] == [n]
        assert got["iters"][k].tolist() == [n], f"pair {k}"
        assert np.array_equal(got["motion"][k], one["motion"]), f"pair {k}"
        assert np.abs(got["motion"][k] - o["motion"]).max() <= TOL
        # the bar tests/test_gpu_batch.py applies to Diffusion's errors: one float32 ulp
        eb, e1 = got["errs"][k], np.asarray(one["errs"], np.float32)
        assert eb.shape == e1.shape == (n,)
        assert np.all(np.abs(eb.astype(np.float64) - e1.astype(np.float64))
                      <= np.spacing(e1).astype(np.float64)), f"pair {k}"
    # two calls give the same bits
    again = run_batch(CONV_DIMS, [200], 0, CONV_PARAMS, 1, refs, movs)
    assert np.array_equal(again["motion"], got["motion"])
    assert all(np.array_equal(a, b) for a, b in zip(again["errs"], got["errs"]))


# ------------------------------------------------------------ warm start, device I/O
def test_warm_start_is_a_reused_one_pair_object(gpu):
    from opticalflow2d_amd import BatchRegistration, ImageRegistration
    dims, niter, nscales = (32, 16), [4, 5], 1
    refs, movs = make_pairs(dims, 3)
    with BatchRegistration(3, dims, niter, nscales, PARAMS, reg=1, device=0, fixed_iters=1,
                           warm_start=1) as b:
        b.register(refs, movs)
        first = b.motion()
        b.register(refs, movs)
        second = b.motion()
    assert not np.array_equal(first, second)
    for k in range(3):
        with ImageRegistration(dims, niter, nscales, 1, PARAMS, curvature_dct=1, fixed_iters=1,
                               device=0) as r:
            r.register(refs[k], movs[k])
            assert np.array_equal(first[k], r.motion())
            r.register(refs[k], movs[k])
            assert np.array_equal(second[k], r.motion()), f"pair {k}"


def test_device_io(gpu):
    import torch
    from opticalflow2d_amd import BatchRegistration
    dims, niter = (32, 16), [4]
    refs, movs = make_pairs(dims, 3)
    host = run_batch(dims, niter, 0, PARAMS, 1, refs, movs, fixed_iters=1)
    with BatchRegistration(3, dims, niter, 0, PARAMS, reg=1, device=0, fixed_iters=1) as b:
        b.register(torch.as_tensor(refs, device="cuda:0"), torch.as_tensor(movs, device="cuda:0"))
        torch.cuda.synchronize()
        assert np.array_equal(b.motion(), host["motion"])
        md = b.motion_device()
        assert md.is_cuda
        assert np.array_equal(md.cpu().numpy().astype(np.float64), host["motion"])
        jac = b.jacobian()
    assert jac is not None
