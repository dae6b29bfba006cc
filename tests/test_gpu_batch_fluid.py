"""Batched Fluid on the device (BatchRegistration(reg=5): the option "fluid" of
an Elastic batch): every pair of a batch bit for bit the
one-pair Fluid registration and the oracle, motion, warp, iteration counts and
the reference's Dumax / Regridding lines, at the sizes where the in-workgroup
loop can go wrong; regrids inside the kernel, one in a loop's last iteration,
skipped time steps, per-pair convergence, the velocity across refines and
register calls, pairs independent of each other, and what surrounds the loop.
Every comparison is np.array_equal or string equality, except the errors (one
float32 ulp, the bar of the other batched methods)."""
import numpy as np
import pytest

from opticalflow2d_amd import synthetic as S
from test_gpu_batch import make_pairs, ref_of
from test_gpu_fluid import body

pytestmark = pytest.mark.gpu

PARAMS = [0.25, 0.0, 0.9]


def threads(dx):
    return min((dx + 63) // 64 * 64, 512)


def snapshot(b, movs):
    B = len(movs)
    return {"motion": b.motion(), "warp": b.warp(movs), "iters": b.iterations(),
            "status": b.status(), "info": b.info(), "error": b.last_error(),
            "errs": [b.last_errors(k) for k in range(B)],
            "log": [b.fluid_log(k) for k in range(B)],
            "lines": [b.fluid_lines(k) for k in range(B)]}


def run_batch(dims, niter, nscales, params, nrefine, refs, movs, calls=1, **opt):
    from opticalflow2d_amd import BatchRegistration
    with BatchRegistration(len(movs), dims, niter, nscales, params, nrefine, reg=5, device=0,
                           **opt) as b:
        outs = []
        for _ in range(calls):
            b.register(refs, movs)
            outs.append(snapshot(b, movs))
    return outs[0] if calls == 1 else outs


def one_pair(gpu, dims, niter, nscales, params, nrefine, ref, mov, calls=1, **opt):
    """The one-pair path; its printed lines come through the print sink."""
    from opticalflow2d_amd import ImageRegistration
    outs = []
    with ImageRegistration(dims, niter, nscales, 5, params, nrefine, device=0, **opt) as r:
        for _ in range(calls):
            gpu.clear()
            r.register(ref, mov)
            outs.append({"motion": r.motion(), "warp": r.warp(mov), "iters": r.iterations(),
                         "errs": np.asarray(r.last_errors(), np.float32),
                         "lines": body("".join(gpu))})
    return outs[0] if calls == 1 else outs


def oracle_pair(O, dims, niter, nscales, params, nrefine, ref, mov, fixed=True, calls=1):
    L = O.lib()
    outs = []
    o = O.Registration(dims, niter, nscales, 5, params, nrefine, 0, fixed_iters=fixed)
    for _ in range(calls):
        L.oracle_clear_output()
        o.register(ref, mov)
        outs.append({"motion": o.motion(), "warp": o.warp(mov), "iters": o.iterations(),
                     "errs": np.asarray(o.last_errors()),
                     "lines": body(L.oracle_captured_output().decode())})
    o.close()
    return outs[0] if calls == 1 else outs


def same(got, k, want, what):
    assert got["iters"][k].tolist() == want["iters"], f"pair {k}: {what} iterations"
    assert np.array_equal(got["motion"][k], want["motion"]), f"pair {k}: {what} motion"
    assert np.array_equal(got["warp"][k], want["warp"]), f"pair {k}: {what} warp"
    assert got["lines"][k] == want["lines"], f"pair {k}: {what} lines"


def check(gpu, oracle, dims, niter, nscales, params, nrefine, refs, movs, got, one_params=None,
          pairs=None):
    """got, a fixed_iters batch: every pair (or `pairs`) against the one-pair
    path and the oracle.  Returns the oracle's results."""
    B = len(movs)
    one_params = params if one_params is None else one_params
    want = [n for n in reversed(niter[: nscales + 1]) for _ in range(nrefine)]
    assert got["status"].tolist() == [0] * B and got["error"] == ""
    assert got["info"]["placement"] == [0] * (nscales + 1)
    assert got["info"]["threads"] == [threads(int(np.float32(dims[0]) / np.float32(2 ** s)))
                                      for s in range(nscales + 1)]
    assert got["iters"].tolist() == [want] * B
    oracles = {}
    for k in (range(B) if pairs is None else pairs):
        assert got["errs"][k].size == 0  # fixed_iters: no errors recorded
        assert [len(a) for a in got["log"][k]] == want
        one = one_pair(gpu, dims, niter, nscales, one_params, nrefine, ref_of(refs, k), movs[k],
                       fixed_iters=1)
        same(got, k, one, "one-pair")
        o = oracle_pair(oracle, dims, niter, nscales, one_params, nrefine, ref_of(refs, k),
                        movs[k])
        same(got, k, o, "oracle")
        oracles[k] = o
    return oracles


def regrids(lines):
    """The iterations of the 'Regridding on iteration: %d' lines."""
    return [int(l.split(":")[1].split("\t")[0]) for l in lines if l.startswith("Regridding")]


def disk(dims, shift=(9, 5)):
    ref, mov = S.shifted_disk(max(dims), shift=shift)
    return ref[: dims[0], : dims[1]], mov[: dims[0], : dims[1]]


def disk_pairs(dims, shifts):
    pairs = [disk(dims, sh) for sh in shifts]
    return np.stack([r for r, _ in pairs]), np.stack([m for _, m in pairs])


# ------------------------------------------------------------ fixed iterations
FIXED_CASES = [
    # dims, B, niter, shared reference
    ((3, 3), 2, [5], False),       # one interior pixel
    ((5, 4), 3, [5], False),
    ((63, 9), 2, [4], False),      # the one-pair strip's width
    ((64, 9), 2, [4], True),       # one wave, no barrier
    ((65, 9), 2, [4], False),      # two waves
    ((130, 20), 2, [4], False),    # three waves, barriers
    ((9, 200), 2, [6], False),     # tall: the wavefront longer than wide
    ((1024, 16), 2, [4], False),   # more columns than threads
    ((512, 512), 2, [2], False),   # the largest
]


@pytest.mark.parametrize("dims, B, niter, shared", FIXED_CASES)
def test_fixed_iterations_bit_for_bit(gpu, oracle, dims, B, niter, shared):
    refs, movs = make_pairs(dims, B, shared)
    got = run_batch(dims, niter, 0, PARAMS, 1, refs, movs, fixed_iters=1)
    assert got["motion"].any()
    check(gpu, oracle, dims, niter, 0, PARAMS, 1, refs, movs, got)


@pytest.mark.parametrize("dims", [(2, 7), (7, 2)])
def test_no_interior(gpu, oracle, dims):
    """A side below 3: no pixel is relaxed, the velocity stays 0, maxabs is 0,
    dt = inf and every step is skipped; the motion is +0 on the bits."""
    refs, movs = make_pairs(dims, 2)
    got = run_batch(dims, [4], 0, PARAMS, 1, refs, movs, fixed_iters=1)
    assert got["motion"].tobytes() == np.zeros_like(got["motion"]).tobytes()
    for k in range(2):
        assert got["lines"][k] == ["Dumax: 0.650\tMaxabs increment: 0.000\t Timestep: inf"] * 4
        assert np.array_equal(got["log"][k][0],
                              np.array([[0.0, np.inf, 1.0, 0.0]] * 4, np.float32))
    check(gpu, oracle, dims, [4], 0, PARAMS, 1, refs, movs, got)


# ------------------------------------------------------------ regrids
@pytest.mark.parametrize("dims", [(64, 40), (63, 40), (65, 40), (96, 96)])
def test_regrids_inside_the_kernel(gpu, oracle, dims):
    """The disk shifted by (9, 5): the Jacobian falls below 0.5 every few
    iterations.  Pair 0 is that disk, pair 1 a disk shifted otherwise, so the
    two regrid on different iterations of one launch.  At (64, 40) the oracle
    regrids at iterations 2, 6, 10, 15, 19, 24, 28, 34, 36 and 39, the last
    one of the loop."""
    refs, movs = disk_pairs(dims, [(9, 5), (6, -7)])
    got = run_batch(dims, [40], 0, PARAMS, 1, refs, movs, fixed_iters=1)
    o = check(gpu, oracle, dims, [40], 0, PARAMS, 1, refs, movs, got)
    assert len(regrids(o[0]["lines"])) >= 1 and len(regrids(o[1]["lines"])) >= 1
    assert regrids(o[0]["lines"]) != regrids(o[1]["lines"])
    if dims == (64, 40):
        assert regrids(o[0]["lines"]) == [2, 6, 10, 15, 19, 24, 28, 34, 36, 39]
    # the record's flags are the lines' iterations
    for k in range(2):
        assert np.flatnonzero(got["log"][k][0][:, 3]).tolist() == regrids(o[k]["lines"])
        assert (got["log"][k][0][got["log"][k][0][:, 3] != 0, 2] < 0.5).all()


@pytest.mark.parametrize("niter", [[10], [11]])
def test_regrid_in_the_last_iteration(gpu, oracle, niter):
    """The (64, 40) disk regrids at iteration 10: with 11 iterations that is the
    loop's last one, the motion has accumulated the estimate and the final
    estimate is zero; with 10 the loop ends one iteration before it."""
    dims = (64, 40)
    refs, movs = disk_pairs(dims, [(9, 5), (9, 5), (6, -7)])
    got = run_batch(dims, niter, 0, PARAMS, 1, refs, movs, fixed_iters=1)
    o = check(gpu, oracle, dims, niter, 0, PARAMS, 1, refs, movs, got, pairs=(0, 2))
    last = o[0]["lines"][-1]
    if niter == [11]:
        assert last.startswith("Regridding on iteration: 10")
    else:
        assert last.startswith("Dumax") and regrids(o[0]["lines"]) == [2, 6]
    assert np.array_equal(got["motion"][0], got["motion"][1])


def test_timestep_skip_and_integrate(gpu, oracle):
    """tests/test_gpu_fluid.py's faint input: dt >= 65 in some iterations (the
    integration is skipped, OpticalFlowFluid.cpp:135-137) and below in others."""
    ref, mov = S.texture_pair(96, seed=5)
    faint = ref + 0.08 * (mov - ref)
    refs, movs = np.stack([ref, ref]), np.stack([faint, mov])
    got = run_batch((96, 96), [25], 0, [0.25, 0.0], 1, refs, movs, fixed_iters=1)
    check(gpu, oracle, (96, 96), [25], 0, [0.25, 0.0], 1, refs, movs, got)
    dts = [float(l.split("Timestep:")[1]) for l in got["lines"][0] if "Timestep:" in l]
    assert len(dts) == 25
    assert any(t >= 65.0 for t in dts) and any(t < 65.0 for t in dts), dts


# ------------------------------------------------------------ convergence
CONV_COUNTS = [3, 5, 27, 60]


def test_pairs_that_differ_within_one_batch(gpu, oracle):
    """The three inputs of test_fluid_convergence_break_on_device and the disk
    in one batch, [mu, lambda] through the class, cap 60: the oracle (fp64
    Logger sums) and the one-pair path (logger_fp64=1) stop at 3, 5 and 27
    iterations, and the disk runs all 60.

    The oracle's errors, on the CPU: 0.0 at each break; one iteration earlier
    0.226 ('mid') and 1.0 ('tex'); 'faint' has errors 0, 0, 0 and is held back
    by `it > 1` alone; the disk never falls below 0.47.  So an equal count does
    not hang on the last bits of the fp64 sums; the test asserts again, on the
    oracle's own errors, that every iteration after the second that did not
    break keeps 1e-5 above 0.001 and the breaking one 1e-5 below."""
    ref, mov = S.texture_pair(96, seed=5)
    dref, dmov = S.shifted_disk(96, shift=(9, 5))
    refs = np.stack([ref, ref, ref, dref])
    movs = np.stack([ref + 0.08 * (mov - ref), ref + 0.3 * (mov - ref), mov, dmov])
    dims, cap, params = (96, 96), [60], [0.25, 0.0]
    B = len(movs)
    got = run_batch(dims, cap, 0, params, 1, refs, movs)
    assert got["status"].tolist() == [0] * B
    oracle.lib().oracle_set_logger_fp64(1)
    try:
        oracles = [oracle_pair(oracle, dims, cap, 0, params, 1, refs[k], movs[k], fixed=False)
                   for k in range(B)]
    finally:
        oracle.lib().oracle_set_logger_fp64(0)
    for k in range(B):
        o, n = oracles[k], CONV_COUNTS[k]
        assert o["iters"] == [n]
        e = o["errs"].astype(np.float64)
        assert e.shape == (n,)
        assert (e[2:n - 1] - 0.001 >= 1e-5).all()
        if n < cap[0]:
            assert 0.001 - e[n - 1] >= 1e-5
        else:
            assert e[n - 1] - 0.001 >= 1e-5
        one = one_pair(gpu, dims, cap, 0, params, 1, refs[k], movs[k], logger_fp64=1)
        assert one["iters"] == [n]
        same(got, k, one, "one-pair")
        same(got, k, o, "oracle")
        eb, e1 = got["errs"][k], one["errs"]
        assert eb.shape == e1.shape == (n,)
        assert np.all(np.abs(eb.astype(np.float64) - e1.astype(np.float64))
                      <= np.spacing(e1).astype(np.float64)), f"pair {k}"
    assert got["iters"][:, 0].tolist() == CONV_COUNTS
    # two calls give the same bits
    again = run_batch(dims, cap, 0, params, 1, refs, movs)
    assert np.array_equal(again["motion"], got["motion"])
    assert again["lines"] == got["lines"]
    assert all(np.array_equal(a, b) for a, b in zip(again["errs"], got["errs"]))


# ------------------------------------------------------------ pyramid, warm start
def test_pyramid_and_refines(gpu, oracle):
    """Two levels, two refines: the velocity carries across the refines of a
    level, and both levels regrid."""
    dims, niter = (96, 96), [60, 40]
    refs, movs = disk_pairs(dims, [(9, 5), (6, -7)])
    got = run_batch(dims, niter, 1, PARAMS, 2, refs, movs, fixed_iters=1)
    check(gpu, oracle, dims, niter, 1, PARAMS, 2, refs, movs, got)
    for k in range(2):
        per_loop = [int(a[:, 3].sum()) for a in got["log"][k]]
        assert len(per_loop) == 4 and all(n >= 1 for n in per_loop), per_loop


def test_warm_start_keeps_the_velocity(gpu):
    from opticalflow2d_amd import BatchRegistration
    dims, niter = (64, 40), [12]
    refs, movs = disk_pairs(dims, [(9, 5), (6, -7), (3, 2)])
    first, second = run_batch(dims, niter, 0, PARAMS, 1, refs, movs, calls=2, fixed_iters=1,
                              warm_start=1)
    assert not np.array_equal(first["motion"], second["motion"])
    for k in range(3):
        one = one_pair(gpu, dims, niter, 0, PARAMS, 1, refs[k], movs[k], calls=2, fixed_iters=1)
        same(first, k, one[0], "first call")
        same(second, k, one[1], "second call")
    # warm_start 0: the velocity is zeroed, the second call is the first
    a, b = run_batch(dims, niter, 0, PARAMS, 1, refs, movs, calls=2, fixed_iters=1)
    assert np.array_equal(a["motion"], first["motion"]) and a["lines"] == first["lines"]
    assert np.array_equal(b["motion"], a["motion"]) and b["lines"] == a["lines"]
    # reset_motion: a fresh handle's bits, the velocity included
    with BatchRegistration(3, dims, niter, 0, PARAMS, reg=5, device=0, fixed_iters=1,
                           warm_start=1) as h:
        h.register(refs, movs)
        h.reset_motion()
        assert h.motion().tobytes() == np.zeros_like(first["motion"]).tobytes()
        h.register(refs, movs)
        assert np.array_equal(h.motion(), first["motion"])
        assert [h.fluid_lines(k) for k in range(3)] == first["lines"]
        # set_motion leaves the velocity alone, as of2d_set_motion: the second
        # call's start state again
        h.set_motion(first["motion"])
        h.register(refs, movs)
        assert np.array_equal(h.motion(), second["motion"])


# ------------------------------------------------------------ independence, scale
def test_pairs_do_not_see_each_other(gpu):
    dims, niter = (64, 40), [14]
    refs, movs = disk_pairs(dims, [(9, 5), (6, -7), (3, 2), (9, 5)])
    all4 = run_batch(dims, niter, 0, PARAMS, 1, refs, movs, fixed_iters=1)
    assert sum(len(regrids(l)) for l in all4["lines"]) >= 2
    for k in (0, 2):
        one = run_batch(dims, niter, 0, PARAMS, 1, refs[k:k + 1], movs[k:k + 1], fixed_iters=1)
        assert np.array_equal(one["motion"][0], all4["motion"][k])
        assert np.array_equal(one["warp"][0], all4["warp"][k])
        assert one["lines"][0] == all4["lines"][k]
        assert one["info"]["launches"] == all4["info"]["launches"]
    assert np.array_equal(all4["motion"][0], all4["motion"][3])


def test_launch_count_does_not_depend_on_batch_size(gpu):
    dims, niter = (16, 12), [3]
    refs, movs = make_pairs(dims, 64, shared=True)
    one = run_batch(dims, niter, 0, PARAMS, 1, refs, movs[:1], fixed_iters=1)
    many = run_batch(dims, niter, 0, PARAMS, 1, refs, movs, fixed_iters=1)
    # what an Elastic batch reports: 4 per loop + 1 zeroing of failed pairs
    assert one["info"]["launches"] == many["info"]["launches"] == 4 + 1
    assert many["info"]["threads"] == [64] and many["info"]["placement"] == [0]
    assert np.array_equal(one["motion"][0], many["motion"][0])


def test_more_pairs_than_block_slots(gpu):
    """1100 workgroups: more than the device holds at a time."""
    dims, niter, B = (16, 12), [3], 1100
    both = [S.texture_pair(16, seed=7, sigma=1.5, shift=sh, ny=12)
            for sh in [(0.5, 0.25), (-0.75, 0.5), (1.25, -1.0), (0.1, 0.9)]]
    ref, four = both[0][0], [m for _, m in both]
    which = (np.arange(B) * 7 + np.arange(B) // 256) % 4
    movs = np.stack([four[w] for w in which])
    from opticalflow2d_amd import BatchRegistration
    with BatchRegistration(B, dims, niter, 0, PARAMS, reg=5, device=0, fixed_iters=1) as b:
        b.register(ref, movs)
        motion, warp, iters = b.motion(), b.warp(movs), b.iterations()
        lines = {k: b.fluid_lines(k) for k in (0, B // 2, B - 1)}
        assert not b.status().any()
    assert iters.tolist() == [[3]] * B
    for k in (0, B // 2, B - 1):
        one = run_batch(dims, niter, 0, PARAMS, 1, ref, movs[k:k + 1], fixed_iters=1)
        assert one["motion"].any()
        assert np.array_equal(motion[k], one["motion"][0])
        assert np.array_equal(warp[k], one["warp"][0])
        assert lines[k] == one["lines"][0]
    for w in range(4):
        sel = which == w
        assert np.array_equal(motion[sel], np.broadcast_to(motion[sel][0], motion[sel].shape))


# ------------------------------------------------------------ surroundings
def test_fluid_0_afterwards_is_the_elastic_batch(gpu):
    from opticalflow2d_amd import BatchRegistration
    dims, niter = (37, 29), [5]
    refs, movs = make_pairs(dims, 3)
    with BatchRegistration(3, dims, niter, 0, PARAMS, reg=2, device=0, fixed_iters=1) as e:
        e.register(refs, movs)
        elastic = e.motion()
        assert all(a.shape == (0, 4) for a in e.fluid_log(0))
    with BatchRegistration(3, dims, niter, 0, PARAMS, reg=5, device=0, fixed_iters=1) as b:
        b.register(refs, movs)
        fluid = b.motion()
        assert len(b.fluid_lines(0)) >= 5
        b.set_option("fluid", 0)
        assert b.fluid_lines(0) == []
        b.register(refs, movs)
        assert np.array_equal(b.motion(), elastic)
        assert b.fluid_lines(0) == []
        # and back: the velocity was zeroed by the change, a fresh handle's bits
        b.set_option("fluid", 1)
        b.register(refs, movs)
        assert np.array_equal(b.motion(), fluid)
    assert not np.array_equal(fluid, elastic)


def test_device_io(gpu):
    import torch
    from opticalflow2d_amd import BatchRegistration
    dims, niter = (37, 29), [6]
    refs, movs = make_pairs(dims, 3)
    host = run_batch(dims, niter, 0, PARAMS, 1, refs, movs, fixed_iters=1)
    with BatchRegistration(3, dims, niter, 0, PARAMS, reg=5, device=0, fixed_iters=1) as b:
        b.register(torch.as_tensor(refs, device="cuda:0"), torch.as_tensor(movs, device="cuda:0"))
        torch.cuda.synchronize()
        assert np.array_equal(b.motion(), host["motion"])
        assert [b.fluid_lines(k) for k in range(3)] == host["lines"]
        md = b.motion_device()
        assert np.array_equal(md.cpu().numpy().astype(np.float64), host["motion"])
        wd = b.warp(torch.as_tensor(movs, device="cuda:0"))
        assert np.array_equal(wd.cpu().numpy(), host["warp"])


def test_jacobian_agrees_with_the_one_pair_entry(gpu):
    from opticalflow2d_amd import BatchRegistration, ImageRegistration
    dims, niter = (64, 40), [12]
    refs, movs = disk_pairs(dims, [(9, 5), (6, -7)])
    with BatchRegistration(2, dims, niter, 0, PARAMS, reg=5, device=0, fixed_iters=1) as b:
        b.register(refs, movs)
        m0 = b.motion()
        jac, st = b.jacobian()
        assert np.array_equal(b.motion(), m0)
    k = 1
    with ImageRegistration(dims, niter, 0, 5, PARAMS, 1, fixed_iters=1, device=0) as r:
        r.register(refs[k], movs[k])
        wjac, wst = r.jacobian()
    assert np.array_equal(np.asarray(jac[k], np.float64).view(np.uint64), wjac.view(np.uint64))
    for key in ("min", "max", "folded", "below_half"):
        assert st[k][key] == wst[key], key
