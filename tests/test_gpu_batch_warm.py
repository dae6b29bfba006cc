"""The batch's warm start and motion input on the device (BatchRegistration
warm_start=1, set_motion, reset_motion) against the oracle:
a reused oracle object per pair, bit for bit after every call; the default
untouched; a supplied motion through the host form and every access pattern of
the pack kernels; the analysis of a supplied field; pairs independent of each
other; a failed pair under warm start; the launch count; more pairs than block
slots.  The pyramid's yardstick, ``estimate_from``, is held to the oracle in
tests/test_warm_reference.py."""
import numpy as np
import pytest

from test_warm_reference import (ALPHA, downsample_motion, estimate_from, f32, field_of,
                                 level_dims, motion_of, warm_pairs, zero_levels)

pytestmark = pytest.mark.gpu

SHAPES = [(40, 24), (19, 13)]  # the second: odd, below every tile and wave width
DEMONS = [1.0, 2.0, 1.0, 1.0, 5]
# name -> (batch reg, batch parameters, batch options, one-pair reg, one-pair parameters)
METHODS = {
    "diffusion": (0, [ALPHA], {}, 0, [ALPHA]),
    "thirion": (3, DEMONS + [0], {}, 3, DEMONS + [0]),
    "thirion_addition": (3, DEMONS + [1], {}, 3, DEMONS + [1]),
    "diffeomorphic": (3, DEMONS + [0], {"diffeomorphic": 1}, 4, DEMONS),
    # sigma_x = sigma_i and a wider diffusion kernel: the loops of the series
    # below converge (with DEMONS most oscillate past 200 iterations)
    "thirion_conv": (3, [1.0, 1.0, 2.5, 1.0, 5, 0], {}, 3, [1.0, 1.0, 2.5, 1.0, 5, 0]),
}


def batch_of(B, dims, niter, nscales, method, nrefine=1, **opt):
    from opticalflow2d_amd import BatchRegistration
    reg, p, mopt, _, _ = METHODS[method]
    opt.setdefault("fixed_iters", 1)
    return BatchRegistration(B, dims, niter, nscales, p, nrefine, reg=reg, device=0,
                             **mopt, **opt)


def oracle_of(O, dims, niter, nscales, method, nrefine=1, fixed=True):
    _, _, _, reg, p = METHODS[method]
    return O.Registration(dims, niter, nscales, reg, p, nrefine, fixed_iters=fixed)


def launches_formula(nscales, nrefine, demons, warm):
    """per loop warp, (gradients,) loop and accumulate; a
    motion downsample per level strictly between the coarsest and level 0, an
    upsample per level above 0; the zeroing of failed pairs, once, or with
    warm_start once per level."""
    return ((3 if demons else 4) * (nscales + 1) * nrefine + max(nscales - 1, 0) + nscales +
            (nscales + 1 if warm else 1))


# ------------------------------------------------------------ 1. reused object
REUSED = [("diffusion", [6], 0, 1), ("diffusion", [4, 5, 6], 2, 2), ("thirion", [5, 6], 1, 1),
          ("thirion_addition", [5, 6], 1, 1), ("diffeomorphic", [5, 6], 1, 1)]


@pytest.mark.parametrize("dims", SHAPES)
@pytest.mark.parametrize("method, niter, nscales, nrefine", REUSED)
def test_reused_object_bit_for_bit(gpu, oracle, dims, method, niter, nscales, nrefine):
    refs, movs = warm_pairs(dims)
    B = len(refs)
    objs = [oracle_of(oracle, dims, niter, nscales, method, nrefine) for _ in range(B)]
    cold_last = oracle_of(oracle, dims, niter, nscales, method, nrefine)
    cold_last.register(refs[0], movs[2][0])
    want_iters = [n for n in reversed(niter) for _ in range(nrefine)]
    with batch_of(B, dims, niter, nscales, method, nrefine, warm_start=1) as b:
        for call in range(3):
            b.register(refs, movs[call])
            got_m, got_w = b.motion(), b.warp(movs[call])
            assert b.status().tolist() == [0] * B
            assert b.iterations().tolist() == [want_iters] * B
            for k, o in enumerate(objs):
                o.register(refs[k], movs[call][k])
                assert o.motion().any()
                assert np.array_equal(got_m[k], o.motion()), f"call {call}, pair {k}: motion"
                assert np.array_equal(got_w[k], o.warp(movs[call][k])), f"call {call}, pair {k}"
        # the warm start is live: a fresh object gives other bits on the last call
        assert not np.array_equal(got_m[0], cold_last.motion())
    for o in objs + [cold_last]:
        o.close()


CONV_NITER = [200]
# relative distance of every oracle error from the 0.001 threshold that the
# test demands: the batch's and the oracle's fp64 sums of at most 960 terms
# differ by 960 * 2^-53 relative at most, and the float sqrt and division that
# follow by a few float ulps (6e-8 each); 1e-4 is three orders above both
CONV_MARGIN = 1e-4


# (method, dims) -> the series' blur and step per call, chosen on the CPU from
# the oracle alone so that the conditions of the test below hold
CONV_SERIES = {("diffusion", (40, 24)): (2.0, 0.8), ("diffusion", (19, 13)): (2.0, 1.2),
               ("thirion_conv", (40, 24)): (2.0, 0.5), ("thirion_conv", (19, 13)): (2.0, 0.5)}


def conv_expectations(O, method, dims):
    """On the CPU: three reused oracle objects with the Logger's sums in fp64,
    three calls; per call the pairs' counts, motions and the smallest relative
    distance of an error from the threshold."""
    sigma, step = CONV_SERIES[method, dims]
    refs, movs = warm_pairs(dims, sigma=sigma, step=step)
    B = len(refs)
    O.lib().oracle_set_logger_fp64(1)
    try:
        objs = [oracle_of(O, dims, CONV_NITER, 0, method, fixed=False) for _ in range(B)]
        calls = []
        for call in range(3):
            counts, motions, dist = [], [], np.inf
            for k, o in enumerate(objs):
                o.register(refs[k], movs[call][k])
                counts.append(o.iterations())
                motions.append(o.motion())
                e = o.last_errors().astype(np.float64)
                assert e.size == counts[-1][0]
                dist = min(dist, float(np.min(np.abs(e[2:] - 0.001)) / 0.001))
            calls.append((counts, motions, dist))
        for o in objs:
            o.close()
    finally:
        O.lib().oracle_set_logger_fp64(0)
    return refs, movs, calls


@pytest.mark.parametrize("dims", SHAPES)
@pytest.mark.parametrize("method", ["diffusion", "thirion_conv"])
def test_reused_object_convergence_counts(gpu, oracle, dims, method):
    """Convergence on: every pair of every call stops on the iteration of its
    reused oracle object (fp64 Logger sums).  Established on the CPU first: no
    error lies within CONV_MARGIN of the threshold, every loop of the first
    two calls breaks before niter, and the second call's counts differ between
    the pairs and from the first call's: the warm start is live in the counts."""
    refs, movs, calls = conv_expectations(oracle, method, dims)
    B = len(refs)
    for call, (counts, _, dist) in enumerate(calls):
        assert dist > CONV_MARGIN, dist
        if call < 2:
            assert all(2 < c[0] < CONV_NITER[0] for c in counts), counts
    second = [c[0] for c in calls[1][0]]
    first = [c[0] for c in calls[0][0]]
    assert len(set(second)) == B, second
    assert all(a != b for a, b in zip(first, second)), (first, second)
    with batch_of(B, dims, CONV_NITER, 0, method, warm_start=1, fixed_iters=0) as b:
        for call, (counts, motions, _) in enumerate(calls):
            b.register(refs, movs[call])
            assert b.status().tolist() == [0] * B
            assert b.iterations().tolist() == counts, f"call {call}"
            got = b.motion()
            for k in range(B):
                assert np.array_equal(got[k], motions[k]), f"call {call}, pair {k}"


# ------------------------------------------------------------ 2. default untouched
@pytest.mark.parametrize("method, niter, nscales", [("diffusion", [4, 5, 6], 2),
                                                    ("thirion", [5, 6], 1)])
def test_default_is_the_cold_estimate(gpu, method, niter, nscales):
    dims = SHAPES[0]
    refs, movs = warm_pairs(dims)
    B = len(refs)
    junk = np.random.default_rng(3).standard_normal((B,) + dims + (2,))
    with batch_of(B, dims, niter, nscales, method) as fresh:
        fresh.register(refs, movs[1])
        cold, cold_launches = fresh.motion(), fresh.info()["launches"]
    assert cold_launches == launches_formula(nscales, 1, method != "diffusion", warm=False)
    with batch_of(B, dims, niter, nscales, method, warm_start=0) as b:
        b.register(refs, movs[0])
        b.register(refs, movs[1])
        assert np.array_equal(b.motion(), cold)
        assert b.info()["launches"] == cold_launches
        b.set_motion(junk)
        assert np.array_equal(b.motion(), f32(junk).astype(np.float64))
        b.register(refs, movs[1])  # the supplied motion is ignored
        assert np.array_equal(b.motion(), cold)
        # warm, then back to the default
        b.set_option("warm_start", 1)
        b.register(refs, movs[2])
        b.register(refs, movs[1])
        assert not np.array_equal(b.motion(), cold)
        b.set_option("warm_start", 0)
        b.register(refs, movs[1])
        assert np.array_equal(b.motion(), cold)


# ------------------------------------------------------------ device forms
def device_forms(m):
    """``m`` ([B, dimx, dimy, 2], float32 values) as CUDA tensors of that shape:
    every access pattern and instantiation of the pack kernels.  A contiguous
    tensor has y faster than x (the transposing tile); a permuted [B, dimy,
    dimx, 2] has x faster (rows)."""
    import torch
    B, dx, dy, _ = m.shape
    m32 = np.ascontiguousarray(m, np.float32)
    out = {}
    for name, a in (("f32", m32), ("f64", m32.astype(np.float64))):
        t = torch.from_numpy(a).to("cuda")
        out[f"{name}_contiguous_tile_vec2"] = t
        rows = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 1, 3))).to("cuda")
        out[f"{name}_permuted_rows_vec2"] = rows.permute(0, 2, 1, 3)
        # a slice of a larger tensor: not contiguous, even strides and offset
        big = torch.zeros((B, dx + 3, dy + 2, 2), dtype=t.dtype, device="cuda")
        big[:, 1:1 + dx, 2:, :] = t
        out[f"{name}_slice_tile_vec2"] = big[:, 1:1 + dx, 2:, :]
        # planar: the component stride is not 1
        planar = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 2, 1))).to("cuda")
        out[f"{name}_planar_rows"] = planar.permute(0, 3, 2, 1)
        planar_t = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2))).to("cuda")
        out[f"{name}_planar_tile"] = planar_t.permute(0, 2, 3, 1)
        # the base one element off the pair's alignment, component stride 1
        flat = torch.zeros(a.size + 1, dtype=t.dtype, device="cuda")
        flat[1:] = t.reshape(-1)
        out[f"{name}_offset_tile"] = flat[1:].view(B, dx, dy, 2)
        flat_r = torch.zeros(a.size + 1, dtype=t.dtype, device="cuda")
        flat_r[1:] = rows.reshape(-1)
        out[f"{name}_offset_rows"] = flat_r[1:].view(B, dy, dx, 2).permute(0, 2, 1, 3)
    for name, t in out.items():
        assert tuple(t.shape) == m.shape, name
        assert np.array_equal(t.cpu().numpy().astype(np.float32), m32), name
    assert out["f32_offset_tile"].data_ptr() % 8 == 4
    assert out["f64_offset_rows"].data_ptr() % 16 == 8
    assert not out["f32_slice_tile_vec2"].is_contiguous()
    if dx > 1 and dy > 1:
        assert out["f32_permuted_rows_vec2"].stride(1) < out["f32_permuted_rows_vec2"].stride(2)
        assert out["f32_contiguous_tile_vec2"].stride(1) > out["f32_contiguous_tile_vec2"].stride(2)
    return out


# ------------------------------------------------------------ 3. supplied motion
def supplied_case(O, dims, method, niter):
    """Per pair: register(A) -> m_A, then register(B) -> R on one oracle object."""
    refs, movs = warm_pairs(dims)
    mA, R, W = [], [], []
    for k in range(len(refs)):
        o = oracle_of(O, dims, niter, 0, method)
        o.register(refs[k], movs[0][k])
        mA.append(o.motion())
        o.register(refs[k], movs[1][k])
        R.append(o.motion())
        W.append(o.warp(movs[1][k]))
        o.close()
    return refs, movs, np.stack(mA), np.stack(R), np.stack(W)


@pytest.mark.parametrize("dims", SHAPES)
@pytest.mark.parametrize("method", ["diffusion", "thirion", "diffeomorphic"])
def test_supplied_motion_host_and_device_forms(gpu, oracle, dims, method):
    niter = [6]
    refs, movs, mA, R, W = supplied_case(oracle, dims, method, niter)
    B = len(refs)
    assert mA.any() and not np.array_equal(mA, R)
    forms = {"host": mA}
    forms.update(device_forms(mA))
    with batch_of(B, dims, niter, 0, method, warm_start=1) as b:
        for name, m in forms.items():
            b.set_motion(m)
            b.register(refs, movs[1])
            assert np.array_equal(b.motion(), R), name
            assert np.array_equal(b.warp(movs[1]), W), name
            assert b.status().tolist() == [0] * B


# ------------------------------------------------------------ 4. supplied motion, pyramid
def test_supplied_motion_pyramid(gpu, oracle):
    """nscales 2, Diffusion: the estimate starts from {m, downSample(m)}; and
    the recipe that continues a pyramid from its own full-resolution result,
    ``b.set_motion(b.motion_device())``."""
    niter, nscales, nrefine = [4, 5, 6], 2, 2
    for dims in SHAPES:
        refs, movs, mA, _, _ = supplied_case(oracle, dims, "diffusion", [6])
        B = len(refs)
        ldim = level_dims(dims, nscales)

        def start_from(m):
            lv = zero_levels(dims, nscales)
            lv[0] = field_of(m)
            lv[nscales] = downsample_motion(oracle, lv[0], ldim[nscales])
            return lv

        want1, want2 = [], []
        for k in range(B):
            lv = estimate_from(oracle, start_from(mA[k]), refs[k], movs[1][k], niter, nscales,
                               nrefine, ALPHA)[0]
            want1.append(motion_of(lv[0]))
            lv = estimate_from(oracle, start_from(want1[k]), refs[k], movs[2][k], niter, nscales,
                               nrefine, ALPHA)[0]
            want2.append(motion_of(lv[0]))
        forms = {"host": mA}
        dev = device_forms(mA)
        forms.update({n: dev[n] for n in ("f32_contiguous_tile_vec2", "f64_planar_rows")})
        with batch_of(B, dims, niter, nscales, "diffusion", nrefine, warm_start=1) as b:
            for name, m in forms.items():
                b.set_motion(m)
                b.register(refs, movs[1])
                assert np.array_equal(b.motion(), np.stack(want1)), (dims, name)
            b.set_motion(b.motion_device())
            b.register(refs, movs[2])
            assert np.array_equal(b.motion(), np.stack(want2)), dims


# ------------------------------------------------------------ 5. round trip and use
# the last two: more than one block of the pack kernels along x, and two tiles
# on both axes
@pytest.mark.parametrize("dims", [(37, 21), (1, 9), (9, 1), (70, 67), (130, 17)])
def test_round_trip(gpu, dims):
    B = 3
    rng = np.random.default_rng(11)
    m = f32(3.0 * rng.standard_normal((B,) + dims + (2,)))
    with batch_of(B, dims, [3], 0, "diffusion") as b:
        forms = {"host": m.astype(np.float64)}
        forms.update(device_forms(m))
        for name, t in forms.items():
            b.reset_motion()
            assert not b.motion().any()
            b.set_motion(t)
            assert np.array_equal(b.motion().astype(np.float32).view(np.uint32),
                                  m.view(np.uint32)), name
            back = b.motion_device().cpu().numpy()
            assert back.dtype == np.float32
            assert np.array_equal(back.view(np.uint32), m.view(np.uint32)), name


def test_analysis_of_a_supplied_field(gpu, oracle):
    dims, B = (37, 21), 3
    dimx, dimy = dims
    rng = np.random.default_rng(12)
    m = f32(1.5 * rng.standard_normal((B,) + dims + (2,)))
    imgs = rng.random((B,) + dims)
    L = oracle.lib()
    with batch_of(B, dims, [3], 0, "diffusion") as b:
        b.set_motion(m)
        warped = b.warp(imgs)
        jac, stats = b.jacobian()
        assert b.status().tolist() == [0] * B
    for k in range(B):
        u = f32(m[k].transpose(1, 0, 2))
        I = f32(imgs[k].T)
        L.oracle_warp2d(I, u.reshape(-1), dimx, dimy)
        assert np.array_equal(warped[k], I.T.astype(np.float64)), f"pair {k}: warp"
        J = np.zeros((dimy, dimx), np.float32)
        L.oracle_jacobian(u.reshape(-1), dimx, dimy, J)
        assert np.array_equal(jac[k], J.T.astype(np.float64)), f"pair {k}: jacobian"
        assert stats[k]["min"] == float(J.min()) and stats[k]["max"] == float(J.max())


# ------------------------------------------------------------ 6. isolation
def test_supplied_fields_do_not_see_each_other(gpu, oracle):
    dims, niter = SHAPES[0], [4, 5]
    refs, movs, mA, _, _ = supplied_case(oracle, dims, "thirion", [6])
    B = len(refs)
    other = mA.copy()
    other[1] = mA[1] + 0.25
    with batch_of(B, dims, niter, 1, "thirion", warm_start=1) as b:
        b.set_motion(mA)
        b.register(refs, movs[1])
        base = b.motion()
        b.set_motion(other)
        b.register(refs, movs[1])
        got = b.motion()
    for k in (0, 2):
        assert np.array_equal(got[k], base[k]), f"pair {k}"
    assert not np.array_equal(got[1], base[1])


# ------------------------------------------------------------ 7. failure under warm start
def test_failed_pair_under_warm_start(gpu, oracle):
    from opticalflow2d_amd import _lib
    dims, niter, nscales, method, bad = SHAPES[0], [5, 6], 1, "thirion", 1
    refs, movs = warm_pairs(dims)
    B = len(refs)
    refs2, movs2 = refs.copy(), movs[1].copy()
    refs2[bad] = 0.5  # constant images: a zero denominator on every pixel
    movs2[bad] = 0.5
    calls = [(refs, movs[0]), (refs2, movs2), (refs, movs[2])]
    objs = [oracle_of(oracle, dims, niter, nscales, method) for _ in range(B)]
    with batch_of(B, dims, niter, nscales, method, warm_start=1) as b:
        for call, (r, m) in enumerate(calls):
            b.register(r, m)
            got_m, got_w = b.motion(), b.warp(m)
            failing = call == 1
            want = [_lib.OF2D_OK] * B
            if failing:
                want[bad] = _lib.OF2D_ERR_RUNTIME
            assert b.status().tolist() == want, f"call {call}"
            assert (f"pair {bad}" in b.last_error()) == failing
            assert b.info()["launches"] == launches_formula(nscales, 1, True, warm=True)
            for k in range(B):
                if k == bad and failing:
                    with pytest.raises(oracle.OracleError, match="Divide by zero exception"):
                        objs[k].register(r[k], m[k])
                    assert not got_m[k].any()
                    # its next estimate starts as a fresh object's first
                    objs[k].close()
                    objs[k] = oracle_of(oracle, dims, niter, nscales, method)
                    continue
                objs[k].register(r[k], m[k])
                assert np.array_equal(got_m[k], objs[k].motion()), f"call {call}, pair {k}"
                assert np.array_equal(got_w[k], objs[k].warp(m[k])), f"call {call}, pair {k}"
    for o in objs:
        o.close()


# ------------------------------------------------------------ 8. reset_motion
@pytest.mark.parametrize("method, niter, nscales", [("diffusion", [4, 5, 6], 2),
                                                    ("diffeomorphic", [5, 6], 1)])
def test_reset_motion_gives_a_fresh_handle(gpu, method, niter, nscales):
    dims = SHAPES[1]
    refs, movs = warm_pairs(dims)
    B = len(refs)
    with batch_of(B, dims, niter, nscales, method, warm_start=1) as fresh:
        fresh.register(refs, movs[2])
        want_m, want_w = fresh.motion(), fresh.warp(movs[2])
    with batch_of(B, dims, niter, nscales, method, warm_start=1) as b:
        b.register(refs, movs[0])
        b.register(refs, movs[1])  # an odd number of buffer swaps at level 0 or not: both occur
        b.reset_motion()
        assert not b.motion().any()
        b.register(refs, movs[2])
        assert np.array_equal(b.motion(), want_m)
        assert np.array_equal(b.warp(movs[2]), want_w)
        b.set_motion(want_m + 1.0)
        b.reset_motion()
        b.set_option("warm_start", 0)
        b.register(refs, movs[2])
        assert np.array_equal(b.motion(), want_m)


# ------------------------------------------------------------ 9. launches
@pytest.mark.parametrize("method, demons", [("diffusion", False), ("thirion", True)])
def test_launches_of_a_warm_estimate(gpu, method, demons):
    dims, niter, nscales, nrefine = SHAPES[1], [3, 3, 3], 2, 2
    cold = launches_formula(nscales, nrefine, demons, warm=False)
    warm = launches_formula(nscales, nrefine, demons, warm=True)
    assert (cold, warm) == ((22, 24) if demons else (28, 30))
    seen = []
    for B in (2, 40):
        refs, movs = warm_pairs(dims, B=B)
        with batch_of(B, dims, niter, nscales, method, nrefine, warm_start=1) as b:
            b.register(refs, movs[0])
            first = b.info()["launches"]
            b.register(refs, movs[1])
            seen.append((first, b.info()["launches"]))
            b.set_option("warm_start", 0)
            b.register(refs, movs[1])
            assert b.info()["launches"] == cold
    assert seen == [(warm, warm), (warm, warm)]


# ------------------------------------------------------------ 10. more pairs than block slots
def test_more_pairs_than_block_slots(gpu, oracle):
    """600 workgroups of 1024 threads against the 512 the device holds at a
    time; the pack and the downsample take the pair as grid dimension z."""
    dims, niter, B, method = (16, 12), [3], 600, "diffusion"
    refs, movs, mA, R, W = supplied_case(oracle, dims, method, niter)
    which = np.arange(B) % 3
    with batch_of(B, dims, niter, 0, method, warm_start=1) as b:
        b.set_motion(mA[which])
        assert np.array_equal(b.motion(), mA[which])
        b.register(refs[which], movs[1][which])
        assert not b.status().any()
        got_m, got_w = b.motion(), b.warp(movs[1][which])
    assert R.any()
    assert np.array_equal(got_m, R[which])
    assert np.array_equal(got_w, W[which])
