"""The one-pair motion input on the device (ImageRegistration.set_motion,
reset_motion; include/of2d.h of2d_set_motion): a supplied motion continues as
the oracle's reused object does, through the host and the device form; the
pyramid's start {m, downSample(m)}; reset_motion gives a new object's result;
set_motion then motion() is the identity."""
import numpy as np
import pytest

from test_warm_reference import (ALPHA, downsample_motion, estimate_from, f32, field_of,
                                 level_dims, motion_of, warm_pairs, zero_levels)

pytestmark = pytest.mark.gpu

DIMS = (40, 24)
# regularisation, parameters
METHODS = {"diffusion": (0, [ALPHA]), "thirion": (3, [1.0, 2.0, 1.0, 1.0, 5, 0]),
           "elastic": (2, [0.5, 0.25]), "fluid": (5, [0.25, 0.0])}


def device_of(method, niter, nscales, nrefine=1, dims=DIMS):
    from opticalflow2d_amd import ImageRegistration
    reg, p = METHODS[method]
    return ImageRegistration(dims, niter, nscales, reg, p, nrefine, fixed_iters=1, device=0)


def tensors_of(m):
    """``m`` [dimx, dimy, 2] as CUDA tensors: contiguous (y faster than x),
    x faster, planar float64, and a base one element off the pair's alignment."""
    import torch
    m32 = f32(m)
    t = torch.from_numpy(m32).to("cuda")
    rows = torch.from_numpy(np.ascontiguousarray(m32.transpose(1, 0, 2))).to("cuda")
    planar = torch.from_numpy(np.ascontiguousarray(m32.transpose(2, 1, 0)).astype(np.float64))
    flat = torch.zeros(m32.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = t.reshape(-1)
    out = {"f32_contiguous": t, "f32_x_fastest": rows.permute(1, 0, 2),
           "f64_planar": planar.to("cuda").permute(2, 1, 0),
           "f32_offset": flat[1:].view(*m32.shape)}
    for name, x in out.items():
        assert np.array_equal(x.cpu().numpy().astype(np.float32), m32), name
    return out


@pytest.mark.parametrize("method", ["diffusion", "thirion", "elastic"])
def test_supplied_motion_continues_as_the_reused_oracle(gpu, oracle, method):
    reg, p = METHODS[method]
    niter = [6]
    refs, movs = warm_pairs(DIMS)
    o = oracle.Registration(DIMS, niter, 0, reg, p, 1, fixed_iters=True)
    o.register(refs[0], movs[0][0])
    mA = o.motion()
    o.register(refs[0], movs[1][0])
    R, W = o.motion(), o.warp(movs[1][0])
    o.close()
    assert mA.any() and not np.array_equal(mA, R)
    forms = {"host": mA}
    forms.update(tensors_of(mA))
    for name, m in forms.items():
        with device_of(method, niter, 0) as r:
            r.set_motion(m)
            assert np.array_equal(r.motion(), mA), name
            r.register(refs[0], movs[1][0])
            assert np.array_equal(r.motion(), R), name
            assert np.array_equal(r.warp(movs[1][0]), W), name


def test_supplied_motion_pyramid(gpu, oracle):
    niter, nscales, nrefine = [4, 5, 6], 2, 2
    refs, movs = warm_pairs(DIMS)
    o = oracle.Registration(DIMS, [6], 0, 0, [ALPHA], 1, fixed_iters=True)
    o.register(refs[1], movs[0][1])
    mA = o.motion()
    o.close()
    lv = zero_levels(DIMS, nscales)
    lv[0] = field_of(mA)
    lv[nscales] = downsample_motion(oracle, lv[0], level_dims(DIMS, nscales)[nscales])
    want = motion_of(estimate_from(oracle, lv, refs[1], movs[1][1], niter, nscales, nrefine,
                                   ALPHA)[0][0])
    forms = {"host": mA}
    forms.update(tensors_of(mA))
    with device_of("diffusion", niter, nscales, nrefine) as r:
        for name, m in forms.items():
            r.set_motion(m)
            r.register(refs[1], movs[1][1])
            assert np.array_equal(r.motion(), want), name


@pytest.mark.parametrize("method, niter, nscales, dims", [
    ("diffusion", [4, 5, 6], 2, DIMS), ("thirion", [5, 6], 1, DIMS), ("elastic", [6], 0, DIMS),
    ("fluid", [6], 0, (96, 96))])
def test_reset_motion_gives_a_new_object(gpu, method, niter, nscales, dims):
    """Fluid: the velocity survives an estimate as the motion does, so the
    reset clears it too."""
    refs, movs = warm_pairs(dims)
    with device_of(method, niter, nscales, dims=dims) as fresh:
        fresh.register(refs[0], movs[2][0])
        want = fresh.motion()
    with device_of(method, niter, nscales, dims=dims) as r:
        r.register(refs[0], movs[0][0])
        r.register(refs[0], movs[1][0])
        r.reset_motion()
        assert not r.motion().any()
        r.register(refs[0], movs[2][0])
        assert want.any() and np.array_equal(r.motion(), want)
        r.register(refs[0], movs[2][0])  # and without the reset it continues
        assert not np.array_equal(r.motion(), want)


@pytest.mark.parametrize("dims", [(37, 21), (1, 9), (9, 1), (70, 67), (130, 17)])
def test_set_motion_then_motion_is_the_identity(gpu, dims):
    from opticalflow2d_amd import ImageRegistration
    m = f32(3.0 * np.random.default_rng(5).standard_normal(dims + (2,)))
    forms = {"host": m.astype(np.float64)}
    forms.update(tensors_of(m))
    with ImageRegistration(dims, [3], 0, 0, [ALPHA], fixed_iters=1, device=0) as r:
        for name, t in forms.items():
            r.reset_motion()
            r.set_motion(t)
            assert np.array_equal(r.motion().astype(np.float32).view(np.uint32),
                                  m.view(np.uint32)), name
            back = r.motion_device().cpu().numpy()
            assert np.array_equal(back.view(np.uint32), m.view(np.uint32)), name
