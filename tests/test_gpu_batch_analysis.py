"""Batched deformation analysis (batch_analysis_kernels.hip): the Jacobian map
with its statistics, the inverse field and the similarity of every pair of a
stack in one launch each, at the per-launch entries (`prim.batch_*`) and on a
BatchRegistration.

References are the oracle (the Jacobian map, bit for bit) and the one-pair
entries `field.jacobian / invert / similarity`, which tests/test_gpu_analysis.py
holds to the oracle.  The maps, every iterate of the inverse, its residuals and
counts, minima, maxima and the integer counts are compared exactly (uint32
views).  The only tolerances are for fp64 sums taken in another order: the
Jacobian mean (2 n 2^-53 mean|J|, the bound for reordering an fp64 sum of n
terms) and MSE / NCC (1e-11 relative: non-negative images, n <= 10^4), as in
tests/test_gpu_analysis.py.

Shapes: (2, 2) and (16, 12) have fewer pixels than the workgroup's 1024
threads, (37, 29) is one round of pixels plus a ragged second, (130, 33)
crosses the 128 pitch, (97, 61) is ragged in both axes.  B = 1, 3, 5, and 300
pairs of (16, 12): more workgroups than compute units.

Arrays at the per-launch entries are in the C-ABI's layout with a leading pair
axis: images [B, dimy, dimx], motion [B, dimy, dimx, 2].
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from opticalflow2d_amd import BatchRegistration, ImageRegistration, field
from opticalflow2d_amd import synthetic as S
from opticalflow2d_amd.prims import prim
from opticalflow2d_amd.registration import INVERT_CHUNK

pytestmark = pytest.mark.gpu
F = np.float32

SHAPES = [(2, 2), (16, 12), (37, 29), (130, 33), (97, 61)]
BATCHES = [1, 3, 5]
ids = lambda s: "x".join(str(v) for v in s) if isinstance(s, tuple) else str(s)  # noqa: E731


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    if len(bad):
        k = tuple(bad[0])
        pytest.fail(f"{what}: {len(bad)} of {g.size} words differ, first at {k}: "
                    f"got {np.asarray(got, F)[k]!r} want {np.asarray(want, F)[k]!r}")


def same_beside_nan(got, want, what=""):
    """NaN in the same places, the same bits everywhere else."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    same(np.where(nan, F(0), got), np.where(nan, F(0), want), what)


def frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def sinusoids(dimx, dimy, amp):
    """tests/test_gpu_analysis.py's: ux = A sin(2 pi i / dimx + 0.3) cos(2 pi j / dimy),
    uy = 0.7 A cos(4 pi i / dimx) sin(2 pi j / dimy + 0.5)."""
    j, i = np.mgrid[0:dimy, 0:dimx].astype(np.float64)
    u = np.zeros((dimy, dimx, 2))
    u[..., 0] = amp * np.sin(2 * np.pi * i / dimx + 0.3) * np.cos(2 * np.pi * j / dimy)
    u[..., 1] = 0.7 * amp * np.cos(4 * np.pi * i / dimx) * np.sin(2 * np.pi * j / dimy + 0.5)
    return frozen(u.astype(F))


@functools.lru_cache(maxsize=None)
def noisy(dimx, dimy):
    """The smooth base plus seeded noise: mixed-sign derivatives everywhere."""
    rng = np.random.default_rng(dimx * 1000 + dimy)
    return frozen((sinusoids(dimx, dimy, 2.0) +
                   rng.uniform(-0.3, 0.3, (dimy, dimx, 2))).astype(F))


# ------------------------------------------------------------------ Jacobian
@functools.lru_cache(maxsize=None)
def jacobian_kinds(dimx, dimy):
    """Five fields that differ: noisy, a planted fold (du.x/dx = -1.5 at one
    pixel: J = -0.5), zero, smooth, and a uniform compression with J = 0.3."""
    fold = np.zeros((dimy, dimx, 2), F)
    fold[dimy // 2, min(dimx // 2 + 1, dimx - 1), 0] = -3.0
    half = np.zeros((dimy, dimx, 2), F)
    half[..., 0] = F(-0.7) * np.arange(dimx, dtype=F)[None, :]
    return (noisy(dimx, dimy), frozen(fold), frozen(np.zeros((dimy, dimx, 2), F)),
            sinusoids(dimx, dimy, 1.5), frozen(half))


@functools.lru_cache(maxsize=None)
def jacobian_wants(dimx, dimy):
    """The oracle's map of each kind, computed once."""
    from oracle import oracle as O
    out = []
    for u in jacobian_kinds(dimx, dimy):
        jac = np.zeros((dimy, dimx), F)
        O.lib().oracle_jacobian(np.ascontiguousarray(u).reshape(-1), dimx, dimy, jac.reshape(-1))
        out.append(frozen(jac))
    return tuple(out)


def check_jacobian_pair(st, jac, want, what):
    n = want.size
    same(jac, want, f"{what}: map")
    assert F(st[0]) == want.min() and F(st[1]) == want.max(), what
    assert st[3] == int((want <= 0).sum()) and st[4] == int((want < F(0.5)).sum()), what
    w64 = want.astype(np.float64)
    bound = 2 * n * 2.0 ** -53 * np.abs(w64).mean()
    print(f"{what}: mean {st[2]!r} numpy {w64.mean()!r} diff {abs(st[2] - w64.mean()):.3e} "
          f"bound {bound:.3e}")
    assert abs(st[2] - w64.mean()) <= bound, what


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_jacobian(gpu, oracle, shape, B):
    kinds, wants = jacobian_kinds(*shape), jacobian_wants(*shape)
    assert wants[1].min() < 0 and 0 < wants[4].min() and wants[4].max() < 0.5
    assert np.array_equal(bits(wants[2]), bits(np.ones_like(wants[2])))
    which = [k % 5 for k in range(B)]
    u = np.stack([kinds[k] for k in which])
    jac, st = prim.batch_jacobian(u)
    for p, k in enumerate(which):
        check_jacobian_pair(st[p], jac[p], wants[k], f"{ids(shape)} pair {p} (kind {k})")
    none, st2 = prim.batch_jacobian(u, jac=False)
    assert none is None and np.array_equal(st2.view(np.uint64), st.view(np.uint64))
    jac3, st3 = prim.batch_jacobian(u)
    assert np.array_equal(bits(jac3), bits(jac))
    assert np.array_equal(st3.view(np.uint64), st.view(np.uint64))
    if B > 1:  # no pair sees another: permuting the pairs permutes the results
        perm = np.roll(np.arange(B), 1)[::-1].copy()
        jp, sp = prim.batch_jacobian(u[perm])
        assert np.array_equal(bits(jp), bits(jac[perm]))
        assert np.array_equal(sp.view(np.uint64), st[perm].view(np.uint64))


# ------------------------------------------------------------------ inverse
def amplitude_scale(dimx, dimy):
    """tests/test_gpu_analysis.py's INVERTIBLE amplitudes are for about 61
    lines; smaller grids take them in proportion."""
    return min(1.0, min(dimx, dimy) / 61.0)


@functools.lru_cache(maxsize=None)
def invert_stack(dimx, dimy):
    s = amplitude_scale(dimx, dimy)
    fields = [np.zeros((dimy, dimx, 2), F), sinusoids(dimx, dimy, 3.0 * s),
              sinusoids(dimx, dimy, 2.0 * s), sinusoids(dimx, dimy, 0.4 * s)]
    nan = sinusoids(dimx, dimy, 1.0 * s).copy()
    nan[dimy // 2, dimx // 2, 1] = np.nan
    fields.append(nan)
    if (dimx, dimy) == (97, 61):
        fields.append(sinusoids(97, 61, 12.0))  # folded: never converges
    return frozen(np.stack(fields))


@functools.lru_cache(maxsize=None)
def invert_wants(dimx, dimy, max_iter, tol):
    """field.invert on each pair alone, once."""
    return tuple(field.invert(u, max_iter=max_iter, tol=tol) for u in invert_stack(dimx, dimy))


def check_invert_pair(v, info, res, want, max_iter, what):
    wv, winfo, wres = want
    n = winfo["iterations"]
    print(f"{what}: {winfo}")
    assert info[0] == n and info[2] == winfo["out_of_bounds"], what
    assert bool(info[3]) == winfo["converged"], what
    same_beside_nan(v, wv, f"{what}: inverse field")
    same_beside_nan(res[:n], wres, f"{what}: residuals")
    assert not res[n:].any() and len(res) == max_iter, what
    same_beside_nan(F(info[1]), F(winfo["residual"]), f"{what}: reported residual")


@pytest.mark.parametrize("max_iter", [1, INVERT_CHUNK + 1, 50])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_invert(gpu, shape, max_iter):
    tol = 1e-3
    u, wants = invert_stack(*shape), invert_wants(*shape, max_iter, tol)
    v, info, res = prim.batch_invert(u, max_iter=max_iter, tol=tol)
    for p, want in enumerate(wants):
        check_invert_pair(v[p], info[p], res[p], want, max_iter, f"{ids(shape)} pair {p}")
    its = [w[1]["iterations"] for w in wants]
    assert its[0] == 1 and wants[0][1]["converged"] and not np.asarray(wants[0][0]).any()
    if max_iter == 1:
        assert its == [1] * len(wants)
    else:
        # the pairs really stop on different updates
        print(f"{ids(shape)} max_iter {max_iter}: iterations {its}")
        assert len(set(its)) >= 2, its
        if shape == (97, 61) and max_iter == 50:
            assert len(set(its[1:4])) == 3 and max(its[1:4]) < 50, its
    # the planted NaN reaches the first residual (v_0 = 0 samples the pixel itself)
    assert np.isnan(wants[4][2][0]) and its[4] >= min(2, max_iter)
    if shape == (97, 61) and max_iter > 1:
        assert its[5] == max_iter and not wants[5][1]["converged"]
    v2, info2, res2 = prim.batch_invert(u, max_iter=max_iter, tol=tol)
    assert np.array_equal(bits(v2), bits(v)) and np.array_equal(bits(res2), bits(res))
    assert np.array_equal(info2.view(np.uint64), info.view(np.uint64))
    # without the residuals array, and with the pairs in another order
    perm = np.roll(np.arange(len(u)), 2)
    vp, ip, none = prim.batch_invert(u[perm], max_iter=max_iter, tol=tol, residuals=False)
    assert none is None
    assert np.array_equal(bits(vp), bits(v[perm]))
    assert np.array_equal(ip.view(np.uint64), info[perm].view(np.uint64))


# ------------------------------------------------------------------ similarity
@functools.lru_cache(maxsize=None)
def image_stacks(dimx, dimy, B):
    rng = np.random.default_rng(7 * dimx + dimy + B)
    a = rng.uniform(0.0, 1.0, (B, dimy, dimx)).astype(F)
    b = (0.6 * a + 0.4 * rng.uniform(0.0, 1.0, (B, dimy, dimx))).astype(F)
    return frozen(a), frozen(b)


def numpy_similarity(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    da, db = a - a.mean(), b - b.mean()
    return ((a - b) ** 2).mean(), (da * db).mean() / np.sqrt((da * da).mean() * (db * db).mean())


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_similarity(gpu, shape, B):
    a, b = image_stacks(*shape, B)
    for shared in (False, True):
        got = prim.batch_similarity(a[0] if shared else a, b)
        for p in range(B):
            wm, wn = numpy_similarity(a[0] if shared else a[p], b[p])
            print(f"{ids(shape)} pair {p} shared {shared}: mse {got[p, 0]!r} numpy {wm!r}; "
                  f"ncc {got[p, 1]!r} numpy {wn!r}")
            assert abs(got[p, 0] - wm) <= 1e-11 * abs(wm)
            assert abs(got[p, 1] - wn) <= 1e-11 * abs(wn)
        again = prim.batch_similarity(a[0] if shared else a, b)
        assert np.array_equal(again.view(np.uint64), got.view(np.uint64))
    same_img = prim.batch_similarity(a, a)
    assert not same_img[:, 0].any() and np.all(np.abs(same_img[:, 1] - 1.0) <= 1e-11)


@pytest.mark.parametrize("which", ["a", "b"])
def test_similarity_constant_image_is_per_pair(gpu, which):
    a, b = (x.copy() for x in image_stacks(37, 29, 5))
    clean = prim.batch_similarity(a, b)
    (a if which == "a" else b)[2] = F(0.7)
    got = prim.batch_similarity(a, b)
    assert np.isnan(got[2, 1]) and not np.isnan(np.delete(got, 2, axis=0)).any()
    want = ((a[2].astype(np.float64) - b[2].astype(np.float64)) ** 2).mean()
    assert abs(got[2, 0] - want) <= 1e-11 * want
    keep = [0, 1, 3, 4]
    assert np.array_equal(got[keep].view(np.uint64), clean[keep].view(np.uint64))


# ------------------------------------------------------------------ more pairs than compute units
def test_300_pairs(gpu, oracle):
    """300 workgroups of 1024 threads on (16, 12): every pair's results are
    those of its kind, whichever workgroup slot it ran in."""
    dimx, dimy, B = 16, 12, 300
    which = (np.arange(B) * 3 + np.arange(B) // 128) % 5
    assert len(set(which.tolist())) == 5
    kinds, wants = jacobian_kinds(dimx, dimy), jacobian_wants(dimx, dimy)
    jac, st = prim.batch_jacobian(np.stack([kinds[k] for k in which]))
    first = {k: int(np.argmax(which == k)) for k in range(5)}
    for k, p in first.items():
        check_jacobian_pair(st[p], jac[p], wants[k], f"pair {p} (kind {k})")
    for p, k in enumerate(which):
        assert np.array_equal(bits(jac[p]), bits(wants[k])), p
        assert np.array_equal(st[p].view(np.uint64), st[first[k]].view(np.uint64)), p
    u, inv = invert_stack(dimx, dimy), invert_wants(dimx, dimy, 50, 1e-3)
    v, info, res = prim.batch_invert(u[which], max_iter=50, tol=1e-3)
    for p, k in enumerate(which):
        if p == first[k]:
            check_invert_pair(v[p], info[p], res[p], inv[k], 50, f"pair {p} (field {k})")
        assert np.array_equal(bits(v[p]), bits(v[first[k]])), p
        assert np.array_equal(info[p].view(np.uint64), info[first[k]].view(np.uint64)), p
        assert np.array_equal(bits(res[p]), bits(res[first[k]])), p
    a, b = image_stacks(dimx, dimy, 5)
    sim = prim.batch_similarity(a[which], b[which])
    five = prim.batch_similarity(a, b)
    assert np.array_equal(sim.view(np.uint64), five[which].view(np.uint64))


# ------------------------------------------------------------------ on a BatchRegistration
DEMONS = [1.0, 0.25, 1.5, 2.5, 5, 0]
REGS = {"hs": (0, [0.1], 0.1, [12]), "demons": (3, DEMONS, DEMONS, [6])}


@functools.lru_cache(maxsize=None)
def pairs(dimx, dimy, B=3, seed0=10):
    """tests/test_gpu_batch.py's make_pairs: textured pairs with different shifts."""
    refs, movs = [], []
    for k in range(B):
        shift = (0.4 + 0.35 * k, -0.3 - 0.2 * k if k % 2 else 0.25 + 0.15 * k)
        r, m = S.texture_pair(dimx, seed=seed0 + k, sigma=2.0, shift=shift, ny=dimy)
        refs.append(r)
        movs.append(m)
    return frozen(np.stack(refs)), frozen(np.stack(movs))


def image32(a):
    """[dimx, dimy] (the boundary's layout) -> float32 [dimy, dimx]."""
    return np.ascontiguousarray(np.asarray(a).T, dtype=F)


def check_against_one_pair(reg, params, niter, dims, ref, mov, warped, jac, st, inv, info, q,
                           what):
    """The batch's results for one pair: the bit-exact ones against an
    ImageRegistration on that pair, the reordered fp64 sums against numpy at
    the bounds of the per-launch tests."""
    n = dims[0] * dims[1]
    with ImageRegistration(dims, niter, 0, reg, params, 1, fixed_iters=1, device=0) as r:
        r.register(ref, mov)
        wjac, wst = r.jacobian()
        winv, winfo = r.inverse_motion()
        wq = r.quality(ref, mov)
        wwarp = r.warp(mov)
    assert np.array_equal(np.asarray(jac, np.float64).view(np.uint64), wjac.view(np.uint64)), what
    assert (st["min"], st["max"], st["folded"], st["below_half"]) == \
        (wst["min"], wst["max"], wst["folded"], wst["below_half"]), what
    bound = 2 * n * 2.0 ** -53 * np.abs(wjac).mean()
    print(f"{what}: mean {st['mean']!r} one-pair {wst['mean']!r} numpy {wjac.mean()!r} "
          f"bound {bound:.3e}")
    assert abs(st["mean"] - wjac.mean()) <= bound, what
    assert np.array_equal(np.asarray(inv, np.float64).view(np.uint64), winv.view(np.uint64)), what
    assert info == winfo, what
    assert np.array_equal(warped.view(np.uint64), wwarp.view(np.uint64)), what
    before = numpy_similarity(image32(ref), image32(mov))
    after = numpy_similarity(image32(ref), image32(warped))
    print(f"{what}: batch {q} one-pair {wq} numpy {before + after}")
    for key, want in zip(("mse_before", "ncc_before", "mse_after", "ncc_after"), before + after):
        assert abs(q[key] - want) <= 1e-11 * abs(want), f"{what} {key}: {q[key]!r} {want!r}"
        assert abs(wq[key] - want) <= 1e-11 * abs(want), f"{what} one-pair {key}"


@pytest.mark.parametrize("dims", [(37, 29), (130, 33)], ids=ids)
@pytest.mark.parametrize("name", list(REGS))
def test_on_a_batch(gpu, name, dims):
    import torch
    reg, one_params, alpha, niter = REGS[name]
    refs, movs = pairs(*dims)
    B = len(movs)
    L = __import__("opticalflow2d_amd")._lib.lib()
    with BatchRegistration(B, dims, niter, 0, alpha, reg=reg, fixed_iters=1, device=0) as b:
        # before the first estimate the motion is zero
        _, st0 = b.jacobian(jac=False)
        assert all(s == {"min": 1.0, "max": 1.0, "mean": 1.0, "folded": 0, "below_half": 0}
                   for s in st0)
        b.register(refs, movs)
        m0 = b.motion()
        launches = b.info()["launches"]
        assert all(np.abs(m0[k]).max() > 0.05 for k in range(B))
        jac, st = b.jacobian()
        none, st2 = b.jacobian(jac=False)
        inv, info = b.inverse_motion()
        q = b.quality(refs, movs)
        qs = b.quality(refs[0], movs)
        warped = b.warp(movs)
        assert none is None and st2 == st
        assert jac.shape == (B,) + dims and inv.shape == (B,) + dims + (2,)
        # CUDA tensors: float32 and float64, contiguous and a transposed view
        dev = torch.device("cuda", 0)
        for dtype in (torch.float32, torch.float64):
            for transposed in (False, True):
                if transposed:
                    jt = torch.zeros((B, dims[1], dims[0]), dtype=dtype, device=dev).transpose(1, 2)
                    vt = torch.zeros((B, dims[1], dims[0], 2), dtype=dtype,
                                     device=dev).transpose(1, 2)
                    assert not jt.is_contiguous() and not vt.is_contiguous()
                else:
                    jt = torch.zeros((B,) + dims, dtype=dtype, device=dev)
                    vt = torch.zeros((B,) + dims + (2,), dtype=dtype, device=dev)
                out, std = b.jacobian(out=jt)
                assert out is jt and std == st
                assert np.array_equal(jt.cpu().numpy().astype(np.float64), jac)
                out, infod = b.inverse_motion(out=vt)
                assert out is vt and infod == info
                assert np.array_equal(vt.cpu().numpy().astype(np.float64).view(np.uint64),
                                      inv.view(np.uint64))
                rt = torch.as_tensor(np.array(refs), dtype=dtype, device=dev)
                mt = torch.as_tensor(np.array(movs), dtype=dtype, device=dev)
                if transposed:
                    rt = rt.transpose(1, 2).contiguous().transpose(1, 2)
                    mt = mt.transpose(1, 2).contiguous().transpose(1, 2)
                if dtype == torch.float64:  # the float32 tensors hold other images
                    assert b.quality(rt, mt) == q and b.quality(rt[0], mt) == qs
                else:
                    q32 = b.quality(rt, mt)
                    assert q32 == b.quality(rt.cpu().numpy(), mt.cpu().numpy())
        # nothing above touched the motion, the stored images or the launch count
        assert np.array_equal(b.motion().view(np.uint64), m0.view(np.uint64))
        assert b.info()["launches"] == launches
        b._chk(L.of2d_batch_estimate(b._h))
        assert np.array_equal(b.motion().view(np.uint64), m0.view(np.uint64))
        assert b.info()["launches"] == launches
    for k in range(B):
        check_against_one_pair(reg, one_params, niter, dims, refs[k], movs[k], warped[k], jac[k],
                               st[k], inv[k], info[k], q[k], f"{name} {ids(dims)} pair {k}")
        assert q[k]["mse_after"] < q[k]["mse_before"]
    for key in ("mse_before", "ncc_before", "mse_after", "ncc_after"):
        assert qs[0][key] == q[0][key]  # pair 0's reference is the shared one


@pytest.mark.parametrize("name", list(REGS))
def test_failed_pair(gpu, name):
    """A pair with a zero denominator keeps a zero motion: J = 1, a zero
    inverse that converged at its first update, after == before."""
    from opticalflow2d_amd import _lib
    reg, _, alpha, niter = REGS[name]
    dims, bad = (40, 33), 2  # tests/test_gpu_batch.py's divide-by-zero case
    refs, movs = (x.copy() for x in pairs(*dims, 4))
    refs[bad] = 0.5
    movs[bad] = 0.5
    with BatchRegistration(4, dims, niter, 0, 0.0 if reg == 0 else alpha, reg=reg, fixed_iters=1,
                           device=0) as b:
        b.register(refs, movs)
        assert b.status().tolist() == [0, 0, _lib.OF2D_ERR_RUNTIME, 0]
        jac, st = b.jacobian()
        inv, info = b.inverse_motion()
        refs[bad], movs[bad] = (x[bad] for x in pairs(*dims, 4))  # something to warp
        q = b.quality(refs, movs)
    assert np.array_equal(jac[bad], np.ones(dims))
    assert st[bad] == {"min": 1.0, "max": 1.0, "mean": 1.0, "folded": 0, "below_half": 0}
    assert not inv[bad].any()
    assert info[bad] == {"iterations": 1, "residual": 0.0, "out_of_bounds": 0, "converged": True}
    assert q[bad]["mse_before"] > 0 and abs(q[bad]["ncc_before"]) < 1
    assert (q[bad]["mse_after"], q[bad]["ncc_after"]) == (q[bad]["mse_before"],
                                                          q[bad]["ncc_before"])
    for k in (0, 1, 3):
        assert info[k]["iterations"] > 1 and q[k]["mse_after"] != q[k]["mse_before"]


# ------------------------------------------------------------------ the demo's report
def test_demo_batch_report(gpu):
    import re
    from conftest import ROOT
    demo = os.path.join(ROOT, "examples", "demo_batch.py")
    out = subprocess.run([sys.executable, demo, "--size", "32", "--frames", "4", "--niter", "5",
                          "--report"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    text = out.stdout
    assert re.search(r"^folded pairs \d+ of 4, worst min Jacobian [-0-9.]+$", text, re.M), text
    assert re.search(r"^inverse: mean [0-9.]+ iterations, worst residual [0-9.e+-]+ px$", text,
                     re.M), text
    m = re.search(r"^mean MSE ([0-9.e+-]+) -> ([0-9.e+-]+), mean NCC ([-0-9.]+) -> ([-0-9.]+)$",
                  text, re.M)
    assert m, text
