#!/usr/bin/env python3
"""A 64-frame synthetic series registered against its first frame in one call.

Every frame is the first one translated a little further; BatchRegistration
runs the 64 Horn-Schunck registrations together (one workgroup per frame, each
stopping on its own iteration) and the per-frame iteration counts are printed.
With --reg 3 the registrations are Thirion's Demons (parameters 1, 0.25, 1.5,
2.5, kernel width 5, Composition); --diffeomorphic with it turns on the batch's
option of that name: Diffeomorphic Demons, every frame with its own number of
squarings per iteration.  With --reg 1 they are Curvature registrations (alpha
0.05, tau 50; --size must then be a power of two from 16 to 512, as must its
half, the coarser level).  With --reg 2 they are Elastic registrations (mu
0.05, lambda 0.02, omega 1.5; any size).  With --reg 5 they are viscous-fluid
registrations (mu 0.25, lambda 0, omega 0.9; the option "fluid" of an Elastic
batch, which the class sets): the regrids of every frame are counted from the
batch's log, and the reference's printed lines of the last frame are shown.

    python examples/demo_batch.py [--size 128] [--frames 64] [--niter 300] [--reg 1|2|3|5]
                                  [--diffeomorphic] [--resident] [--conv-lds] [--report]
                                  [--track T]

--resident (Horn-Schunck only) turns on the batch's option of that name: the
levels that fit keep the iterate in LDS and the gradients in registers across
the iterations.  The iteration counts and the motion are the same bits; the
placement per level is printed.

--conv-lds (--reg 3 only) turns on the batch's option "conv_lds": the levels
that fit keep the field the Demons loop's two convolutions read in LDS.  Again
the same bits, and the placement per level is printed.

--report adds the deformation analysis of the batch, one call each for all
frames: how many frames fold and the worst minimum Jacobian, the inverse of
every frame's motion, and MSE / NCC against frame 0 before and after.

--track T is another workload: T time frames of --frames slices each
(synthetic.cine_series: every slice's displacement grows a little from frame to
frame), registered frame after frame on one batch with warm_start=1, so that
frame t starts from frame t-1's motion, against a second batch that starts
every frame from zero.  It prints the mean iterations per pair of each frame,
warm against cold.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from opticalflow2d_amd import BatchRegistration  # noqa: E402
from opticalflow2d_amd import synthetic as S  # noqa: E402


# the parameters of --reg 1, 2 and 3; --reg 0 takes --alpha
REG_PARAMS = {0: None, 1: [0.05, 50.0], 2: [0.05, 0.02, 1.5], 3: [1.0, 0.25, 1.5, 2.5, 5, 0],
              5: [0.25, 0.0, 0.9]}


def options_of(a):
    options = {"diffeomorphic": 1} if a.diffeomorphic else {}
    if a.resident:
        options["resident"] = 1
    if a.conv_lds:
        options["conv_lds"] = 1
    return options


def track(a):
    """T frames of B slices, frame after frame: warm_start=1 against the default."""
    n, B, T = a.size, a.frames, a.track
    refs, frames, shifts = S.cine_series(n, B, T)
    params = REG_PARAMS[a.reg] or a.alpha
    options = options_of(a)
    rows = []
    with BatchRegistration(B, (n, n), [a.niter], 0, params, reg=a.reg, warm_start=1,
                           **options) as warm, \
            BatchRegistration(B, (n, n), [a.niter], 0, params, reg=a.reg, **options) as cold:
        for t in range(T):
            warm.register(refs, frames[t])
            cold.register(refs, frames[t])
            inner = (slice(None), slice(8, n - 8), slice(8, n - 8))
            rms = [np.sqrt(((b.warp(frames[t]) - refs) ** 2)[inner].mean()) for b in (warm, cold)]
            rows.append((np.abs(shifts[t]).max(), warm.iterations().mean(),
                         cold.iterations().mean(), rms[0], rms[1]))
    print(f"{T} frames of {B} slices of {n} x {n}, frame t from frame t-1's motion "
          f"(warm_start=1) against every frame from zero")
    print("frame  max shift (px)  mean iterations per pair: warm    cold   rms after: warm    cold")
    for t, (sh, wi, ci, wr, cr) in enumerate(rows):
        print(f"{t + 1:5d}  {sh:14.2f}  {wi:30.1f}  {ci:6.1f}  {wr:16.4f}  {cr:.4f}")
    print(f"mean iterations per pair and frame: warm {np.mean([r[1] for r in rows]):.1f}, "
          f"cold {np.mean([r[2] for r in rows]):.1f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--niter", type=int, default=300)
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--reg", type=int, default=0, choices=[0, 1, 2, 3, 5],
                    help="0 Horn-Schunck (alpha), 1 Curvature, 2 Elastic, 3 Thirion's Demons, "
                         "5 Fluid")
    ap.add_argument("--diffeomorphic", action="store_true",
                    help="with --reg 3: Diffeomorphic Demons (the option 'diffeomorphic')")
    ap.add_argument("--resident", action="store_true",
                    help="with --reg 0: the iterate on the CU at the levels that fit "
                         "(the option 'resident')")
    ap.add_argument("--conv-lds", action="store_true",
                    help="with --reg 3: the convolved field in LDS at the levels that fit "
                         "(the option 'conv_lds')")
    ap.add_argument("--report", action="store_true",
                    help="print the batch's Jacobian, inverse and quality summary")
    ap.add_argument("--track", type=int, default=0, metavar="T",
                    help="T time frames of --frames slices, frame after frame with warm_start=1")
    a = ap.parse_args()
    if a.diffeomorphic and a.reg != 3:
        ap.error("--diffeomorphic is an option of --reg 3")
    if a.resident and a.reg != 0:
        ap.error("--resident is an option of --reg 0")
    if a.conv_lds and a.reg != 3:
        ap.error("--conv-lds is an option of --reg 3")
    if a.track:
        return track(a)
    n, B = a.size, a.frames
    ref, _ = S.texture_pair(n, seed=3, sigma=3.0)
    # frame k: the first frame moved along a slow arc, up to ~2.5 px
    t = np.arange(1, B + 1) / B
    shifts = np.stack([2.5 * t * np.cos(2 * t), 2.5 * t * np.sin(2 * t)], axis=1)
    # texture_pair's second image is its first (one seed: ref) shifted bilinearly
    frames = np.stack([S.texture_pair(n, seed=3, sigma=3.0, shift=(sx, sy))[1]
                       for sx, sy in shifts])
    params = REG_PARAMS[a.reg] or a.alpha
    options = options_of(a)
    with BatchRegistration(B, (n, n), [a.niter, a.niter], 1, params, reg=a.reg, **options) as b:
        b.register(ref, frames)  # one reference shared by every frame
        motion = b.motion()
        iters = b.iterations()
        warped = b.warp(frames)
        info = b.info()
        if a.reg == 5:
            logs = [b.fluid_log(k) for k in range(B)]
            last_lines = b.fluid_lines(B - 1)
        if a.report:
            _, stats = b.jacobian(jac=False)
            _, inv = b.inverse_motion()
            quality = b.quality(ref, frames)
    print(f"{B} frames of {n} x {n} against frame 0: {info['launches']} kernel launches, "
          f"loop kernels {info['loop_us']} us")
    if a.resident:
        print(f"iterate placement per level from level 0 (1: on the CU): {info['placement']}")
    if a.conv_lds:
        print(f"convolved field's placement per level from level 0 (1: in LDS): "
              f"{info['placement']}")
    print("frame  shift (px)      iterations (coarse, fine)  mean motion (px)    rms before -> after")
    inner = (slice(None), slice(8, n - 8), slice(8, n - 8))
    before = np.sqrt(((frames - ref) ** 2)[inner].reshape(B, -1).mean(axis=1))
    after = np.sqrt(((warped - ref) ** 2)[inner].reshape(B, -1).mean(axis=1))
    mean = motion[:, 8:n - 8, 8:n - 8].reshape(B, -1, 2).mean(axis=1)
    for k in range(B):
        print(f"{k + 1:5d}  ({shifts[k, 0]:5.2f}, {shifts[k, 1]:5.2f})  {str(iters[k].tolist()):>24}  "
              f"({mean[k, 0]:5.2f}, {mean[k, 1]:5.2f})     {before[k]:.4f} -> {after[k]:.4f}")
    if a.reg == 5:
        regrids = [int(sum(loop[:, 3].sum() for loop in log)) for log in logs]
        print(f"regrids per frame: {regrids}")
        print(f"frame {B}: the reference's lines, the last 3 of {len(last_lines)}")
        for line in last_lines[-3:]:
            print("  " + line)
    if a.report:
        folded = sum(s["folded"] > 0 for s in stats)
        print(f"folded pairs {folded} of {B}, worst min Jacobian {min(s['min'] for s in stats):.4f}")
        print(f"inverse: mean {np.mean([i['iterations'] for i in inv]):.1f} iterations, "
              f"worst residual {max(i['residual'] for i in inv):.3e} px")
        mq = {k: np.mean([q[k] for q in quality]) for k in quality[0]}
        print(f"mean MSE {mq['mse_before']:.3e} -> {mq['mse_after']:.3e}, "
              f"mean NCC {mq['ncc_before']:.4f} -> {mq['ncc_after']:.4f}")


if __name__ == "__main__":
    main()
