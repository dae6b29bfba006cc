#!/usr/bin/env python3
"""bench.py's timed loop on a 4096^2 pair with large flat regions
(profiles/quad_fixup_ab.log, the "flat" lines).

    [OF2D_LIB_PATH=<another build's libof2d.so>] python tools/hs_fixup_flat_ab.py \
        [--grid 4096] [--steps 20] [--warmup 5] [--flat-from 0.25] [--flat-to 0.5]

The procedural pair of config 2 with the j-lines [flat-from, flat-to) x grid of
the moving image set to a constant: their gradients are exactly 0 (and those
of the two j-lines around the block in y), It = Imov - Iref is not, so the
quad kernel's row steps there take the unscaled division WITH its fix-up
(hs_jacobi_impl.h, the comment above hs::recip_refined), the others without.
One process times one library, as bench.py does (alpha 0.1, 1000 fixed
iterations per step, the Logger sums reserved, wall clock around the steps);
the A/B alternates processes between two builds in one call.  Prints one line:
ms per step, Mpx-it/s and the fused kernel's own launch time.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflow2d_amd import SlabSolver, lib  # noqa: E402
from opticalflow2d_amd import synthetic as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters-per-step", type=int, default=1000)
    ap.add_argument("--flat-from", type=float, default=0.25)
    ap.add_argument("--flat-to", type=float, default=0.5)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    lib()
    n, ips, steps = args.grid, args.iters_per_step, args.steps
    ref, mov = S.procedural_pair(n, 0, n)
    j0, j1 = int(args.flat_from * n), int(args.flat_to * n)
    mov = mov.copy()
    mov[:, j0:j1] = 0.5
    s = SlabSolver(n, n, 0.1)
    s.set_images(ref, mov)
    s.set_option("hs_gradients_from_image", -1)
    s.reserve(ips)
    assert s.info()["iterations_per_launch"] == 4
    for _ in range(args.warmup):
        s.run(ips, fixed_iters=True)
    us_sum, cnt = 0.0, 0
    t0 = time.perf_counter()
    for _ in range(steps):
        s.run(ips, fixed_iters=True)
        us, c = s.last_run_kernel_us()
        us_sum += us * c
        cnt += c
    dt = time.perf_counter() - t0
    print(f"{args.tag} flat j-lines [{j0}, {j1}) of {n}: ms_per_step {1000 * dt / steps:.5f} "
          f"value {n * n * ips * steps / dt / 1e6:.1f} avg_launch_us {us_sum / cnt:.3f}", flush=True)
    s.close()


if __name__ == "__main__":
    main()
