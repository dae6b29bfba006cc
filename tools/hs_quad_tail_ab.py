#!/usr/bin/env python3
"""Interleaved A/B of the slab option hs_quad_tail_exchange in one process
(profiles/quad_tail_ab.log, the "round ..." lines).

    python tools/hs_quad_tail_ab.py [--grid 4096] [--rounds 4] [--steps 10] [--warmup 8]

bench.py's timed loop on bench.py's inputs (config 2: the procedural pair,
alpha 0.1, 1000 fixed iterations per step, the Logger sums reserved): after
`--warmup` steps, `--rounds` times option 0 (the quad kernel without the
end-of-band exchange) then 1 (with it), each one
untimed step and then `--steps` timed steps, wall clock around the steps as
bench.py takes it.  Prints per round and setting: ms per step, Mpx-it/s, the
GPU time per step by HIP events and the fused kernel's own launch time
(of2d_slab_last_run_kernel_us), per launch and per iteration.

The other half of profiles/quad_tail_ab.log is bench.py itself, alternating between
two builds of the library in one call:
    OF2D_LIB_PATH=<the parent commit's libof2d.so> python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 1 --steps 20 --warmup 5
three rounds, and both once more with --steps 2 --warmup 1 --dump-outputs DIR,
the arrays compared byte for byte.
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
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--iters-per-step", type=int, default=1000)
    args = ap.parse_args()
    lib()
    n, ips, steps = args.grid, args.iters_per_step, args.steps
    s = SlabSolver(n, n, 0.1)
    ref, mov = S.procedural_pair(n, 0, n)
    s.set_images(ref, mov)
    s.set_option("hs_gradients_from_image", -1)
    s.reserve(ips)
    for _ in range(args.warmup):
        s.run(ips, fixed_iters=True)
    for rnd in range(args.rounds):
        for q in (0, 1):
            s.set_option("hs_quad_tail_exchange", q)
            k = s.info()["iterations_per_launch"]
            assert k == 4 and s.info()["quad_tail_exchange"] == q
            s.run(ips, fixed_iters=True)
            gpu_ms, us_sum, cnt = 0.0, 0.0, 0
            t0 = time.perf_counter()
            for _ in range(steps):
                s.run(ips, fixed_iters=True)
                gpu_ms += s.last_run_ms()
                us, c = s.last_run_kernel_us()
                us_sum += us * c
                cnt += c
            dt = time.perf_counter() - t0
            print(f"round {rnd} tail_exchange {q} iters/launch {k}: ms_per_step {1000 * dt / steps:.4f} "
                  f"value {n * n * ips * steps / dt / 1e6:.1f} Mpx-it/s  "
                  f"gpu_ms/step {gpu_ms / steps:.4f} launch_us {us_sum / cnt:.3f} "
                  f"({us_sum / cnt / k:.3f} per iteration)", flush=True)
    s.close()


if __name__ == "__main__":
    main()
