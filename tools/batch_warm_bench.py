#!/usr/bin/env python3
"""BatchRegistration with warm_start 1 against 0 on a cine series.

The workload of examples/demo_batch.py --track (synthetic.cine_series): T time
frames of B slices whose displacement grows by a fixed step per frame,
registered frame after frame with register(), Diffusion (alpha 0.1, niter 200
per level), convergence on.  Sides, all on the same build:

  cold    warm_start 0: every frame starts from zero
  warm    warm_start 1: frame t starts from what frame t-1 left at every level
          (with nscales 2 that is the coarsest level's motion only)
  recipe  warm_start 1 and b.set_motion(b.motion_device()) after every frame
          (nscales 2 only): frame t starts from frame t-1's full-resolution
          result at every level; the hand-back is inside the timed window

Per configuration (size 128 and 256, B 64 and 256, nscales 0 and 2): the mean
iterations per pair and frame, summed over the loops of a pair, and the seconds
per pair and frame of register().  A repetition is the whole series after
reset_motion(), so every repetition of every side does the same work; a figure
is the minimum over a round's repetitions (after a warm-up series; at least 2,
up to 10 or 1 s), then the median of the rounds.  The driver alternates one
child process per side and round, so the sides are interleaved on one box.

Writes profiles/batch_warm_bench.log.  Not run by any test.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NITER, ALPHA = 200, 0.1
SIDES = ("cold", "warm", "recipe")


def timed_series(fn, min_s=1.0, max_reps=10):
    fn()  # warm-up: code objects, allocations, every shape of the window
    ts = []
    while len(ts) < max_reps and (len(ts) < 2 or sum(ts) < min_s):
        t0 = time.perf_counter()
        fn()  # every register() ends in a device synchronise
        ts.append(time.perf_counter() - t0)
    return min(ts)


def child(side, sizes, batches, scales, T, step):
    import numpy as np
    from opticalflow2d_amd import BatchRegistration, set_print_sink
    from opticalflow2d_amd import synthetic as S
    set_print_sink(lambda s: None)
    for n in sizes:
        for B in batches:
            refs, frames, _ = S.cine_series(n, B, T, step=step)
            for nscales in scales:
                if side == "recipe" and nscales == 0:
                    continue  # level 0 is the only level: warm is the recipe
                with BatchRegistration(B, (n, n), [NITER] * (nscales + 1), nscales, ALPHA,
                                       device=0, warm_start=0 if side == "cold" else 1) as b:
                    iters = []

                    def series():
                        iters.clear()
                        b.reset_motion()
                        for t in range(T):
                            b.register(refs, frames[t])
                            iters.append(b.iterations().sum(axis=1).mean())
                            if side == "recipe":
                                b.set_motion(b.motion_device())

                    dt = timed_series(series)
                    failed = int(b.status().astype(bool).sum())
                print(json.dumps({"side": side, "n": n, "B": B, "nscales": nscales, "T": T,
                                  "s_per_pair_frame": dt / (B * T), "failed": failed,
                                  "iters_per_frame": [float(x) for x in iters],
                                  "mean_iters": float(np.mean(iters)),
                                  "mean_iters_after_first": float(np.mean(iters[1:]))}),
                      flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--scales", type=int, nargs="+", default=[0, 2])
    ap.add_argument("--frames", type=int, default=6, help="time frames of the series")
    ap.add_argument("--step", type=float, default=0.3, help="displacement growth per frame (px)")
    ap.add_argument("--child", choices=SIDES)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_warm_bench.log"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.sizes, a.batches, a.scales, a.frames, a.step)
    common = ["--sizes", *map(str, a.sizes), "--batches", *map(str, a.batches), "--scales",
              *map(str, a.scales), "--frames", str(a.frames), "--step", str(a.step)]
    rows = []
    for rnd in range(a.rounds):
        for side in SIDES:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side,
                                *common], stdout=subprocess.PIPE, text=True, check=True)
            print(f"round {rnd}: {side} done", file=sys.stderr, flush=True)
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    rows.append(dict(json.loads(line), round=rnd))

    def med(side, n, B, s, key):
        v = [r[key] for r in rows if (r["side"], r["n"], r["B"], r["nscales"]) == (side, n, B, s)]
        return statistics.median(v) if v else None

    lines = [f"# tools/batch_warm_bench.py: Diffusion alpha {ALPHA}, niter {NITER} per level, "
             f"convergence on, {a.frames} frames, step {a.step} px per frame",
             f"# rounds {a.rounds}, sides interleaved per round; times: the minimum over a "
             "round's repetitions of the whole series, then the median of the rounds",
             "# iterations: mean per pair and frame, summed over a pair's loops "
             "(all frames | frames 2..T)",
             "size    B  nscales  side    iters all  iters 2..T   us/pair/frame   vs cold"]
    for n in a.sizes:
        for B in a.batches:
            for s in a.scales:
                cold = med("cold", n, B, s, "s_per_pair_frame")
                for side in SIDES:
                    t = med(side, n, B, s, "s_per_pair_frame")
                    if t is None:
                        continue
                    lines.append(f"{n:4d}  {B:3d}  {s:7d}  {side:6s}  {med(side, n, B, s, 'mean_iters'):9.1f}"
                                 f"  {med(side, n, B, s, 'mean_iters_after_first'):10.1f}"
                                 f"  {1e6 * t:14.1f}  {t / cold:7.3f}")
    lines += ["# rows"] + [json.dumps(r) for r in rows]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print("\n".join(lines[: 4 + 3 * len(a.sizes) * len(a.batches) * len(a.scales)]))


if __name__ == "__main__":
    main()
