#!/usr/bin/env python3
"""Batched Fluid against a sequence of one-pair registrations.

register() of B pairs in one BatchRegistration(reg=5) call, 200 fixed
iterations at nscales 0, on shifted disks so that the loops regrid, against B
registrations in sequence on one ImageRegistration(reg=5, fixed_iters=1) (a
reused object: its velocity carries over from pair to pair, which changes the
values and not the work of an iteration).  The one-pair path is the same code at
any tree, so both sides come from the library under test and run in one
process, interleaved: every round times the batch, then the sequence, for every
B of a size.  A figure is the minimum over the repetitions of a timed window
(after a warm-up call; at least 2, up to 10 or 0.5 s); the table holds the
median of the rounds' minima, as microseconds per pair and iteration, the loop
kernel's device time per iteration (HIP events, of2d_batch_info), and that time
per step of the sweep (2 dx + dy - 8 steps an iteration; the iteration's other
stages and its regrids are in that figure too), and the regrids per pair.  B = 1
is expected to be slower than the one-pair path: one workgroup is one compute
unit.

Writes profiles/batch_fluid_bench.log.  Not run by any test.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NITER, PARAMS = 200, [0.25, 0.0, 0.9]
# size: the batch sizes measured there
DEFAULT = {64: [1, 16, 64, 256, 1024], 128: [1, 16, 64, 256, 1024], 256: [64, 256]}


def pairs(n, count):
    import numpy as np
    from opticalflow2d_amd import synthetic as S
    # the disk of config 4 moved by an eighth of the side, eight directions
    d = n / 8.0
    base = [S.shifted_disk(n, shift=(round(d * np.cos(0.7 * k + 0.3)), round(d * np.sin(0.7 * k + 0.3))))
            for k in range(8)]
    refs = np.stack([base[k % 8][0] for k in range(count)])
    movs = np.stack([base[k % 8][1] for k in range(count)])
    return refs, movs


def timed(fn, min_s=0.5, max_reps=10):
    fn()  # warm-up: code objects, allocations
    ts = []
    while len(ts) < max_reps and (len(ts) < 2 or sum(ts) < min_s):
        t0 = time.perf_counter()
        fn()  # ends in a device synchronise (the library's entry points do)
        ts.append(time.perf_counter() - t0)
    return min(ts)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=sorted(DEFAULT))
    ap.add_argument("--batches", type=int, nargs="+", default=None,
                    help="for every size; the default is 1 16 64 256 1024, at 256 x 256 64 256")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seq-max", type=int, default=16,
                    help="the sequence runs min(B, this) registrations and is scaled per pair")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_fluid_bench.log"))
    a = ap.parse_args()
    from opticalflow2d_amd import BatchRegistration, ImageRegistration, set_print_sink
    set_print_sink(lambda s: None)
    lines = [f"# batched Fluid, {NITER} fixed iterations, mu {PARAMS[0]} lambda {PARAMS[1]} "
             f"omega {PARAMS[2]}, {a.rounds} interleaved rounds, median of the rounds' minima",
             "# size B | batch us/pair/it | loop kernel us/it (whole batch) | loop kernel ns/step "
             "| sequence us/pair/it | sequence / batch | regrids per pair (mean)"]
    for n in a.sizes:
        batches = a.batches or DEFAULT.get(n, DEFAULT[64])
        steps = 2 * n + n - 8
        got = {B: {"batch": [], "loop": [], "seq": [], "regrids": []} for B in batches}
        refs, movs = pairs(n, max(batches))
        for _ in range(a.rounds):
            for B in batches:
                with BatchRegistration(B, (n, n), [NITER], 0, PARAMS, reg=5, fixed_iters=1) as b:
                    t = timed(lambda: b.register(refs[:B], movs[:B]))
                    got[B]["batch"].append(1e6 * t / B / NITER)
                    got[B]["loop"].append(b.info()["loop_us"] / NITER)
                    got[B]["regrids"].append(sum(float(b.fluid_log(k)[0][:, 3].sum())
                                                 for k in range(min(B, 8))) / min(B, 8))
                nb = min(B, a.seq_max)
                with ImageRegistration((n, n), [NITER], 0, 5, PARAMS, fixed_iters=1) as r:
                    def seq():
                        for k in range(nb):
                            r.register(refs[k], movs[k])
                    t = timed(seq)
                    got[B]["seq"].append(1e6 * t / nb / NITER)
        for B in batches:
            m = {k: statistics.median(v) for k, v in got[B].items()}
            lines.append(f"{n:4d} {B:5d} | {m['batch']:9.3f} | {m['loop']:9.3f} | "
                         f"{1e3 * m['loop'] / steps:8.1f} | {m['seq']:9.3f} | "
                         f"{m['seq'] / m['batch']:7.2f} | {m['regrids']:6.1f}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
