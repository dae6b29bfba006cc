#!/usr/bin/env python3
"""BatchRegistration reg=3 with conv_lds=1 against conv_lds=0.

The same handle's estimate with the Demons loop's convolved field in LDS
(option "conv_lds") against the global-memory loop, alternating in one process
on one box: for every row the two sides are timed one after the other within a
round, and the rounds follow one another, so both sides see the same machine
state.  Never a figure against an earlier run of the code.

Workload: tools/batch_demons_bench.py's (100 fixed iterations per level, eight
textured pairs repeated), Thirion with [1, 0.25, 1.5, 2.5, 5, 0] and
diffeomorphic with [1, 2, 1, 1, 5, 0], at 64 x 64 and 128 x 128 for B = 1, 16,
64, 256 with nscales 0, and one pyramid run: 256 x 256, nscales 2, B = 64
(levels 128 and 64 in LDS, level 0 in global memory).

Every figure is the minimum over a round's repetitions of the timed estimate
(after a warm-up call; at least 2, up to 20 or 0.3 s), then the median of the
rounds.  Per row: the loop kernels' device time per iteration (HIP events,
of2d_batch_info), seconds per pair for the estimate, the ratio conv_lds=0 /
conv_lds=1 of each (above 1: conv_lds is faster) and the spread of the loop
time over the rounds, (max - min) / median, the larger of the two sides'.  The
motion of the two sides is compared once per row (np.array_equal).

Writes profiles/batch_demons_lds_bench.log.  Not run by any test.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NITER = 100
METHODS = {"thirion": ([1.0, 0.25, 1.5, 2.5, 5, 0], 0),
           "diffeo": ([1.0, 2.0, 1.0, 1.0, 5, 0], 1)}
SHIFTS = [(1.5, -0.75), (0.6, 0.4), (-1.1, 0.3), (0.9, 1.2), (-0.4, -0.8), (1.3, 0.2),
          (0.2, -1.4), (-0.7, 0.9)]


def pairs(n, count):
    """`count` textured pairs cycling through 8 seeds and shifts."""
    import numpy as np
    from opticalflow2d_amd import synthetic as S
    base = [S.texture_pair(n, seed=20 + k, sigma=3.0, shift=sh) for k, sh in enumerate(SHIFTS)]
    refs = np.stack([base[k % 8][0] for k in range(count)])
    movs = np.stack([base[k % 8][1] for k in range(count)])
    return refs, movs


def timed(fn, min_s=0.3, max_reps=20):
    fn()  # warm-up
    ts = []
    while len(ts) < max_reps and (len(ts) < 2 or sum(ts) < min_s):
        t0 = time.perf_counter()
        fn()  # ends in a device synchronise (the library's entry points do)
        ts.append(time.perf_counter() - t0)
    return min(ts)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--methods", nargs="+", default=list(METHODS), choices=list(METHODS))
    ap.add_argument("--no-pyramid", action="store_true", help="leave the 256 x 256 run out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_demons_lds_bench.log"))
    a = ap.parse_args()

    import numpy as np
    from opticalflow2d_amd import BatchRegistration, _lib, set_print_sink
    set_print_sink(lambda s: None)
    L = _lib.lib()

    configs = [(m, n, B, [NITER], 0) for m in a.methods for n in a.sizes for B in a.batches]
    if not a.no_pyramid:
        configs += [(m, 256, 64, [NITER] * 3, 2) for m in a.methods]
    rows, same, placement = [], {}, {}
    for method, n, B, niter, nscales in configs:
        refs, movs = pairs(n, B)
        total_it = sum(niter)
        params, diffeo = METHODS[method]
        with BatchRegistration(B, (n, n), niter, nscales, params, reg=3, device=0, fixed_iters=1,
                               diffeomorphic=diffeo) as b:
            b.register(refs, movs)  # the upload, once: the sides time the estimate alone
            motion = {}
            for rnd in range(a.rounds):
                for conv_lds in (0, 1):
                    b.set_option("conv_lds", conv_lds)
                    t = timed(lambda: b._chk(L.of2d_batch_estimate(b._h)))
                    info = b.info()
                    rows.append({"method": method, "n": n, "B": B, "nscales": nscales,
                                 "conv_lds": conv_lds, "round": rnd, "s_per_pair_estimate": t / B,
                                 "loop_us_per_iter": info["loop_us"] / total_it,
                                 "placement": info["placement"],
                                 "failed": int(np.count_nonzero(b.status()))})
                    print(json.dumps(rows[-1]), flush=True)
                    if rnd == 0:
                        motion[conv_lds] = b.motion()
                        placement[method, n, B, nscales, conv_lds] = info["placement"]
            same[method, n, B, nscales] = bool(np.array_equal(motion[0], motion[1]))

    def col(key, side, cfg):
        return [r[key] for r in rows
                if (r["method"], r["n"], r["B"], r["nscales"], r["conv_lds"]) == cfg + (side,)]

    lines = ["# tools/batch_demons_lds_bench.py: BatchRegistration reg=3, conv_lds=1 against "
             "conv_lds=0",
             f"# rounds {a.rounds}, the two sides alternating in one process; every figure: the "
             "minimum over a round's repetitions (2 to 20, 0.3 s), then the median of the rounds",
             f"# niter {NITER} per level, fixed_iters; thirion {METHODS['thirion'][0]}, diffeo "
             f"{METHODS['diffeo'][0]} with diffeomorphic=1; the estimate alone (no upload)",
             "# ratio: conv_lds=0 / conv_lds=1 (above 1: conv_lds is faster); spread: (max - min) "
             "/ median of the loop time over the rounds, the larger side's",
             "method   size nscales     B  placement   loop us/iter c=0       c=1   ratio  spread   "
             "est s/pair c=0         c=1   ratio  same bits"]
    for method, n, B, niter, nscales in configs:
        cfg = (method, n, B, nscales)
        ls = [col("loop_us_per_iter", side, cfg) for side in (0, 1)]
        l0, l1 = (statistics.median(v) for v in ls)
        spread = max((max(v) - min(v)) / max(statistics.median(v), 1e-9) for v in ls)
        e0, e1 = (statistics.median(col("s_per_pair_estimate", side, cfg)) for side in (0, 1))
        lines.append(f"{method:8s} {n:4d} {nscales:7d} {B:5d}  "
                     f"{str(placement[cfg + (1,)]):>9}  "
                     f"{l0:16.2f} {l1:9.2f}  {l0 / max(l1, 1e-9):6.2f}  {spread:6.3f}   "
                     f"{e0:14.3e}  {e1:10.3e}  {e0 / e1:6.2f}  {same[cfg]}")
    ntable = len(lines)
    lines.append("# raw rows")
    lines += [json.dumps(r) for r in rows]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:ntable]))


if __name__ == "__main__":
    main()
