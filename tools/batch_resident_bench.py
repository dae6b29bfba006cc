#!/usr/bin/env python3
"""BatchRegistration with resident=1 against resident=0.

The same handle's estimate with the Horn-Schunck loop's iterate on the CU
(option "resident") against the global-memory loop, alternating in one process
on one box: for every row the two sides are timed one after the other within a
round, and the rounds follow one another, so both sides see the same machine
state.  Never a figure against an earlier run of the code.

Workload: case a of tools/batch_bench.py (200 fixed iterations, nscales 0,
alpha 0.1) at 64 x 64 and 128 x 128 for B = 1, 16, 64, 256, 1024, and one
pyramid run: 256 x 256, nscales 2, B = 256 (levels 128 and 64 resident, level 0
in global memory).

Every figure is the minimum over a round's repetitions of the timed estimate
(after a warm-up call; at least 2, up to 20 or 0.3 s), then the median of the
rounds.  Per row: the loop kernels' device time per iteration (HIP events,
of2d_batch_info), seconds per pair for the estimate, and the ratio
resident=0 / resident=1 of each (above 1: resident is faster).  The motion of
the two sides is compared once per row (np.array_equal).

Writes profiles/batch_resident_bench.log.  Not run by any test.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NITER, ALPHA = 200, 0.1
SHIFTS = [(2, 1), (1, 2), (3, 1), (1, 1), (2, 2), (3, 2), (1, 3), (2, 3)]


def pairs(n, count):
    """`count` config-1 pairs (translated squares) cycling through 8 shifts."""
    import numpy as np
    from opticalflow2d_amd import synthetic as S
    base = [S.translated_square(n, shift=sh) for sh in SHIFTS]
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
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 64, 256, 1024])
    ap.add_argument("--no-pyramid", action="store_true", help="leave the 256 x 256 run out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_resident_bench.log"))
    a = ap.parse_args()

    import numpy as np
    from opticalflow2d_amd import BatchRegistration, _lib, set_print_sink
    set_print_sink(lambda s: None)
    L = _lib.lib()

    configs = [(n, B, [NITER], 0) for n in a.sizes for B in a.batches]
    if not a.no_pyramid:
        configs.append((256, 256, [NITER] * 3, 2))
    rows, same, placement = [], {}, {}
    for n, B, niter, nscales in configs:
        refs, movs = pairs(n, B)
        total_it = sum(niter)
        with BatchRegistration(B, (n, n), niter, nscales, ALPHA, device=0, fixed_iters=1) as b:
            b.register(refs, movs)  # the upload, once: the sides time the estimate alone
            motion = {}
            for rnd in range(a.rounds):
                for resident in (0, 1):
                    b.set_option("resident", resident)
                    t = timed(lambda: b._chk(L.of2d_batch_estimate(b._h)))
                    info = b.info()
                    rows.append({"n": n, "B": B, "nscales": nscales, "resident": resident,
                                 "round": rnd, "s_per_pair_estimate": t / B,
                                 "loop_us_per_iter": info["loop_us"] / total_it,
                                 "placement": info["placement"]})
                    print(json.dumps(rows[-1]), flush=True)
                    if rnd == 0:
                        motion[resident] = b.motion()
                        placement[n, B, nscales, resident] = info["placement"]
            same[n, B, nscales] = bool(np.array_equal(motion[0], motion[1]))

    def med(n, B, nscales, resident, key):
        return statistics.median(r[key] for r in rows
                                 if (r["n"], r["B"], r["nscales"], r["resident"]) ==
                                 (n, B, nscales, resident))

    lines = ["# tools/batch_resident_bench.py: BatchRegistration resident=1 against resident=0",
             f"# rounds {a.rounds}, the two sides alternating in one process; every figure: the "
             "minimum over a round's repetitions (2 to 20, 0.3 s), then the median of the rounds",
             f"# niter {NITER} per level, fixed_iters, alpha {ALPHA}; the estimate alone (no upload)",
             "# ratio: resident=0 / resident=1 (above 1: resident is faster)",
             "size nscales     B  placement   loop us/iter r=0       r=1   ratio   "
             "est s/pair r=0         r=1   ratio  same bits"]
    for n, B, niter, nscales in configs:
        l0, l1 = (med(n, B, nscales, r, "loop_us_per_iter") for r in (0, 1))
        e0, e1 = (med(n, B, nscales, r, "s_per_pair_estimate") for r in (0, 1))
        lines.append(f"{n:4d} {nscales:7d} {B:5d}  {str(placement[n, B, nscales, 1]):>9}  "
                     f"{l0:16.2f} {l1:9.2f}  {l0 / max(l1, 1e-9):6.2f}   "
                     f"{e0:14.3e}  {e1:10.3e}  {e0 / e1:6.2f}  {same[n, B, nscales]}")
    ntable = len(lines)
    lines.append("# raw rows")
    lines += [json.dumps(r) for r in rows]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:ntable]))


if __name__ == "__main__":
    main()
