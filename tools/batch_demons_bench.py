#!/usr/bin/env python3
"""BatchRegistration(reg=3) against a sequence of one-pair Demons calls.

Seconds per pair for B pairs of Thirion's Demons in one BatchRegistration
call, against the EXISTING one-pair path: one ImageRegistration object
registering pair after pair with the same parameters, from a baseline build of
the library (the parent commit's: --baseline-lib; never the code under test).
One case: 100 fixed iterations, nscales 0, parameters [1, 0.25, 1.5, 2.5, kw 5,
Composition], textured pairs (a flat image has a zero Demons denominator).

The method is tools/batch_bench.py's: the driver alternates one child process
per side and round (each loads one library), so the two sides are interleaved
on one box; within a child every figure is the minimum over the repetitions of
a timed window (after a warm-up call; at least 2, up to 20 or 0.5 s); the table
holds the median of the rounds' minima.  Also recorded: the loop kernel's
device time per iteration (HIP events, of2d_batch_info) and the bytes that
implies at 72 B per pixel and iteration, every array of a stage counted once
(warp: u 8, Iaux 4, W out 4; correction: W 4, Iref 4, c out 8; smoothing and
update: c 8, u 8, mid out 8; smoothing: mid 8, u' out 8).

--diffeomorphic: the batch runs with the option
"diffeomorphic" and the sequence is one-pair Diffeomorphic Demons (reg 4), with
parameters whose squarings are live, [1, 2, 1, 1, kw 5]: |c| reaches 1 and an
iteration takes 0, 1 or 2 squarings (the count is the pair's own in the batch;
the one-pair path enqueues its bound every iteration).  The bytes per pixel and
iteration are then a lower bound: a squaring adds 16 (one field in, one out),
the scaling 16, and the split of stages 3 and 4 another 16.

Writes profiles/batch_demons_bench.log, or profiles/batch_diffeo_bench.log with
--diffeomorphic.  Not run by any test.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_bench import timed  # noqa: E402

NITER = 100
PARAMS = [1.0, 0.25, 1.5, 2.5, 5, 0]
DIFFEO_PARAMS = [1.0, 2.0, 1.0, 1.0, 5, 0]  # the one-pair reg 4 takes the first five
BYTES_PX_ITER = 72.0
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


def child_batch(sizes, batches, diffeo=False):
    from opticalflow2d_amd import BatchRegistration, _lib, set_print_sink
    set_print_sink(lambda s: None)
    L = _lib.lib()
    for n in sizes:
        for B in batches:
            refs, movs = pairs(n, B)
            opt = {"diffeomorphic": 1} if diffeo else {}
            with BatchRegistration(B, (n, n), [NITER], 0, DIFFEO_PARAMS if diffeo else PARAMS,
                                   reg=3, device=0, fixed_iters=1, **opt) as b:
                t_reg = timed(lambda: b.register(refs, movs))
                t_est = timed(lambda: b._chk(L.of2d_batch_estimate(b._h)))
                it = b.iterations()
                info = b.info()
                failed = int(b.status().astype(bool).sum())
            total_it = int(it.sum())
            row = {"side": "batch", "n": n, "B": B, "s_per_pair_register": t_reg / B,
                   "s_per_pair_estimate": t_est / B, "mean_iters": total_it / B,
                   "loop_us": info["loop_us"],
                   "loop_us_per_iter": info["loop_us"] / max(int(it.max()), 1),
                   "loop_GBps": BYTES_PX_ITER * n * n * total_it / max(info["loop_us"], 1) / 1e3,
                   "launches": info["launches"], "failed_pairs": failed}
            print(json.dumps(row), flush=True)


def child_sequence(sizes, batches, diffeo=False):
    import ctypes
    from opticalflow2d_amd import ImageRegistration, _lib, set_print_sink
    # bind what the baseline library exports
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in [k for k in _lib.SIGNATURES if not hasattr(raw, k)]:
        del _lib.SIGNATURES[name]
    set_print_sink(lambda s: None)
    for n in sizes:
        refs, movs = pairs(n, 8)  # pair k of the batch's inputs is pair k % 8
        reg, params = (4, DIFFEO_PARAMS[:5]) if diffeo else (3, PARAMS)
        with ImageRegistration((n, n), [NITER], 0, reg, params, device=0, fixed_iters=1) as r:
            for B in batches:
                iters = []

                def run():
                    iters.clear()
                    for k in range(B):
                        r.register(refs[k % 8], movs[k % 8])
                        iters.extend(r.iterations())
                t = timed(run)
                print(json.dumps({"side": "sequence", "n": n, "B": B,
                                  "s_per_pair_register": t / B,
                                  "mean_iters": sum(iters) / max(len(iters), 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--baseline-lib", help="libof2d.so of the parent commit (the sequence's side)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--diffeomorphic", action="store_true",
                    help="the batch's option against one-pair Diffeomorphic Demons (reg 4)")
    ap.add_argument("--out", help="default: profiles/batch_demons_bench.log, or "
                    "profiles/batch_diffeo_bench.log with --diffeomorphic")
    ap.add_argument("--child", choices=["batch", "sequence"])
    a = ap.parse_args()
    if not a.out:
        a.out = os.path.join(ROOT, "profiles", "batch_diffeo_bench.log" if a.diffeomorphic
                             else "batch_demons_bench.log")
    if a.child == "batch":
        return child_batch(a.sizes, a.batches, a.diffeomorphic)
    if a.child == "sequence":
        return child_sequence(a.sizes, a.batches, a.diffeomorphic)
    if not a.baseline_lib or not os.path.exists(a.baseline_lib):
        sys.exit("--baseline-lib: the parent commit's libof2d.so is required "
                 "(the baseline is never the code under test)")
    rows = []
    common = ["--sizes", *map(str, a.sizes), "--batches", *map(str, a.batches)]
    if a.diffeomorphic:
        common.append("--diffeomorphic")
    for rnd in range(a.rounds):
        for side in ("batch", "sequence"):
            env = dict(os.environ)
            if side == "sequence":
                env["OF2D_LIB_PATH"] = os.path.abspath(a.baseline_lib)
            else:
                env.pop("OF2D_LIB_PATH", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side,
                                *common], env=env, stdout=subprocess.PIPE, text=True, check=True,
                               timeout=600)  # a failed or hung child ends the run
            print(f"round {rnd}: {side} done", file=sys.stderr, flush=True)
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    rows.append(dict(json.loads(line), round=rnd))

    def med(side, n, key, B):
        return statistics.median(r[key] for r in rows
                                 if r["side"] == side and r["n"] == n and r["B"] == B)

    what = ("BatchRegistration(reg=3, diffeomorphic=1) against ImageRegistration "
            "(Diffeomorphic Demons, reg 4)" if a.diffeomorphic else
            "BatchRegistration(reg=3) against ImageRegistration (Thirion's Demons)")
    shown = DIFFEO_PARAMS if a.diffeomorphic else PARAMS
    lines = [f"# tools/batch_demons_bench.py: {what} in sequence",
             f"# rounds {a.rounds}, sides interleaved per round; every figure: the minimum over a "
             "round's repetitions (2 to 20, 0.5 s), then the median of the rounds",
             f"# niter {NITER} fixed, nscales 0, params {shown}; sequence: B registrations one "
             "after another on one object, baseline library "
             + os.path.basename(os.path.abspath(a.baseline_lib)),
             "# s/pair: register() = upload + estimate; est: estimate alone; ratio: sequence / "
             f"batch register(); loop GB/s at {BYTES_PX_ITER:.0f} B per pixel and iteration",
             "size     B  batch s/pair  (est s/pair)  sequence s/pair   ratio  "
             "loop us/iter  loop GB/s  failed"]
    for n in a.sizes:
        for B in a.batches:
            seq = med("sequence", n, "s_per_pair_register", B)
            bt = med("batch", n, "s_per_pair_register", B)
            lines.append(
                f"{n:4d} {B:5d}  {bt:12.3e}  ({med('batch', n, 's_per_pair_estimate', B):10.3e})"
                f"  {seq:15.3e}  {seq / bt:6.2f}  "
                f"{med('batch', n, 'loop_us_per_iter', B):12.2f}  "
                f"{med('batch', n, 'loop_GBps', B):9.1f}  "
                f"{int(med('batch', n, 'failed_pairs', B)):6d}")
    ntable = len(lines)
    lines.append("# raw rows")
    lines += [json.dumps(r) for r in rows]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:ntable]))


if __name__ == "__main__":
    main()
