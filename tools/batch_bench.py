#!/usr/bin/env python3
"""BatchRegistration against a sequence of ImageRegistration calls.

Seconds per pair for B pairs in one BatchRegistration call, against the
EXISTING one-pair path: one ImageRegistration object registering pair after
pair with the same options, from a baseline build of the library (the parent
commit's: --baseline-lib; never the code under test).  Two cases per size:

  a  200 fixed iterations, nscales 0 (fixed_iters=1 on both sides);
  b  config 1's parameters (niter 200, nscales 0, alpha 0.1) with convergence
     on; the sequence runs with logger_fp64=1, the batch's Logger semantics.

The driver alternates one child process per side and round (each loads one
library), so the two sides are interleaved on one box.  Within a child every
figure is the minimum over the repetitions of a timed window (after a warm-up
call; at least 2, up to 20 or 0.5 s); the table holds the median of the rounds'
minima.  The sequence runs B registrations one after another for every B of
the table.  Also recorded: the loop kernel's device time per iteration (HIP
events, of2d_batch_info) and the bytes that implies at 28 B per pixel and
iteration (u in 8, dI 8, It 4, u' out 8).

Writes profiles/batch_bench.log.  Not run by any test.
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
SHIFTS = [(2, 1), (1, 2), (3, 1), (1, 1), (2, 2), (3, 2), (1, 3), (2, 3)]


def pairs(n, count):
    """`count` config-1 pairs (translated squares) cycling through 8 shifts."""
    import numpy as np
    from opticalflow2d_amd import synthetic as S
    base = [S.translated_square(n, shift=sh) for sh in SHIFTS]
    refs = np.stack([base[k % 8][0] for k in range(count)])
    movs = np.stack([base[k % 8][1] for k in range(count)])
    return refs, movs


def timed(fn, min_s=0.5, max_reps=20):
    fn()  # warm-up: code objects, allocations, every shape of the window
    ts = []
    while len(ts) < max_reps and (len(ts) < 2 or sum(ts) < min_s):
        t0 = time.perf_counter()
        fn()  # ends in a device synchronise (the library's entry points do)
        ts.append(time.perf_counter() - t0)
    return min(ts)


def child_batch(sizes, batches):
    from opticalflow2d_amd import BatchRegistration, _lib, set_print_sink
    set_print_sink(lambda s: None)
    L = _lib.lib()
    out = []
    for n in sizes:
        for case in "ab":
            for B in batches:
                refs, movs = pairs(n, B)
                opt = {"fixed_iters": 1} if case == "a" else {}
                with BatchRegistration(B, (n, n), [NITER], 0, ALPHA, device=0, **opt) as b:
                    t_reg = timed(lambda: b.register(refs, movs))
                    t_est = timed(lambda: b._chk(L.of2d_batch_estimate(b._h)))
                    it = b.iterations()
                    info = b.info()
                total_it = int(it.sum())
                us_it = info["loop_us"] / max(int(it.max()), 1)  # the longest pair's loop
                out.append({"side": "batch", "n": n, "case": case, "B": B,
                            "s_per_pair_register": t_reg / B, "s_per_pair_estimate": t_est / B,
                            "mean_iters": total_it / B, "loop_us": info["loop_us"],
                            "loop_us_per_iter": us_it,
                            "loop_GBps": 28.0 * n * n * total_it / max(info["loop_us"], 1) / 1e3,
                            "launches": info["launches"]})
                print(json.dumps(out[-1]), flush=True)


def child_sequence(sizes, batches):
    import ctypes
    from opticalflow2d_amd import ImageRegistration, _lib, set_print_sink
    # bind what the baseline library exports (the parent's has no batch entries)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in [k for k in _lib.SIGNATURES if not hasattr(raw, k)]:
        del _lib.SIGNATURES[name]
    set_print_sink(lambda s: None)
    for n in sizes:
        refs, movs = pairs(n, 8)  # pair k of the batch's inputs is pair k % 8
        for case in "ab":
            opt = {"fixed_iters": 1} if case == "a" else {"logger_fp64": 1}
            with ImageRegistration((n, n), [NITER], 0, 0, [ALPHA], device=0, **opt) as r:
                for B in batches:
                    iters = []

                    def run():
                        iters.clear()
                        for k in range(B):
                            r.register(refs[k % 8], movs[k % 8])
                            iters.extend(r.iterations())
                    t = timed(run)
                    print(json.dumps({"side": "sequence", "n": n, "case": case, "B": B,
                                      "s_per_pair_register": t / B,
                                      "mean_iters": sum(iters) / max(len(iters), 1)}),
                          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--baseline-lib", help="libof2d.so of the parent commit (the sequence's side)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 128])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 64, 256, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_bench.log"))
    ap.add_argument("--child", choices=["batch", "sequence"])
    a = ap.parse_args()
    if a.child == "batch":
        return child_batch(a.sizes, a.batches)
    if a.child == "sequence":
        return child_sequence(a.sizes, a.batches)
    if not a.baseline_lib or not os.path.exists(a.baseline_lib):
        sys.exit("--baseline-lib: the parent commit's libof2d.so is required "
                 "(the baseline is never the code under test)")
    rows = []
    common = ["--sizes", *map(str, a.sizes), "--batches", *map(str, a.batches)]
    for rnd in range(a.rounds):
        for side in ("batch", "sequence"):
            env = dict(os.environ)
            if side == "sequence":
                env["OF2D_LIB_PATH"] = os.path.abspath(a.baseline_lib)
            else:
                env.pop("OF2D_LIB_PATH", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side,
                                *common], env=env, stdout=subprocess.PIPE, text=True, check=True,
                               timeout=900)  # a failed or hung child ends the run
            print(f"round {rnd}: {side} done", file=sys.stderr, flush=True)
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    rows.append(dict(json.loads(line), round=rnd))

    def med(side, n, case, key, B=None):
        v = [r[key] for r in rows if r["side"] == side and r["n"] == n and r["case"] == case
             and (B is None or r["B"] == B)]
        return statistics.median(v)

    lines = ["# tools/batch_bench.py: BatchRegistration against ImageRegistration in sequence",
             f"# rounds {a.rounds}, sides interleaved per round; every figure: the minimum over a "
             "round's repetitions (2 to 20, 0.5 s), then the median of the rounds",
             f"# niter {NITER}, nscales 0, alpha {ALPHA}; sequence: B registrations one after "
             "another on one object, baseline library "
             + os.path.basename(os.path.dirname(os.path.abspath(a.baseline_lib))),
             "# case a: fixed_iters; case b: convergence on (sequence with logger_fp64=1)",
             "# s/pair: register() = upload + estimate; est: estimate alone",
             "size case     B  batch s/pair  (est s/pair)  sequence s/pair   ratio  "
             "iters b/s   loop us/iter  loop GB/s"]
    for n in a.sizes:
        for case in "ab":
            for B in a.batches:
                seq = med("sequence", n, case, "s_per_pair_register", B)
                bt = med("batch", n, case, "s_per_pair_register", B)
                lines.append(
                    f"{n:4d} {case:>4} {B:5d}  {bt:12.3e}  ({med('batch', n, case, 's_per_pair_estimate', B):10.3e})"
                    f"  {seq:15.3e}  {seq / bt:6.1f}  "
                    f"{med('batch', n, case, 'mean_iters', B):5.0f}/{med('sequence', n, case, 'mean_iters', B):<5.0f}"
                    f"  {med('batch', n, case, 'loop_us_per_iter', B):10.2f}  "
                    f"{med('batch', n, case, 'loop_GBps', B):9.1f}")
    lines.append("# raw rows")
    lines += [json.dumps(r) for r in rows]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:6 + 2 * len(a.sizes) * len(a.batches)]))


if __name__ == "__main__":
    main()
