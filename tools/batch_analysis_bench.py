#!/usr/bin/env python3
"""BatchRegistration's analysis calls against the per-pair sequence.

Seconds per pair of `jacobian()`, `inverse_motion()` and `quality()` on a
registered batch of B pairs, against what a batch user had to do before them,
with a baseline build of the library (the parent commit's: --baseline-lib;
never the code under test):

  jacobian  motion(), then field.jacobian per pair
  inverse   motion(), then field.invert per pair
  quality   warp(Imov), then field.similarity(Iref, Imov) and
            field.similarity(Iref, warped) per pair

Both sides return host arrays (the maps, the inverse fields, the statistics).
The batch is registered once per size and B (Horn-Schunck, 50 fixed
iterations: a smooth sub-pixel motion whose inverse converges in a few
updates); the timed windows hold the analysis only.  The method is
tools/batch_bench.py's: one child process per side and round, sides
interleaved; within a child every figure is the minimum over the repetitions
of a timed window (after a warm-up call; 2 to 20, 0.5 s); the table holds the
median of the rounds' minima.

Writes profiles/batch_analysis_bench.log.  Not run by any test.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.batch_bench import timed  # noqa: E402

NITER, ALPHA = 50, 0.1
CALLS = ("jacobian", "inverse", "quality")


def pairs(n, count):
    """`count` textured pairs cycling through 8 sub-pixel shifts."""
    import numpy as np
    from opticalflow2d_amd import synthetic as S
    base = [S.texture_pair(n, seed=5, sigma=3.0, shift=(0.3 + 0.15 * k, -0.2 - 0.1 * k))
            for k in range(8)]
    refs = np.stack([base[k % 8][0] for k in range(count)])
    movs = np.stack([base[k % 8][1] for k in range(count)])
    return refs, movs


def child(side, sizes, batches):
    import ctypes
    import numpy as np
    from opticalflow2d_amd import _lib
    if side == "sequence":
        # bind what the baseline library exports (the parent's has no batch analysis)
        raw = ctypes.CDLL(_lib.LIB_PATH)
        for table in (_lib.SIGNATURES, _lib.PRODUCT_SIGNATURES, _lib.PRIM_SIGNATURES):
            for name in [k for k in table if not hasattr(raw, k)]:
                del table[name]
    from opticalflow2d_amd import BatchRegistration, field, set_print_sink
    set_print_sink(lambda s: None)
    F = np.float32

    def fields32(m):  # [B, dimx, dimy, 2] -> float32 [B, dimy, dimx, 2]
        return np.ascontiguousarray(m.transpose(0, 2, 1, 3), dtype=F)

    def images32(a):  # [B, dimx, dimy] -> float32 [B, dimy, dimx]
        return np.ascontiguousarray(a.transpose(0, 2, 1), dtype=F)

    for n in sizes:
        for B in batches:
            refs, movs = pairs(n, B)
            with BatchRegistration(B, (n, n), [NITER], 0, ALPHA, device=0, fixed_iters=1) as b:
                b.register(refs, movs)
                if side == "batch":
                    run = {"jacobian": lambda: b.jacobian(),
                           "inverse": lambda: b.inverse_motion(),
                           "quality": lambda: b.quality(refs, movs)}
                    its = [i["iterations"] for i in b.inverse_motion()[1]]
                else:
                    its = []

                    def seq_jacobian():
                        u = fields32(b.motion())
                        return [field.jacobian(u[k]) for k in range(B)]

                    def seq_inverse():
                        u = fields32(b.motion())
                        out = [field.invert(u[k]) for k in range(B)]
                        its[:] = [o[1]["iterations"] for o in out]
                        return out

                    def seq_quality():
                        w = images32(b.warp(movs))
                        r, m = images32(refs), images32(movs)
                        return [field.similarity(r[k], m[k]) + field.similarity(r[k], w[k])
                                for k in range(B)]
                    run = {"jacobian": seq_jacobian, "inverse": seq_inverse,
                           "quality": seq_quality}
                for call in CALLS:
                    t = timed(run[call])
                    print(json.dumps({"side": side, "n": n, "B": B, "call": call,
                                      "s_per_pair": t / B,
                                      "mean_inverse_iters": sum(its) / max(len(its), 1)}),
                          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--baseline-lib", help="libof2d.so of the parent commit (the sequence's side)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64, 256, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_analysis_bench.log"))
    ap.add_argument("--child", choices=["batch", "sequence"])
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.sizes, a.batches)
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

    def med(side, n, B, call, key="s_per_pair"):
        return statistics.median(r[key] for r in rows if r["side"] == side and r["n"] == n and
                                 r["B"] == B and r["call"] == call)

    lines = ["# tools/batch_analysis_bench.py: the batch's analysis calls against motion() / "
             "warp() and the one-pair entries per pair",
             f"# rounds {a.rounds}, sides interleaved per round; every figure: the minimum over a "
             "round's repetitions (2 to 20, 0.5 s), then the median of the rounds",
             f"# HS, niter {NITER} fixed, nscales 0, alpha {ALPHA}; both sides return host arrays; "
             "baseline library "
             + os.path.basename(os.path.dirname(os.path.abspath(a.baseline_lib))),
             "# ratio = sequence / batch (above 1: the batch call is faster)",
             "size     B  call      batch s/pair  sequence s/pair   ratio  inverse iters b/s"]
    for n in a.sizes:
        for B in a.batches:
            for call in CALLS:
                bt, seq = med("batch", n, B, call), med("sequence", n, B, call)
                lines.append(f"{n:4d} {B:5d}  {call:8}  {bt:12.3e}  {seq:15.3e}  {seq / bt:6.2f}  "
                             f"{med('batch', n, B, call, 'mean_inverse_iters'):5.1f}/"
                             f"{med('sequence', n, B, 'inverse', 'mean_inverse_iters'):<5.1f}")
    nhead = len(lines)
    lines.append("# raw rows")
    lines += [json.dumps(r) for r in rows]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:nhead]))


if __name__ == "__main__":
    main()
