#!/usr/bin/env python3
"""Curvature's two transform paths side by side on the GPU.

For every size a child process (its own time limit; the first failure ends
the run) builds one fixed-iteration, single-level Curvature registration per
path ("curvature_dct" 0: the cosine GEMMs, 1: the fast line transforms), warms
each up, and then times them alternately, three rounds: the host clock around
of2d_estimate, which ends in a stream synchronise.  An estimate is K
iterations plus one warp, one gradient pass and one accumulation; K is chosen
per path so that those three streaming kernels stay a few percent of the
window, and the figure printed is window / K.  The child also takes the fast
path's per-pass kernel times (of2d_dct_time_passes, HIP events) and prints
them as GB/s over the 32 B per pixel a pass moves (two fp64 planes read and
written).

    python tools/curvature_bench.py [--sizes 512 1024 ...] [--rounds 3]

Sizes above --gemm-max (default 4096) run the fast path only: the GEMM path's
four dense n x n tables per level are 2 GB at 8192^2.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def images(n):
    """A smooth textured pair, the second a sub-pixel warp of the first."""
    import numpy as np
    x = np.arange(n, dtype=np.float64)[:, None]
    y = np.arange(n, dtype=np.float64)[None, :]

    def tex(dx, dy):
        return (np.sin(0.11 * (x + dx)) * np.cos(0.07 * (y + dy)) +
                0.5 * np.sin(0.031 * (x + dx) + 0.043 * (y + dy)) + 2.0)
    return tex(0.0, 0.0), tex(0.4, -0.3)


def child(n, rounds, iters_gemm, iters_fast, with_gemm):
    import numpy as np
    from opticalflow2d_amd import ImageRegistration, _lib, set_print_sink
    set_print_sink(lambda s: None)
    ref, mov = images(n)
    runs = []
    if with_gemm:
        runs.append(("gemm", 0, iters_gemm))
    runs.append(("fast", 1, iters_fast))
    regs = {}
    for name, dct, k in runs:
        r = ImageRegistration((n, n), [k], 0, 1, [0.5, 0.2], fixed_iters=1, curvature_dct=dct)
        r.set_images(ref, mov)
        r.estimate()  # warm-up: tables, code objects, first touches
        want = (n, n, dct, dct)
        assert r.curvature_paths() == [want], (r.curvature_paths(), want)
        regs[name] = (r, k)
    ms = {name: [] for name in regs}
    for _ in range(rounds):
        for name, (r, k) in regs.items():
            t0 = time.perf_counter()
            r.estimate()
            ms[name].append(1e3 * (time.perf_counter() - t0) / k)
    motions = {name: r.motion() for name, (r, k) in regs.items()}
    for r, _ in regs.values():
        r.close()
    us = np.zeros(4)
    L = _lib.lib()
    _lib.check(L.of2d_dct_time_passes(n, n, 20, us), L.of2d_gateway_last_error().decode())
    out = {"n": n, "rounds": rounds, "ms_per_iter": ms,
           "iters": {name: k for name, (r, k) in regs.items()},
           "pass_us": {"x_forward": us[0], "x_inverse": us[1], "transpose": us[2],
                       "y_forward_lines": us[3]},
           "pass_GBps": {k: 32.0 * n * n / (v * 1e-6) / 1e9 for k, v in
                         zip(("x_forward", "x_inverse", "transpose", "y_forward_lines"), us)}}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024, 2048, 4096, 8192])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--gemm-max", type=int, default=4096)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per size")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--iters-gemm", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--iters-fast", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.rounds, a.iters_gemm, a.iters_fast, a.child <= a.gemm_max)
        return 0
    print("# Curvature, one level, fixed iterations: ms per iteration (min of the rounds; all rounds)")
    for n in a.sizes:
        # GEMM cost grows as n^3: fewer iterations per window at large sizes
        kg = 40 if n <= 1024 else (16 if n <= 2048 else 8)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--rounds",
               str(a.rounds), "--gemm-max", str(a.gemm_max), "--iters-gemm", str(kg),
               "--iters-fast", "60"]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"{n}^2: no result within {a.timeout} s; stopping")
            return 1
        res = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(f"{n}^2: child failed (exit {p.returncode}); stopping\n{p.stdout}\n{p.stderr}")
            return 1
        r = json.loads(res[0][7:])
        f = r["ms_per_iter"]["fast"]
        line = f"{n}^2: fast {min(f):.3f} ms/iter {['%.3f' % v for v in f]}"
        if "gemm" in r["ms_per_iter"]:
            g = r["ms_per_iter"]["gemm"]
            line += (f" | gemm {min(g):.3f} ms/iter {['%.3f' % v for v in g]}"
                     f" | gemm/fast {min(g) / min(f):.1f}x")
        else:
            line += " | gemm not run (above --gemm-max)"
        print(line)
        print("    fast passes: " + ", ".join(
            f"{k} {r['pass_us'][k]:.1f} us = {r['pass_GBps'][k]:.0f} GB/s" for k in r["pass_us"]))
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
