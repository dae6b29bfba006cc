#!/usr/bin/env python3
"""The deformation-analysis kernels at benchmark size on the GPU.

A child process (its own time limit) calls of2d_analysis_time_kernels: HIP
events around `--launches` back-to-back launches after one untimed launch, of
the Jacobian map with its statistics (the map launch and its one-block
reduction) and of one update of the inverse at an iterate near the fixed point
of a smooth 3-pixel field, `--rounds` times each.  The rates printed are the
algorithmic bytes over the launch time: the Jacobian reads the motion (8 B/px)
and writes the map (4 B/px); an update of the inverse reads v (8 B/px), gathers
u (counted once: 8 B/px; the four taps of neighbouring pixels overlap in cache)
and writes v (8 B/px).

    python tools/analysis_bench.py [--size 4096] [--launches 200] [--rounds 3]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BYTES_PER_PX = {"jacobian": 8 + 4, "invert_update": 8 + 8 + 8}


def child(n, launches, rounds):
    import numpy as np
    from opticalflow2d_amd import _lib
    from opticalflow2d_amd._lib import check
    L = _lib.lib()
    us = np.zeros(2, np.float64)
    out = {k: [] for k in BYTES_PER_PX}
    for _ in range(rounds):
        check(L.of2d_analysis_time_kernels(n, n, launches, us),
              L.of2d_gateway_last_error().decode())
        out["jacobian"].append(float(us[0]))
        out["invert_update"].append(float(us[1]))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds for the child")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.size, a.launches, a.rounds)
        return 0
    n = a.size
    print(f"# deformation analysis {n}^2: us per launch over {a.launches} back-to-back launches "
          "(min of the rounds; all rounds), algorithmic bytes / time")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--size", str(n), "--launches",
           str(a.launches), "--rounds", str(a.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {a.timeout} s")
        return 1
    res = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not res:
        print(f"child failed (exit {p.returncode})\n{p.stdout}\n{p.stderr}")
        return 1
    r = json.loads(res[0][7:])
    for name, bpp in BYTES_PER_PX.items():
        t = min(r[name])
        print(f"{name:14s} {t:8.1f} us {['%.1f' % v for v in r[name]]} | {bpp} B/px -> "
              f"{bpp * n * n / (t * 1e-6) / 1e12:.2f} TB/s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
