#!/usr/bin/env python3
"""Thirion's Demons with its two smoothings side by side on the GPU.

For every case a child process (its own time limit; the first failure ends
the run) builds one fixed-iteration, single-level Thirion registration per
path ("demons_separable" 0: the reference's direct kw x kw convolution, 1: the
row + column passes on the interior pixels), warms each up, and then times
them alternately, three rounds: the host clock around of2d_estimate, which
ends in a stream synchronise.  An estimate is K iterations plus one warp and
one accumulation, a few percent of the window at K = 20; the figure printed
is window / K, and Gpx-it/s is pixels x iterations per second.  The child also
prints the largest |difference| between the two paths' motion fields after
their first estimate (K iterations each from zero motion on the same images;
a handle's motion carries over into its later estimates, which the timed
rounds are).

Case 1 is BASELINE config 3 (4096^2, kw 5, both sigmas 2); case 2 the same
images with kw 9, 13 and 15 and both sigmas (kw - 1) / 6, the widths a user
who wants sigma = 1.3 .. 2.3 px with the usual 6 sigma + 1 support sets.

    python tools/demons_bench.py [--size 4096] [--widths 9 13 15] [--rounds 3]
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


def child(n, kw, sigma, iters, rounds):
    import numpy as np
    from opticalflow2d_amd import ImageRegistration, set_print_sink
    from opticalflow2d_amd import synthetic as S
    set_print_sink(lambda s: None)
    ref, mov = S.procedural_pair(n, 0, n)  # bench_configs.py config 3's pair
    params = [1.0, 0.25, sigma, sigma, kw, 0]
    regs = {}
    for name, sep in (("direct", 0), ("separable", 1)):
        r = ImageRegistration((n, n), [iters], 0, 3, params, fixed_iters=1, demons_separable=sep)
        r.set_images(ref, mov)
        r.estimate()  # warm-up: code objects, first touches
        assert r.demons_paths() == [(n, n, kw, sep)], r.demons_paths()
        regs[name] = r
    m = {name: r.motion() for name, r in regs.items()}
    ms = {name: [] for name in regs}
    for _ in range(rounds):
        for name, r in regs.items():
            t0 = time.perf_counter()
            r.estimate()
            ms[name].append(1e3 * (time.perf_counter() - t0) / iters)
    for r in regs.values():
        r.close()
    out = {"n": n, "kw": kw, "sigma": sigma, "iters": iters, "ms_per_iter": ms,
           "max_abs_du": float(np.abs(m["direct"] - m["separable"]).max()),
           "max_abs_u": float(np.abs(m["direct"]).max())}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--widths", type=int, nargs="+", default=[9, 13, 15])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--sigma", type=float, default=0.0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.size, a.child, a.sigma, a.iters, a.rounds)
        return 0
    n = a.size
    print(f"# Thirion's Demons {n}^2, one level, {a.iters} fixed iterations per estimate: "
          "ms per iteration (min of the rounds; all rounds)")
    cases = [(5, 2.0)] + [(kw, (kw - 1) / 6.0) for kw in a.widths]
    for kw, sigma in cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(kw), "--sigma",
               repr(sigma), "--size", str(n), "--iters", str(a.iters), "--rounds", str(a.rounds)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"kw {kw}: no result within {a.timeout} s; stopping")
            return 1
        res = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(f"kw {kw}: child failed (exit {p.returncode}); stopping\n{p.stdout}\n{p.stderr}")
            return 1
        r = json.loads(res[0][7:])
        d, s = r["ms_per_iter"]["direct"], r["ms_per_iter"]["separable"]
        gpx = lambda v: n * n / (v * 1e-3) / 1e9  # noqa: E731
        print(f"kw {kw:2d} sigma {sigma:.3f}: direct {min(d):.3f} ms/iter = {gpx(min(d)):.2f} "
              f"Gpx-it/s {['%.3f' % v for v in d]} | separable {min(s):.3f} ms/iter = "
              f"{gpx(min(s)):.2f} Gpx-it/s {['%.3f' % v for v in s]} | direct/separable "
              f"{min(d) / min(s):.2f}x | max |du| after {a.iters} iterations {r['max_abs_du']:.3e} px "
              f"(max |u| {r['max_abs_u']:.3f})")
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
