#!/usr/bin/env python3
"""BatchRegistration fed torch CUDA tensors against host arrays.

Seconds per pair of register() (images in + estimate) with host float64 arrays
(the existing path: its code is the parent commit's, unchanged) and with
float32 CUDA tensors [B, n, n] (contiguous, so y fastest: layout (b)), and of
motion() against motion_device().  200 fixed iterations, nscales 0, alpha 0.1.
A device-side window ends with a synchronise of the caller's stream.

One process; the sides alternate inside every round.  Every figure is the
minimum over the repetitions of a timed window (after a warm-up call; at least
2, up to 20 or 0.5 s); the table holds the median of the rounds' minima.

Also: the pack (both stacks of set_images) and the motion unpack alone, between
two events on the caller's stream, as GB/s against their own bytes (float32
read + float32 written), for x fastest (layout (a)) and y fastest (layout
(b)).  The events also see the two cross-stream waits of the stream contract.

Writes profiles/device_io_bench.log.  Not run by any test; nothing here is a
threshold.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NITER, ALPHA = 200, 0.1


def timed(fn, min_s=0.5, max_reps=20):
    fn()  # warm-up: code objects, allocations
    ts = []
    while len(ts) < max_reps and (len(ts) < 2 or sum(ts) < min_s):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def event_ms(torch, fn, reps=10):
    """The shortest of `reps` windows between two events on the current stream."""
    best = float("inf")
    for _ in range(reps + 1):  # the first is the warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def one_round(torch, sizes, batches):
    from batch_bench import pairs
    from opticalflow2d_amd import BatchRegistration, _device, _lib
    L = _lib.lib()
    rows = []
    for n in sizes:
        for B in batches:
            refs, movs = pairs(n, B)
            tref = torch.from_numpy(refs.astype("float32")).to("cuda")
            tmov = torch.from_numpy(movs.astype("float32")).to("cuda")
            with BatchRegistration(B, (n, n), [NITER], 0, ALPHA, device=0, fixed_iters=1) as b:
                def dev_register():
                    b.register(tref, tmov)
                    torch.cuda.current_stream().synchronize()

                out = torch.empty((B, n, n, 2), dtype=torch.float32, device="cuda")

                def dev_motion():
                    b.motion_device(out=out)
                    torch.cuda.current_stream().synchronize()

                row = {"n": n, "B": B,
                       "host_register": timed(lambda: b.register(refs, movs)) / B,
                       "device_register": timed(dev_register) / B,
                       "estimate": timed(lambda: b._chk(L.of2d_batch_estimate(b._h))) / B,
                       "host_motion": timed(b.motion) / B,
                       "device_motion": timed(dev_motion) / B}
                # the launches alone, both layouts; bytes: float32 in + float32 out
                px = B * n * n
                for name, tr, tm, to in [
                        ("b", tref, tmov, out),
                        ("a", tref.swapaxes(1, 2), tmov.swapaxes(1, 2),
                         out.view(B, 2, n, n).permute(0, 3, 2, 1))]:
                    st = _device.stream_of(tm)
                    r = _device.darray(tr, (B, n, n), (0, 1, 2), "Iref")
                    m = _device.darray(tm, (B, n, n), (0, 1, 2), "Imov")
                    ms = event_ms(torch, lambda: b._chk(L.of2d_batch_set_images_device(
                        b._h, C.byref(r), 0, C.byref(m), st)))
                    row[f"pack_{name}_GBps"] = 2 * px * 8 / ms / 1e6
                    ms = event_ms(torch, lambda: b.motion_device(out=to))
                    row[f"unpack_{name}_GBps"] = px * 16 / ms / 1e6
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 128])
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64, 256, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_io_bench.log"))
    a = ap.parse_args()
    import torch
    from opticalflow2d_amd import set_print_sink
    set_print_sink(lambda s: None)
    rows = []
    for rnd in range(a.rounds):
        rows += [dict(r, round=rnd) for r in one_round(torch, a.sizes, a.batches)]

    def med(n, B, key):
        return statistics.median(r[key] for r in rows if r["n"] == n and r["B"] == B)

    lines = ["# tools/device_io_bench.py: BatchRegistration, float32 CUDA tensors against host "
             "float64 arrays",
             f"# rounds {a.rounds}, sides alternating in every round; every figure: the minimum "
             "over a round's repetitions (2 to 20, 0.5 s), then the median of the rounds",
             f"# niter {NITER} fixed, nscales 0, alpha {ALPHA}; s/pair; register = images in + "
             "estimate; est: estimate alone",
             "# pack / unpack GB/s: float32 in + float32 out of the launches between two events "
             "on the caller's stream; (a) x fastest, (b) y fastest (contiguous [B, n, n(, 2)])",
             "size     B  host register  device register  ratio  (est)       host motion  "
             "device motion  ratio   pack a   pack b  unpack a  unpack b"]
    for n in a.sizes:
        for B in a.batches:
            hr, dr = med(n, B, "host_register"), med(n, B, "device_register")
            hm, dm = med(n, B, "host_motion"), med(n, B, "device_motion")
            lines.append(
                f"{n:4d} {B:5d}  {hr:13.3e}  {dr:15.3e}  {hr / dr:5.2f}  ({med(n, B, 'estimate'):9.3e})"
                f"  {hm:11.3e}  {dm:13.3e}  {hm / dm:5.1f}  {med(n, B, 'pack_a_GBps'):7.0f}  "
                f"{med(n, B, 'pack_b_GBps'):7.0f}  {med(n, B, 'unpack_a_GBps'):8.0f}  "
                f"{med(n, B, 'unpack_b_GBps'):8.0f}")
    table = len(lines)
    lines.append("# raw rows")
    lines += [json.dumps(r) for r in rows]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:table]))


if __name__ == "__main__":
    main()
