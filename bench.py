#!/usr/bin/env python3
"""Horn-Schunck Jacobi throughput on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--grid G] [--weak]
                    [--dump-outputs DIR] [--full]

One step = one pass of the hot path: the Horn-Schunck iteration loop of
ImageRegistrationOpticalFlow::estimate_motion_at_current_resolution
(ImageRegistrationOpticalFlow.cpp:123-135) over the whole grid with BASELINE
config 2's 1000 Jacobi iterations (--iters-per-step), each iteration
OpticalFlowDiffusion::get_update + the Logger norms, plus the per-chunk norm
reductions, the read-back of the loop's Logger errors and motion_est->reset()
(:141), and — for N > 1 — the RCCL halo exchanges.  Iterations run in threes
fused into one pass over HBM (hs::jacobi3_kernel: 28 B/px per launch, three iterations per launch,
bit-identical to three single steps; chunks of 33 iterations are eleven
launches, and a single step or a pair fills the run's tail), with a three-j-line
halo exchange per launch overlapped with the interior bands.  Early exit is
disabled (fixed_iters) so that exactly K x 1000 iterations run.

Workloads (BASELINE.json configs):
  N = 1 (default --grid 4096)   config 2: Horn-Schunck 4096^2 fp32 on one GPU
  N > 1 (default --grid 16384)  config 5: Horn-Schunck 16384^2, row slabs of
                                16384/N j-lines per GPU, RCCL halo over xGMI
                                (strong scaling: the global grid is fixed)
  --grid G at any N             G x G split into N row slabs (strong)
  --weak                        every rank owns a G-row slab of a G x (G N)
                                grid (weak scaling)

Per-run setup stays outside the timed region, as in the reference's own loop:
the gradients and the divide-by-zero test run in set_images (once per image
pair), the Logger sums of a loop are reserved before the warm-up, and
the zeroing of the next run's start buffer (motion_est->reset(),
ImageRegistrationOpticalFlow.cpp:141) is enqueued at the end of the previous
run.  The timed region is exactly K loops of 1000 iterations, each followed
by the read-back of its Logger sums (one host synchronisation per loop, as the
reference returns to its caller after every loop).

A plain run does only what `value` needs: set-up, warm-up, the K timed steps,
the output dump when --dump-outputs is given, the JSON line.  --dump-outputs DIR
writes what the last timed step left for its caller as DIR/<name>.npy: `motion`
(float64, the slab's [dimx, rows, 2] motion, or a fixed seeded sample of its
pixels as [k, 2] once the whole field would pass the dump's byte budget) and
`errors` (float32, the loop's Logger errors); with N > 1 every rank writes
`motion_rank<r>` and rank 0 `errors`.  The inputs are the same from run to run,
so two builds can be compared array for array.

Everything else runs only with --full, after the timed region and the dump: the
kernel's isolated back-to-back launch time (`roofline.isolated_launch_us`), the
convergence-on loop (`default_semantics`) and the CPU baseline (`cpu_baseline`);
a plain run leaves these three null.

With --full (N = 1 on config 2's grid, rank 0) the JSON line's
`default_semantics` object records the default convergence-on loop at 4096^2 —
the reference's Logger and break, not part of `value`: iterations executed
against the reference fixtures' 102 / 397, the motion's match, us per
iteration (or the error it raised).  With row slabs whose triples split
(N > 1, or --rccl --self-halo), `config.halo_timing` holds the halo's cost per
launch for rank 0, a middle rank and every rank, sampled with HIP events.

Inputs are a synthetic procedural texture pair generated per slab.  For N > 1
launch with torch.distributed.run (one process per GPU); torch.distributed
(gloo) bootstraps the RCCL communicator, barriers and takes the max time.
Prints one JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "Mpixel-iterations/sec + achieved HBM GB/s, Horn-Schunck 4096^2 @ 1/2/4/8 GPU"
BYTES_PER_PX_IT = 28  # read u 8 + dI 8 + It 4, write u 8
# the fused kernel reads u 8 + dI 8 + It 4 and writes u 8 B/px once per launch
# and advances THREE iterations; once dI + It no longer fit in the MALL it
# derives dI from Iaux in the kernel and reads Iaux 4 instead of dI 8
BYTES_PER_PX_LAUNCH = {"image": 24, "field": 28}
ITERS_PER_LAUNCH = 3
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s peak (spec)
ALPHA = 0.1
KERNEL = {"image": "of2d::hs::jacobi3_kernel<0,4,true,4,4,1,true,true> (gradients from Iaux)",
          "field": "of2d::hs::jacobi3_kernel<0,4,true,4,4,1,true,false> (gradients read from dI)"}
TRAFFIC_PROFILE = os.path.join("profiles", "hs_traffic.json")
# --dump-outputs: bytes a run writes at most, every rank and array together
DUMP_BUDGET = 48 << 20
DUMP_SEED = 0


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # a step is a 1000-iteration loop (28 ms at 4096^2): even the driver's W=5
    # runs past the clock transient of the first ~40 ms of sustained load
    # (profiles/r01_v14_bench_warmup.log)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters-per-step", type=int, default=1000,
                    help="Jacobi iterations per step (config 2: 1000)")
    ap.add_argument("--grid", type=int, default=0,
                    help="global grid G x G (default: 4096 at N=1 = config 2, "
                         "16384 at N>1 = config 5)")
    ap.add_argument("--weak", action="store_true",
                    help="weak scaling: each rank owns G rows of a G x (G N) grid")
    ap.add_argument("--size", type=int, default=0, help=argparse.SUPPRESS)  # old name of --grid
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the last step's motion and Logger "
                         "errors as DIR/<name>.npy (a fixed seeded sample of a large motion)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also measure the isolated kernel launches, "
                         "the convergence-on loop (default_semantics) and the CPU baseline")
    ap.add_argument("--cpu-iters", type=int, default=20)
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="threads of the all-cores CPU baseline (default: OMP_NUM_THREADS, "
                         "else every CPU)")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the CPU baseline")
    ap.add_argument("--gradients", choices=["auto", "image", "field"], default="auto",
                    help="triple kernel: derive dI from Iaux in the kernel (image, 24 B/px "
                         "per launch) or read the stored field dI (field, 28 B/px); auto "
                         "(default): image once dI + It exceed the 256 MB MALL")
    ap.add_argument("--timing-launches", type=int, default=200)
    ap.add_argument("--no-default-semantics", action="store_true",
                    help="with --full: skip the convergence-on (reference Logger) measurement "
                         "after the timed region")
    ap.add_argument("--rccl", action="store_true",
                    help="N = 1: run the Logger all-reduces through a one-rank RCCL communicator")
    ap.add_argument("--self-halo", action="store_true",
                    help="with --rccl at N = 1: the one-rank communicator also sends its "
                         "boundary j-lines to itself between split interior / edge launches "
                         "(slab options rccl_self_halo, split): the N > 1 halo path and its "
                         "timing fields on one GPU")
    return ap.parse_args(argv)


def workload(args, world: int) -> dict:
    """Global grid and scaling mode of this run."""
    g = args.grid or args.size or (4096 if world == 1 else 16384)
    if args.weak:
        dimx, dimy, scaling = g, g * world, "weak"
    else:
        dimx, dimy, scaling = g, g, "strong"
    if dimx == 4096 and dimy == 4096:
        name = "config 2: Horn-Schunck 4096^2 fp32, 1 MI355X"
    elif dimx == 16384 and dimy == 16384:
        name = (f"config 5: Horn-Schunck 16384^2 row-slab sharded over {world} MI355X, "
                "RCCL halo over xGMI")
    else:
        name = f"Horn-Schunck {dimx}x{dimy} row slabs over {world} GPU(s)"
    return {"dimx": dimx, "dimy": dimy, "scaling": scaling, "workload": name}


def cpu_threads(args) -> int:
    if args.cpu_threads > 0:
        return args.cpu_threads
    env = os.environ.get("OMP_NUM_THREADS", "")
    if env.isdigit() and int(env) > 0:
        return min(int(env), os.cpu_count() or 1)
    return os.cpu_count() or 1


def cpu_baseline(size: int, iters: int, threads: int) -> dict:
    """The oracle (C restatement of the reference path) timed on `iters`
    Horn-Schunck iterations of the same size x size workload: once on 1 thread
    in the reference's loop order (i outer / j inner, what the single-threaded
    MEX path does), once on `threads` OpenMP threads over j-lines (the Jacobi
    update is order independent: same motion bit for bit, test_oracle.py)."""
    from oracle import oracle as O
    from opticalflow2d_amd import synthetic as S
    L = O.lib()
    ref, mov = S.procedural_pair(size, 0, size)
    I = np.ascontiguousarray(mov.reshape(-1, order="F").astype(np.float32))
    Ir = np.ascontiguousarray(ref.reshape(-1, order="F").astype(np.float32))
    n = size * size
    dI = np.zeros(2 * n, np.float32)
    It = np.zeros(n, np.float32)
    L.oracle_spatial_derivative(I, size, size, dI)
    L.oracle_temporal_derivative(Ir, I, n, It)
    errs = np.zeros(iters, np.float32)
    u = np.zeros(2 * n, np.float32)
    L.oracle_set_reference_loop_order(1)
    t0 = time.perf_counter()
    L.oracle_hs_loop(u, dI, It, size, size, ALPHA, iters, 1, errs)
    dt1 = time.perf_counter() - t0
    L.oracle_set_reference_loop_order(0)
    mt_iters = iters * 4
    u = np.zeros(2 * n, np.float32)
    errs = np.zeros(mt_iters, np.float32)
    L.oracle_hs_loop_mt(u, dI, It, size, size, ALPHA, 1, threads, errs)  # thread pool up
    u[:] = 0
    t0 = time.perf_counter()
    L.oracle_hs_loop_mt(u, dI, It, size, size, ALPHA, mt_iters, threads, errs)
    dtn = time.perf_counter() - t0
    return {"value": round(n * iters / dt1 / 1e6, 2), "unit": "Mpx-it/s", "cores": 1,
            "kind": "port",
            "sample": f"oracle HS loop (Jacobi + Logger), {size}x{size}, {iters} iterations, "
                      f"1 thread, reference loop order, {dt1:.1f} s",
            "all_cores": {"value": round(n * mt_iters / dtn / 1e6, 2), "unit": "Mpx-it/s",
                          "cores": threads, "nproc": os.cpu_count(),
                          "sample": f"oracle HS loop, {size}x{size}, {mt_iters} iterations, "
                                    f"{threads} OpenMP threads over j-lines, {dtn:.1f} s"}}


def default_semantics(reps: int = 2) -> dict:
    """The default (reference-exact) convergence-on loop at config 2's grid,
    measured after the timed region and kept out of `value`: the 4096^2
    texture and procedural pairs of the convergence fixtures
    (tests/golden/convergence_hs_*4096.json, the oracle's record of the
    reference's Logger and break, ImageRegistrationOpticalFlow.cpp:131-134), each
    on fresh registrations (init -> set_images untimed -> estimate timed, as a
    MEX register call after init), right behind a warm-up registration of the
    same pair (the clocks ramp within ~40 ms of load: the loops are 20-80 ms).
    Records the iterations executed (the reference breaks at 102 and 397),
    whether the motion's SHA-256 matches the fixture, and the best of `reps`
    estimates' wall time per iteration."""
    import hashlib
    from opticalflow2d_amd import ImageRegistration, set_print_sink
    from opticalflow2d_amd import synthetic as S
    set_print_sink(lambda s: None)
    n = 4096
    out = {"grid": [n, n], "niter": 1000, "alpha": ALPHA,
           "logger": "reference float running sums (default)",
           "registration": f"fresh per estimate, best of {reps} after a warm-up"}
    pairs = {"texture": (S.texture_pair(n), "convergence_hs_texture4096.json"),
             "procedural": (S.procedural_pair(n, 0, n), "convergence_hs_procedural4096.json")}
    for name, ((ref, mov), fx_name) in pairs.items():
        fx = json.load(open(os.path.join(ROOT, "tests", "golden", fx_name)))
        best, it, ok = 1e30, None, True
        for rep in range(reps + 1):  # rep 0: the warm-up
            with ImageRegistration((n, n), [1000], 0, 0, [ALPHA]) as r:
                r.set_images(ref, mov)
                t0 = time.perf_counter()
                r.estimate()
                dt = time.perf_counter() - t0
                if rep == 0:
                    continue
                it = r.iterations()[0]
                f = np.asarray(r.motion(), np.float32)
            planar = np.concatenate([f[:, :, 0].reshape(-1, order="F"),
                                     f[:, :, 1].reshape(-1, order="F")])
            ok = ok and (hashlib.sha256(planar.tobytes()).hexdigest()
                         == fx["motion_sha256_f32_planar"]) and it == fx["iterations_executed"][0]
            best = min(best, dt)
        out[name] = {"iterations": it,
                     "reference_iterations": fx["iterations_executed"][0],
                     "motion_matches_reference": ok,
                     "ms": round(best * 1e3, 3), "us_per_iteration": round(best * 1e6 / it, 1)}
    return out


def halo_summary(per_rank: list) -> dict | None:
    """The halo's cost per split triple launch (slab.last_run_halo_us averaged
    over the timed runs), for rank 0, a middle rank and every rank: how long
    the solver stream waited for the previous launch's edge launches (stall),
    the exchange on the halo stream, the two edge launches."""
    if not per_rank or not any(r and r.get("sampled") for r in per_rank):
        return None
    mid = len(per_rank) // 2
    return {"sampled_launches_per_run": max(r.get("sampled", 0) for r in per_rank),
            "unit": "us per sampled split triple",
            "rank0": per_rank[0], "rank_mid": dict(per_rank[mid], rank=mid),
            "per_rank": per_rank}


def dump_arrays(motion: np.ndarray, errors: np.ndarray, rank: int = 0, world: int = 1,
                budget: int = DUMP_BUDGET) -> dict:
    """name -> array of --dump-outputs for one rank: the slab's motion
    ([dimx, rows, 2] float64) whole when the rank's share of `budget` bytes
    holds it, else the [k, 2] motion of k pixels drawn once with DUMP_SEED
    (sorted column-major pixel indices, the same in every run of the same
    grid), and on rank 0 the Logger errors (float32)."""
    motion = np.asarray(motion, np.float64)
    errors = np.asarray(errors, np.float32)
    out = {}
    share = budget // world
    if rank == 0:
        out["errors"] = errors
        share -= errors.nbytes
    pixels = motion.shape[0] * motion.shape[1]
    k = max(share // 16, 1)
    if pixels > k:
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(pixels, size=k, replace=False))
        motion = np.ascontiguousarray(motion.reshape((pixels, 2), order="F")[idx])
    out["motion" if world == 1 else f"motion_rank{rank}"] = motion
    return out


def dump_outputs(dirname: str, arrays: dict) -> None:
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a, allow_pickle=False)


def load_traffic(dimx: int, rows: int, gradients: str = "field"):
    """PMC traffic per launch from the committed profile, only for the grid it
    was measured on (it is not measured inside this run)."""
    p = os.path.join(ROOT, TRAFFIC_PROFILE)
    try:
        t = json.load(open(p))
    except Exception:
        return None
    if list(t.get("grid", [])) != [dimx, rows] or t.get("gradients", "field") != gradients:
        return None
    return t


def make_record(*, world, wl, steps, warmup, elapsed, gpu_ms, avg_us, iso_us, px_rank, info,
                loop_us=None, avg_n=0,
                traffic, cpu, rows_per_rank, iters_per_step=1, gradients="image",
                semantics=None, halo=None):
    """The JSON line (bench.py contract + roofline + cpu_baseline)."""
    dimx, dimy = wl["dimx"], wl["dimy"]
    total_px = dimx * dimy
    bpl = BYTES_PER_PX_LAUNCH[gradients]
    achieved = bpl * px_rank / (avg_us * 1e-6) / 1e9
    iters = steps * iters_per_step
    return {
        "metric": METRIC,
        "value": round(total_px * iters / elapsed / 1e6, 1),
        "unit": "Mpx-it/s",
        "n_gpus": world,
        "steps": steps,
        "warmup": warmup,
        "ms_per_step": round(1000 * elapsed / steps, 5),
        "higher_is_better": True,
        "scaling": wl["scaling"],
        "vs_baseline": None,
        "dtype": "fp32",
        "data": "synthetic (procedural texture pair, shift (1.5,-0.75))",
        "config": {
            "workload": wl["workload"],
            "grid": [dimx, dimy],
            "alpha": ALPHA,
            "step": (f"one HS iteration loop of {iters_per_step} fixed Jacobi iterations "
                     "(ImageRegistrationOpticalFlow.cpp:123-135) + its Logger read-back"),
            "iterations_per_step": iters_per_step,
            "iterations": iters,
            "fixed_iters": True,
            "parallelism": f"row-slab x{world}",
            "rows_per_rank": rows_per_rank,
            "rccl_ranks": info.get("rccl_ranks", 0),
            "halo_lines_per_launch": info.get("halo_lines", 0),
            "halo_bytes_per_exchange": (2 * info.get("halo_lines", 0) * dimx * 8
                                        if world > 1 else 0),
            "interior_edge_split": bool(info.get("split", 0)),
            "halo_timing": halo,
            "gpu_ms_rank0": round(gpu_ms, 3),
            "wall_over_gpu_rank0": round(elapsed * 1000.0 / gpu_ms, 4) if gpu_ms > 0 else None,
            # the path's own algorithmic traffic (28 B/px per fused launch) per GPU
            "hbm_GBps_from_step_time": round(bpl * total_px * iters
                                             / ITERS_PER_LAUNCH / elapsed / 1e9 / world, 1),
            # the reference algorithm's 28 B per pixel-iteration at this rate
            "ref_bytes_GBps_equiv": round(BYTES_PER_PX_IT * total_px * iters
                                          / elapsed / 1e9 / world, 1),
        },
        "roofline": {
            "bound": "hbm",
            "kernel": KERNEL[gradients],
            "scope": "per GPU (rank 0's slab)",
            "iterations_per_launch": ITERS_PER_LAUNCH,
            "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4),
            "avg_launch_us": round(avg_us, 3),
            "avg_launch_source": ("HIP events on the solver's stream around each chunk's "
                                  "back-to-back triple launches inside the timed loops "
                                  f"({avg_n} launches)"),
            "loop_us_per_3_iterations": round(loop_us, 3) if loop_us else None,
            "isolated_launch_us": round(iso_us, 3) if iso_us is not None else None,
            "bytes_per_launch": bpl * px_rank,
            "bytes_per_px_launch": bpl,
            "traffic": (traffic or {}).get("bytes_per_launch"),
            "traffic_source": (f"{TRAFFIC_PROFILE} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, "
                               "committed profile of this kernel at this grid; not measured "
                               "in this run)" if traffic else None),
            # the unfused reference algorithm's 28 B per pixel-iteration at the
            # kernel's per-iteration rate, as a fraction of the HBM peak
            "ref_equiv_frac": round(BYTES_PER_PX_IT * px_rank * ITERS_PER_LAUNCH
                                    / (avg_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
        },
        "cpu_baseline": cpu,
        "default_semantics": semantics,
    }


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            print("bench.py: --gpus > 1 must be launched with torch.distributed.run",
                  file=sys.stderr)
            sys.exit(2)

    # libof2d (and the /opt/rocm HIP runtime and RCCL it links) loads before
    # torch at every N: torch ships its own libamdhip64 / librccl under the same
    # sonames, and whichever loads first serves both
    from opticalflow2d_amd import SlabSolver, lib
    from opticalflow2d_amd import synthetic as S
    from opticalflow2d_amd.slab import halo_rows, rccl_unique_id
    lib()

    dist = None
    if world > 1 or "WORLD_SIZE" in os.environ:  # launched by torch.distributed.run
        import torch.distributed as dist  # noqa: F811
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)

    uid = None
    if world == 1 and args.rccl:
        uid = rccl_unique_id()  # one-rank communicator: the RCCL all-reduces run too
    elif world > 1:
        obj = [rccl_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(obj, src=0)
        uid = obj[0]

    wl = workload(args, world)
    dimx, dimy = wl["dimx"], wl["dimy"]
    solver = SlabSolver(dimx, dimy, ALPHA, rank, world, device=local, unique_id=uid)
    lo, hi = halo_rows(dimy, rank, world)
    ref, mov = S.procedural_pair(dimx, lo, hi)
    solver.set_images(ref, mov)
    del ref, mov
    solver.set_option("hs_gradients_from_image",
                      {"auto": -1, "image": 1, "field": 0}[args.gradients])
    if args.self_halo:
        if not (world == 1 and uid is not None):
            print("bench.py: --self-halo needs --rccl at N = 1", file=sys.stderr)
            sys.exit(2)
        solver.set_option("rccl_self_halo", 1)
        solver.set_option("split", 1)
    ips = args.iters_per_step
    solver.reserve(ips)
    info = solver.info()
    gradients = "image" if info.get("gradients_from_image") else "field"

    def barrier():
        if dist is not None:
            dist.barrier()
        try:  # drains every stream of the device (the solver's own stream included)
            import torch
            if torch.cuda.is_available():
                torch.cuda.synchronize(local)
        except Exception:
            pass

    for _ in range(args.warmup):
        solver.run(ips, fixed_iters=True)
    barrier()
    gpu_ms = 0.0
    done = 0
    tri_us, tri_n = 0.0, 0
    halo = {"stall_us": 0.0, "exchange_us": 0.0, "edges_us": 0.0, "sampled": 0}
    t0 = time.perf_counter()
    for _ in range(args.steps):
        done += solver.run(ips, fixed_iters=True)  # returns after the stream is drained
        gpu_ms += solver.last_run_ms()
        us, n = solver.last_run_kernel_us()
        tri_us += us * n
        tri_n += n
        h = solver.last_run_halo_us()
        for k in ("stall_us", "exchange_us", "edges_us"):
            halo[k] += h[k] / args.steps
        halo["sampled"] = max(halo["sampled"], h["sampled"])
    t1 = time.perf_counter()
    barrier()
    elapsed = t1 - t0
    if dist is not None:
        import torch
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    assert done == args.steps * ips
    halo = {"rank": rank, **{k: round(v, 3) if isinstance(v, float) else v
                             for k, v in halo.items()}}
    halos = [halo]
    if dist is not None:
        halos = [None] * world
        dist.all_gather_object(halos, halo)

    # dominant kernel: its own average duration per launch inside the timed
    # loops, from the HIP events the solver records on its stream around each
    # chunk's back-to-back triple launches (the per-chunk partial reductions
    # and the loop's single-step tail are outside them)
    avg_us = tri_us / tri_n if tri_n else gpu_ms * 1000.0 * ITERS_PER_LAUNCH / (args.steps * ips)
    # per iteration over the whole loop (reductions and tail included)
    loop_us = gpu_ms * 1000.0 * ITERS_PER_LAUNCH / (args.steps * ips)
    if args.dump_outputs:  # what the last timed step left for its caller
        dump_outputs(args.dump_outputs, dump_arrays(solver.motion(), solver.errors(), rank, world))
    # and back-to-back launches of the kernel alone, after the run
    iso_us = solver.time_kernel(args.timing_launches) if args.full else None
    rows = solver.row_end - solver.row_begin
    px_rank = dimx * rows

    if rank == 0:
        cpu = None
        semantics = None
        # the convergence-on loop at config 2's grid, only when that is the
        # timed grid; a failure there is recorded and never costs the line
        if (args.full and world == 1 and not args.no_default_semantics
                and (dimx, dimy) == (4096, 4096)):
            try:
                semantics = default_semantics()
            except Exception as e:  # noqa: BLE001
                semantics = {"error": f"{type(e).__name__}: {e}"}
        if args.full and world == 1 and not args.no_cpu_baseline:
            # the same grid; iterations scaled to keep the sample at ~15-30 s
            cpu_it = max(1, int(args.cpu_iters * (4096.0 / dimx) ** 2))
            cpu = cpu_baseline(dimx, cpu_it, cpu_threads(args))
        rec = make_record(world=world, wl=wl, steps=args.steps, warmup=args.warmup,
                          elapsed=elapsed, gpu_ms=gpu_ms, avg_us=avg_us, iso_us=iso_us,
                          loop_us=loop_us, avg_n=tri_n,
                          px_rank=px_rank, info=info, traffic=load_traffic(dimx, rows, gradients),
                          cpu=cpu, rows_per_rank=rows, iters_per_step=ips,
                          gradients=gradients, semantics=semantics,
                          halo=halo_summary(halos))
        print(json.dumps(rec), flush=True)
    solver.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
