"""bench.py on a GPU as every pull request runs it: a plain run measures the
headline only and, with --dump-outputs, writes what its last timed step
computed, the same arrays from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_last_step(gpu, tmp_path):
    n, ips = 200, 31  # not a multiple of the tile; ten triples and a single step
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
           "--warmup", "1", "--grid", str(n), "--iters-per-step", str(ips),
           "--dump-outputs", str(tmp_path / "d")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert res["config"]["iterations"] == 3 * ips
    assert res["value"] > 0 and res["unit"] == "Mpx-it/s" and res["dtype"] == "fp32"
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(n * n * ips / res["ms_per_step"] / 1e3, rel=1e-3)
    # nothing but the headline: the --full figures are null
    assert res["cpu_baseline"] is None and res["default_semantics"] is None
    assert res["roofline"]["isolated_launch_us"] is None
    assert sorted(os.listdir(tmp_path / "d")) == ["errors.npy", "motion.npy"]
    motion = np.load(tmp_path / "d" / "motion.npy", allow_pickle=False)
    errors = np.load(tmp_path / "d" / "errors.npy", allow_pickle=False)
    assert motion.dtype == np.float64 and errors.dtype == np.float32
    # the step's own result: one loop of `ips` fixed iterations from zero motion
    from opticalflow2d_amd import SlabSolver
    from opticalflow2d_amd import synthetic as S
    ref, mov = S.procedural_pair(n, 0, n)
    s = SlabSolver(n, n, 0.1)
    s.set_images(ref, mov)
    assert s.run(ips, fixed_iters=True) == ips
    want, werr = s.motion(), s.errors()
    s.close()
    assert motion.shape == (n, n, 2) and np.array_equal(motion, want)
    assert np.array_equal(errors.view(np.uint32), werr.view(np.uint32))
