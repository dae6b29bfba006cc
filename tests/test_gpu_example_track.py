"""examples/demo_batch.py --track runs end to end on the GPU: T frames of B
slices registered frame after frame with warm_start=1 against the default, the
mean iterations per pair printed for both."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "examples", "demo_batch.py")


@pytest.mark.gpu
def test_demo_batch_track(gpu):
    out = subprocess.run([sys.executable, DEMO, "--track", "3", "--frames", "4", "--size", "48",
                          "--niter", "100"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = re.findall(r"^\s*(\d+)\s+[0-9.]+\s+([0-9.]+)\s+([0-9.]+)\s+([0-9.]+)\s+([0-9.]+)$",
                      out.stdout, flags=re.M)
    assert [int(r[0]) for r in rows] == [1, 2, 3], out.stdout[-2000:]
    # the first frame starts from zero on both batches
    assert rows[0][1] == rows[0][2] and rows[0][3] == rows[0][4]
    for r in rows:
        assert 2 < float(r[1]) <= 100 and 2 < float(r[2]) <= 100
    m = re.search(r"mean iterations per pair and frame: warm ([0-9.]+), cold ([0-9.]+)", out.stdout)
    assert m, out.stdout[-2000:]
