"""examples/demo_batch.py --reg 1 runs to the end on the device."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_demo_batch_curvature(gpu):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "demo_batch.py"), "--reg",
                        "1", "--size", "32", "--frames", "6", "--niter", "20"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
