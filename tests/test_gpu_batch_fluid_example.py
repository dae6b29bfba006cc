"""examples/demo_batch.py --reg 5 runs to the end on the device."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_demo_batch_fluid(gpu):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "demo_batch.py"), "--reg",
                        "5", "--size", "32", "--frames", "6", "--niter", "20", "--report"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # the launches of an Elastic batch: 4 per loop, an upsample, a zeroing
    assert "6 frames of 32 x 32 against frame 0: 10 kernel launches" in r.stdout, r.stdout
    assert "regrids per frame: [" in r.stdout, r.stdout
    assert "Dumax: 0.650\tMaxabs increment: " in r.stdout, r.stdout
