"""The quad schedule of the fixed-iteration run (opticalflow2d_amd/csrc/
iter_schedule.h: plan_fused with quads, fixed_chunk) checked on the CPU by the
stand-alone program tests/host/iter_schedule_quads_test.cpp, compiled here:
no device and no libof2d.so."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "iter_schedule_quads_test.cpp")
CSRC = os.path.join(ROOT, "opticalflow2d_amd", "csrc")


def test_iter_schedule_quads_host_program(tmp_path):
    exe = str(tmp_path / "iter_schedule_quads_test")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall",
                           "-Wextra", "-I" + CSRC, "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout, r.stdout
