"""The window planner (aruco_slam_amd/csrc/win_plan.h) by itself, under AddressSanitizer and UBSan.

tests/win_plan_check.cpp is an ordinary executable with its own main: it includes the planner's header, needs no HIP runtime, no
context and no device, and plans batches whose buffers are heap blocks of exactly the size the batch needs.  Exact cases sit at the
sizes of the planner's fixed tables (63 / 64 corrections, 64 / 65 popped observations, |S| = s_cap, kWinFrames + 2 frames, the
widen rule at frame 16, detection index 127, the three "left to the device" causes, the arming frame); a seeded random sweep
asserts the invariants of a plan.  A host-only check: it runs where there is no GPU.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="host-only sanitizer check: runs on machines without a GPU")
def test_win_plan_check(tmp_path):
    exe = str(tmp_path / "win_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-psabi",
                           "-I", os.path.join(ROOT, "tests", "hipemu"), "-I", os.path.join(ROOT, "aruco_slam_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "win_plan_check.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "win_plan_check ok" in r.stdout, r.stdout[-4000:]
