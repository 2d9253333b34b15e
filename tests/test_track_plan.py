"""The record cuts of uwvk_pose_run_log_track (plan_run's RECORD launches /
track_records in csrc/uwvk_plan.hpp) on the CPU: tests/cpp/track_plan_test.cpp
checks, over fixed and seeded random (first, count, every), that the segments
between records tile the range, end
at record epochs, number what the closed form says and compose across a split
of the range.  No device, no libuwvk.so.  Built and run twice, the second time
under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_track_plan(tmp_path, sanitize):
    exe = str(tmp_path / "track_plan_test")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags,
                    os.path.join(HERE, "cpp", "track_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
