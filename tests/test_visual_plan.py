"""The launch plan of uwvk_pose_run_log_visual (plan_run with visual flags in
csrc/uwvk_plan.hpp) on the CPU: tests/cpp/visual_plan_test.cpp checks the launch
order FIX, VISUAL, LATCH, RECORD on one epoch, adjacent visual epochs, a visual
row on the first and the last epoch of the range, pdec false from the first
VISUAL launch on (no pair or pd launch after it), a plan without visual flags
equal to the plan_run of before, launch for launch, a split range giving the
concatenation of its parts, the plan of a dense handle, and a restatement (the
cut run's plans) over seeded random flag sets.  No device, no libuwvk.so.
Built and run twice, the second time under the address and
undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_visual_plan(tmp_path, sanitize):
    exe = str(tmp_path / "visual_plan_test")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags,
                    os.path.join(HERE, "cpp", "visual_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
