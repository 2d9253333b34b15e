"""The host planner of uwvk_pose_run_log (csrc/uwvk_plan.hpp) on the CPU:
tests/cpp/plan_test.cpp checks which epoch kernel a handle runs, the split of a
log range into launches (against a naive restatement of the rule, over seeded
random logs), the grid / tail geometry of a launch, the process-noise tables
and the parameter-block scan.  No device, no libuwvk.so: the header is plain
C++17.  Built and run twice, the second time under the address and
undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_plan(tmp_path, sanitize):
    exe = str(tmp_path / "plan_test")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags,
                    os.path.join(HERE, "cpp", "plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
