"""The launch plan of uwvk_pose_run_log_delayed (plan_run with delayed flags in
csrc/uwvk_plan.hpp) on the CPU: tests/cpp/delayed_plan_test.cpp checks that zero
delayed and fix flags give plan_epochs' plan, the fixed cases (a latch on the
first and last epoch, one epoch before an arrival, with an arrival of another
row, on a BodyEfforts, pressure and fix epoch with FIX before LATCH, pdec after a
full BodyEfforts), a per-epoch restatement over seeded random flag sets and
track strides, the plan of a dense handle, and the argument check
delayed_events.  No device, no libuwvk.so.  Built and run twice, the second time
under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_delayed_plan(tmp_path, sanitize):
    exe = str(tmp_path / "delayed_plan_test")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags,
                    os.path.join(HERE, "cpp", "delayed_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
