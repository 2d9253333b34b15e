"""The launch plan of uwvk_pose_run_log_fixes (plan_run with fix flags in
csrc/uwvk_plan.hpp) on the CPU: tests/cpp/fix_plan_test.cpp checks that zero fix
flags give plan_epochs' plan, the fixed cases (first / last / adjacent epochs, a
BodyEfforts, pressure and track record epoch, pd after a fix), a per-epoch
restatement over seeded random flag sets, and the argument check fixes_valid.
No device, no libuwvk.so.  Built and run twice, the second time under the
address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_fix_plan(tmp_path, sanitize):
    exe = str(tmp_path / "fix_plan_test")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags,
                    os.path.join(HERE, "cpp", "fix_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
