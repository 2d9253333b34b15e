"""IndirectPoseUKF::runLog of the C++ facade (tests/cpp/ipose_run_facade_test.cpp):
compiles against the C ABI (CPU); on the GPU a 6-epoch log in two adjacent
calls is bitwise the facade's own updatePoseReference / predictionStep /
integrateMeasurement sequence, and its corrected-pose record is getCorrectedPose
to rounding."""
import subprocess

import pytest

from test_facade_fixes import _build

NAME = "ipose_run_facade_test"


def test_ipose_run_facade_compiles(tmp_path):
    _build(str(tmp_path), NAME)


@pytest.mark.gpu
def test_ipose_run_facade_matches_single_calls(tmp_path):
    exe = _build(str(tmp_path), NAME)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
