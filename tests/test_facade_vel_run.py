"""VelocityUKF::runLog / runLogTrack of the C++ facade
(tests/cpp/vel_run_facade_test.cpp): compiles against the C ABI (CPU); on the
GPU a 20-epoch log in two adjacent runLogTrack calls is bitwise the facade's own
integrateMeasurement / predictionStep sequence at batch 1 and its runLog, and
the one record is bitwise getState."""
import subprocess

import pytest

from test_facade_fixes import _build

NAME = "vel_run_facade_test"


def test_vel_run_facade_compiles(tmp_path):
    _build(str(tmp_path), NAME)


@pytest.mark.gpu
def test_vel_run_facade_matches_single_calls(tmp_path):
    exe = _build(str(tmp_path), NAME)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
