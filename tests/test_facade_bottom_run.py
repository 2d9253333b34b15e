"""BottomUKF::runLog of the C++ facade (tests/cpp/bottom_run_facade_test.cpp):
compiles against the C ABI (CPU); on the GPU a 20-epoch log in two adjacent
calls is bitwise the facade's own setVelocity / predictionStep /
integrateMeasurement sequence."""
import subprocess

import pytest

from test_facade_fixes import _build

NAME = "bottom_run_facade_test"


def test_bottom_run_facade_compiles(tmp_path):
    _build(str(tmp_path), NAME)


@pytest.mark.gpu
def test_bottom_run_facade_matches_single_calls(tmp_path):
    exe = _build(str(tmp_path), NAME)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
