"""The lane map of the pair kernel's fused broadcasts (csrc/uwvk_bcast.hpp) on
the CPU: tests/cpp/bcast_test.cpp emulates a 64-lane wave and checks that
rep16's two copies (one v_permlane16_swap_b32 per dword) and the (copy, N) map
give every lane of either half the value of source lane s < 32 of its own half,
with all lanes active and with one half masked off, for every s and for each
source list of the kernel (Delta_j / Dz_j in lane 2j, P[i][j] in lane i K + j
for M K = 18 and 12; also the Cholesky columns c < 15 and c < 6, whose fused
form was measured and not kept).  No device, no
libuwvk.so: the header is plain C++17.  Built and run twice, the second time
under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_bcast_map(tmp_path, sanitize):
    exe = str(tmp_path / "bcast_test")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags,
                    os.path.join(HERE, "cpp", "bcast_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
