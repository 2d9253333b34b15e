"""The tile map of the pair kernel's rank-M update (csrc/uwvk_tiles.hpp) on the
CPU: tests/cpp/tiles_test.cpp checks that under the store masks every packed
entry of the lower triangle is stored by exactly one (lane, tile position), that
no lane stores above the diagonal, past the triangle or without a tile, and
that every load index stays inside the instance's LDS block, at 26 DOFs and at
other sizes.  No device, no libuwvk.so: the header is plain C++17.  Built and
run twice, the second time under the address and undefined-behaviour
sanitizers."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_tiles(tmp_path, sanitize):
    exe = str(tmp_path / "tiles_test")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags,
                    os.path.join(HERE, "cpp", "tiles_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
