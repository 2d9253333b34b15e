"""uwvk_pose_track across the C ABI (CPU): the struct's size and field offsets
as a C compiler lays out include/uwvk.h against the ctypes mirror
abi.PoseTrack, and the host-only record count uwvk_pose_track_records."""
import ctypes as C
import os
import subprocess

from uwvk import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("every", "capacity", "mean", "variance", "stats", "truth")

PROG = """
#include <stddef.h>
#include <stdio.h>
#include "uwvk.h"
int main(void) {
  printf("sizeof %%zu\\n", sizeof(uwvk_pose_track));
%s
  return 0;
}
""" % "\n".join('  printf("%s %%zu\\n", offsetof(uwvk_pose_track, %s));' % (f, f) for f in FIELDS)


def test_pose_track_layout(tmp_path):
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                   check=True)
    out = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True,
                                                       timeout=60).stdout.splitlines())
    assert [n for n, _ in abi.PoseTrack._fields_] == list(FIELDS)
    assert int(out["sizeof"]) == C.sizeof(abi.PoseTrack)
    for f in FIELDS:
        assert int(out[f]) == getattr(abi.PoseTrack, f).offset, f


def test_track_records():
    L = engine.lib()
    cases = [  # first, count, every -> records (epochs e with (e + 1) % every == 0)
        ((0, 120, 25), 4),    # 24, 49, 74, 99
        ((0, 70, 25), 2), ((70, 50, 25), 2),
        ((0, 24, 25), 0), ((0, 25, 25), 1), ((24, 1, 25), 1), ((25, 24, 25), 0),
        ((3, 10, 1), 10), ((0, 5, 9), 0), ((13, 0, 7), 0),
        ((1 << 33, 2000, 1000), 2),  # 2^33 = 592 (mod 1000): 2^33 + 407 and + 1407
        ((0, 10, 0), 0), ((0, 10, -3), 0), ((-1, 10, 2), 0), ((0, -1, 2), 0),  # no track: no records
    ]
    for args, want in cases:
        assert L.uwvk_pose_track_records(*args) == want, args
