"""uwvk_pose_visual across the C ABI (CPU): the struct's size and field offsets
as a C compiler lays out include/uwvk.h against the ctypes mirror
abi.PoseVisual, the new entry points exported and listed in the header, and the
ABI version (additive: still 3)."""
import ctypes as C
import os
import re
import subprocess

from uwvk import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("visual_offset", "n_visual", "n_features", "features", "feature_cov", "shared_feature_cov",
          "feature_positions", "marker_pose", "shared_marker_pose", "cov_marker_pose", "camera", "camera_in_imu",
          "applied")
NEW = ("uwvk_pose_visual_check", "uwvk_pose_run_log_visual")

PROG = """
#include <stddef.h>
#include <stdio.h>
#include "uwvk.h"
/* the entry points once more, as the issue states them: a conflicting prototype does not compile */
uwvk_status uwvk_pose_visual_check(const uwvk_pose_visual* visual, int64_t epochs, int64_t first, int64_t count);
uwvk_status uwvk_pose_run_log_visual(uwvk_pose* h, const uwvk_pose_log* log, const uwvk_pose_fixes* fixes,
                                     const uwvk_pose_delayed* delayed, const uwvk_pose_visual* visual, int64_t first,
                                     int64_t count, uint32_t* accept_counts, const uwvk_pose_track* track);
int main(void) {
  printf("sizeof %%zu\\n", sizeof(uwvk_pose_visual));
  printf("ABI %%d\\n", UWVK_ABI_VERSION);
%s
  return 0;
}
""" % "\n".join('  printf("%s %%zu\\n", offsetof(uwvk_pose_visual, %s));' % (f, f) for f in FIELDS)


def test_pose_visual_layout(tmp_path):
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                   check=True)
    out = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True,
                                                       timeout=60).stdout.splitlines())
    assert [n for n, _ in abi.PoseVisual._fields_] == list(FIELDS)
    assert int(out["sizeof"]) == C.sizeof(abi.PoseVisual)
    for f in FIELDS:
        assert int(out[f]) == getattr(abi.PoseVisual, f).offset, f
    assert int(out["ABI"]) == engine.ABI_VERSION == 3


def test_entry_points_bound_and_listed():
    L = engine.lib()
    with open(os.path.join(ROOT, "include", "uwvk.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in engine.SYMBOLS and hasattr(L, name), name
        assert re.search(r"uwvk_status\s+%s\s*\(" % name, header), name
    assert L.uwvk_abi_version() == 3
    # the visual struct mirrors the visual part of uwvk_ipose_log field for field (its camera pose is named for the IMU)
    ip = [n for n, _ in abi.IPoseLog._fields_]
    part = ip[ip.index("visual_offset"):]
    assert [n.replace("camera_in_body", "camera_in_imu") for n in part] == list(FIELDS[:-1])
