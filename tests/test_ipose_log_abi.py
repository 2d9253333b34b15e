"""uwvk_ipose_log and uwvk_ipose_track across the C ABI (CPU): size and field
offsets as a C compiler lays out include/uwvk.h against the ctypes mirrors
abi.IPoseLog / abi.IPoseTrack, and the ABI version (additive: still 3)."""
import ctypes as C
import os
import subprocess

from uwvk import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = ("epochs", "dt", "dt_epoch", "pose_ref", "visual_offset", "n_visual", "n_features", "features", "feature_cov",
       "shared_feature_cov", "feature_positions", "marker_pose", "shared_marker_pose", "cov_marker_pose", "camera",
       "camera_in_body")
TRACK = ("every", "capacity", "mean", "variance", "corrected")
ENTRY = ("uwvk_ipose_log_check", "uwvk_ipose_run_log", "uwvk_ipose_synchronize")


def _offsets(struct, tag, fields):
    return "\n".join('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (tag, f, struct, f) for f in fields)


PROG = """
#include <stddef.h>
#include <stdio.h>
#include "uwvk.h"
int main(void) {
  printf("sizeof.log %%zu\\nsizeof.track %%zu\\n", sizeof(uwvk_ipose_log), sizeof(uwvk_ipose_track));
  printf("ABI %%d\\n", UWVK_ABI_VERSION);
%s
%s
  return 0;
}
""" % (_offsets("uwvk_ipose_log", "log", LOG), _offsets("uwvk_ipose_track", "track", TRACK))


def test_ipose_log_layout(tmp_path):
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                   check=True)
    out = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True,
                                                       timeout=60).stdout.splitlines())
    for mirror, tag, fields in ((abi.IPoseLog, "log", LOG), (abi.IPoseTrack, "track", TRACK)):
        assert [n for n, _ in mirror._fields_] == list(fields)
        assert int(out["sizeof." + tag]) == C.sizeof(mirror)
        for f in fields:
            assert int(out["%s.%s" % (tag, f)]) == getattr(mirror, f).offset, (tag, f)
    assert int(out["ABI"]) == engine.ABI_VERSION == 3


def test_entry_points_bound():
    L = engine.lib()
    for name in ENTRY:
        assert name in engine.SYMBOLS and hasattr(L, name), name
