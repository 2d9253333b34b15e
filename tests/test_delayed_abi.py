"""uwvk_pose_delayed across the C ABI (CPU): the struct's size and field offsets
as a C compiler lays out include/uwvk.h against the ctypes mirror
abi.PoseDelayed, the new entry points, and the ABI version (additive: still 3;
uwvk_pose_fixes keeps its layout, tests/test_fixes_abi.py)."""
import ctypes as C
import os
import subprocess

from uwvk import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("index", "latch_epoch", "xy", "n", "xy_cov", "latched", "accept_counts")

PROG = """
#include <stddef.h>
#include <stdio.h>
#include "uwvk.h"
/* the entry points once more, as the issue states them: a conflicting prototype does not compile */
uwvk_status uwvk_pose_run_log_delayed(uwvk_pose* h, const uwvk_pose_log* log, const uwvk_pose_fixes* fixes,
                                      const uwvk_pose_delayed* delayed, int64_t first, int64_t count,
                                      uint32_t* accept_counts, const uwvk_pose_track* track);
uwvk_status uwvk_schedule_delayed(const double* imu, int64_t n_imu, const double* stamp_t, const double* arrival_t,
                                  int64_t n, double time_epsilon, int32_t* index, int32_t* latch_epoch,
                                  int64_t* kept, int64_t* dropped);
int main(void) {
  printf("sizeof %%zu\\n", sizeof(uwvk_pose_delayed));
  printf("ABI %%d\\n", UWVK_ABI_VERSION);
%s
  return 0;
}
""" % "\n".join('  printf("%s %%zu\\n", offsetof(uwvk_pose_delayed, %s));' % (f, f) for f in FIELDS)


def test_pose_delayed_layout(tmp_path):
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                   check=True)
    out = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True,
                                                       timeout=60).stdout.splitlines())
    assert [n for n, _ in abi.PoseDelayed._fields_] == list(FIELDS)
    assert int(out["sizeof"]) == C.sizeof(abi.PoseDelayed)
    for f in FIELDS:
        assert int(out[f]) == getattr(abi.PoseDelayed, f).offset, f
    assert int(out["ABI"]) == engine.ABI_VERSION == 3


def test_entry_points_bound():
    assert "uwvk_pose_run_log_delayed" in engine.SYMBOLS and "uwvk_schedule_delayed" in engine.SYMBOLS
    L = engine.lib()
    assert hasattr(L, "uwvk_pose_run_log_delayed") and hasattr(L, "uwvk_schedule_delayed")
    assert L.uwvk_abi_version() == 3
