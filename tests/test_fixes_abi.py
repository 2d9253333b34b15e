"""uwvk_pose_fixes across the C ABI (CPU): the struct's size and field offsets
as a C compiler lays out include/uwvk.h against the ctypes mirror
abi.PoseFixes, the UWVK_FIX_* constants, and the ABI version (additive: still 3)."""
import ctypes as C
import os
import subprocess

from uwvk import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("host_flags", "xy_index", "xy", "n_xy", "xy_cov", "z_index", "z", "n_z", "z_cov", "geo_index", "geo",
          "n_geo", "geo_cov", "gps_in_body", "accept_counts")

PROG = """
#include <stddef.h>
#include <stdio.h>
#include "uwvk.h"
int main(void) {
  printf("sizeof %%zu\\n", sizeof(uwvk_pose_fixes));
  printf("FIX_XY %%u\\nFIX_Z %%u\\nFIX_GEO %%u\\n", UWVK_FIX_XY, UWVK_FIX_Z, UWVK_FIX_GEO);
  printf("ABI %%d\\n", UWVK_ABI_VERSION);
%s
  return 0;
}
""" % "\n".join('  printf("%s %%zu\\n", offsetof(uwvk_pose_fixes, %s));' % (f, f) for f in FIELDS)


def test_pose_fixes_layout(tmp_path):
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                   check=True)
    out = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True,
                                                       timeout=60).stdout.splitlines())
    assert [n for n, _ in abi.PoseFixes._fields_] == list(FIELDS)
    assert int(out["sizeof"]) == C.sizeof(abi.PoseFixes)
    for f in FIELDS:
        assert int(out[f]) == getattr(abi.PoseFixes, f).offset, f
    assert (int(out["FIX_XY"]), int(out["FIX_Z"]), int(out["FIX_GEO"])) == (abi.FIX_XY, abi.FIX_Z, abi.FIX_GEO)
    assert int(out["ABI"]) == engine.ABI_VERSION == 3


def test_entry_points_bound():
    assert "uwvk_pose_run_log_fixes" in engine.SYMBOLS and "uwvk_schedule_fixes" in engine.SYMBOLS
    L = engine.lib()
    assert hasattr(L, "uwvk_pose_run_log_fixes") and hasattr(L, "uwvk_schedule_fixes")
