"""uwvk_vel_log_host and uwvk_vel_track across the C ABI (CPU): size and field
offsets as a C compiler lays out include/uwvk.h against the ctypes mirrors
abi.VelLogHost / abi.VelTrack, and the ABI version (additive: still 3)."""
import ctypes as C
import os
import subprocess

from uwvk import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ("flags", "dvl_index", "n_dvl", "pressure_index", "n_pressure")
TRACK = ("every", "capacity", "mean", "variance", "model")
ENTRY = ("uwvk_vel_log_check", "uwvk_vel_run_log_track")


def _offsets(struct, tag, fields):
    return "\n".join('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (tag, f, struct, f) for f in fields)


PROG = """
#include <stddef.h>
#include <stdio.h>
#include "uwvk.h"
int main(void) {
  printf("sizeof.host %%zu\\nsizeof.track %%zu\\n", sizeof(uwvk_vel_log_host), sizeof(uwvk_vel_track));
  printf("DVL %%u\\nPRESSURE %%u\\nNAN %%u\\n", UWVK_EV_DVL, UWVK_EV_PRESSURE, UWVK_ST_NAN);
  printf("ABI %%d\\n", UWVK_ABI_VERSION);
%s
%s
  return 0;
}
""" % (_offsets("uwvk_vel_log_host", "host", HOST), _offsets("uwvk_vel_track", "track", TRACK))


def test_vel_track_layout(tmp_path):
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                   check=True)
    out = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True,
                                                       timeout=60).stdout.splitlines())
    for mirror, tag, fields in ((abi.VelLogHost, "host", HOST), (abi.VelTrack, "track", TRACK)):
        assert [n for n, _ in mirror._fields_] == list(fields)
        assert int(out["sizeof." + tag]) == C.sizeof(mirror)
        for f in fields:
            assert int(out["%s.%s" % (tag, f)]) == getattr(mirror, f).offset, (tag, f)
    assert (int(out["DVL"]), int(out["PRESSURE"])) == (abi.EV_DVL, abi.EV_PRESSURE) == (2, 4)
    assert int(out["NAN"]) == 2
    assert int(out["ABI"]) == engine.ABI_VERSION == 3


def test_entry_points_bound():
    L = engine.lib()
    for name in ENTRY:
        assert name in engine.SYMBOLS and hasattr(L, name), name
