"""uwvk_bottom_log and uwvk_bottom_track across the C ABI (CPU): size and field
offsets as a C compiler lays out include/uwvk.h against the ctypes mirrors
abi.BottomLog / abi.BottomTrack, the UWVK_BEV_* constants, and the ABI version
(additive: still 3)."""
import ctypes as C
import os
import subprocess

from uwvk import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = ("epochs", "dt", "flags", "velocity", "beams", "beam_direction", "beam_origin", "range_index", "range",
       "range_var", "n_range", "range_cov", "normal_index", "normal", "n_normal", "normal_cov")
TRACK = ("every", "capacity", "mean", "variance")
ENTRY = ("uwvk_bottom_log_check", "uwvk_bottom_run_log", "uwvk_bottom_synchronize")


def _offsets(struct, tag, fields):
    return "\n".join('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (tag, f, struct, f) for f in fields)


PROG = """
#include <stddef.h>
#include <stdio.h>
#include "uwvk.h"
int main(void) {
  printf("sizeof.log %%zu\\nsizeof.track %%zu\\n", sizeof(uwvk_bottom_log), sizeof(uwvk_bottom_track));
  printf("MAX_BEAMS %%d\\nBEAM0 %%u\\nBEAM7 %%u\\nNORMAL %%u\\n", UWVK_BOTTOM_MAX_BEAMS, UWVK_BEV_BEAM(0),
         UWVK_BEV_BEAM(7), UWVK_BEV_NORMAL);
  printf("ABI %%d\\n", UWVK_ABI_VERSION);
%s
%s
  return 0;
}
""" % (_offsets("uwvk_bottom_log", "log", LOG), _offsets("uwvk_bottom_track", "track", TRACK))


def test_bottom_log_layout(tmp_path):
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                   check=True)
    out = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True,
                                                       timeout=60).stdout.splitlines())
    for mirror, tag, fields in ((abi.BottomLog, "log", LOG), (abi.BottomTrack, "track", TRACK)):
        assert [n for n, _ in mirror._fields_] == list(fields)
        assert int(out["sizeof." + tag]) == C.sizeof(mirror)
        for f in fields:
            assert int(out["%s.%s" % (tag, f)]) == getattr(mirror, f).offset, (tag, f)
    assert int(out["MAX_BEAMS"]) == abi.BOTTOM_MAX_BEAMS == 8
    assert (int(out["BEAM0"]), int(out["BEAM7"])) == (abi.bev_beam(0), abi.bev_beam(7)) == (1, 128)
    assert int(out["NORMAL"]) == abi.BEV_NORMAL == 0x100
    assert int(out["ABI"]) == engine.ABI_VERSION == 3


def test_entry_points_bound():
    L = engine.lib()
    for name in ENTRY:
        assert name in engine.SYMBOLS and hasattr(L, name), name
