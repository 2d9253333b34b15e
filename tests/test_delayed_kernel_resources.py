"""Register / scratch budget of the fix kernel k_psp_fix<DOF, SR> with the
delayed XY kind in it (CPU: hipcc cross-compile only), against the single-call
kernels k_psp_update<DOF, MK_XY | MK_Z | MK_GEO | MK_DELAYED, SR> of its own
translation unit, whose updates it fuses: no scratch if none of them has, and at
least the lowest of their occupancies."""
import re

import pytest

from test_kernel_resources import HAVE_HIPCC, kernel_usage

MK = {5: "XY", 6: "Z", 7: "GEO", 8: "DELAYED"}  # MeasKind (csrc/uwvk_pose_kernels.hpp)


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
@pytest.mark.parametrize("src,side", [("csrc/uwvk_psp_k.hip", 0), ("csrc/uwvk_psp_k_r.hip", 1)])
def test_fix_kernel_with_the_delayed_kind_keeps_the_single_updates_budget(src, side):
    fix = kernel_usage(src, ("_ZN4uwvk3psp9k_psp_fixILi",))
    upd = kernel_usage(src, ("_ZN4uwvk3psp12k_psp_updateILi",))
    assert len(fix) == 2, sorted(fix)  # DOF 53 / 26 of this unit's side; no kernel of its own for the delayed kind
    for dof in (53, 26):
        (name, r), = [(n, v) for n, v in fix.items() if "k_psp_fixILi%dELi%dEE" % (dof, side) in n]
        ref = {}
        for n, v in upd.items():
            m = re.search(r"k_psp_updateILi(\d+)ELi(\d+)ELi(\d)E", n)
            if int(m.group(1)) == dof and int(m.group(2)) in MK and int(m.group(3)) == side:
                ref[MK[int(m.group(2))]] = v
        assert sorted(ref) == ["DELAYED", "GEO", "XY", "Z"], sorted(upd)
        print(dof, side, "k_psp_fix", r, "k_psp_update", ref)
        if all(v["scratch"] == 0 for v in ref.values()):
            assert r["scratch"] == 0, (name, r, ref)
        assert r["occupancy"] >= min(v["occupancy"] for v in ref.values()), (name, r, ref)
