"""Register / scratch budget of the run kernel k_pose_visual_run<DOF, SR> (CPU:
hipcc cross-compile only), against the yardstick in its own translation unit:
the single-call kernel k_pose_visual<DOF, SR> whose feature loop it calls once
per row.  It has no more scratch and at least its occupancy."""
import pytest

from test_kernel_resources import HAVE_HIPCC, kernel_usage

SRC = "csrc/uwvk_pose_visual.hip"


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_run_kernel_keeps_the_single_kernels_budget():
    use = kernel_usage(SRC, ("_ZN4uwvk12_GLOBAL__N_1",))
    seen = 0
    for dof in (53, 26):
        for side in (0, 1):
            tag = "ILi%dELi%dEE" % (dof, side)
            (name, r), = [(n, v) for n, v in use.items() if "k_pose_visual_run" + tag in n]
            (ref,) = [v for n, v in use.items() if "k_pose_visual" + tag in n]
            print("k_pose_visual_run<%d, %d>" % (dof, side), r, ref)
            assert r["scratch"] <= ref["scratch"], (name, r, ref)
            assert r["occupancy"] >= ref["occupancy"], (name, r, ref)
            seen += 1
    assert seen == 4
