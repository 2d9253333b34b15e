"""Register / scratch budget of the run kernel k_ipose_run<0/1> (CPU: hipcc
cross-compile only), against the yardstick in its own translation unit: the
single-call kernels k_ipose_predict / k_ipose_visual of the same SO3 side, whose
steps it fuses.  It has no scratch if neither of them has, and at least the
lower of their occupancies."""
import pytest

from test_kernel_resources import HAVE_HIPCC, kernel_usage

SRC = "csrc/uwvk_small.hip"
SINGLE = ("k_ipose_predict", "k_ipose_visual")


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_run_kernels_keep_the_single_kernels_budget():
    use = kernel_usage(SRC, ("_ZN12_GLOBAL__N_1",))
    for side in (0, 1):
        tag = "ILi%dEE" % side
        (name, r), = [(n, v) for n, v in use.items() if "k_ipose_run" + tag in n]
        ref = {}
        for s in SINGLE:
            (ref[s],) = [v for n, v in use.items() if s + tag in n]
        print("k_ipose_run<%d>" % side, r, ref)
        if all(v["scratch"] == 0 for v in ref.values()):
            assert r["scratch"] == 0, (name, r, ref)
        assert r["occupancy"] >= min(v["occupancy"] for v in ref.values()), (name, r, ref)
