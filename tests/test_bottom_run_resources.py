"""Register / scratch budget of the run kernel k_bottom_run (CPU: hipcc
cross-compile only), against the yardstick in its own translation unit: the
single-call kernels k_bottom_predict / k_bottom_range / k_bottom_normal whose
steps it fuses.  It has no scratch if none of them has, and at least the lowest
of their occupancies."""
import pytest

from test_kernel_resources import HAVE_HIPCC, kernel_usage

SRC = "csrc/uwvk_small.hip"
SINGLE = ("k_bottom_predict", "k_bottom_range", "k_bottom_normal")


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_run_kernel_keeps_the_single_kernels_budget():
    use = kernel_usage(SRC, ("_ZN12_GLOBAL__N_1",))
    (name, r), = [(n, v) for n, v in use.items() if "k_bottom_runE" in n]
    ref = {}
    for s in SINGLE:
        (ref[s],) = [v for n, v in use.items() if s + "E" in n]
    print("k_bottom_run", r, ref)
    if all(v["scratch"] == 0 for v in ref.values()):
        assert r["scratch"] == 0, (name, r, ref)
    assert r["occupancy"] >= min(v["occupancy"] for v in ref.values()), (name, r, ref)
