"""Register / scratch budget of the screened VelocityUKF epoch kernels (CPU:
hipcc cross-compile only): both exist, the lane-per-filter one
(k_vel_epoch_track) compiles without scratch, the 16-lane-row one
(k_vel_epoch_g_track<16>) runs at 1 wave per SIMD or better.  The row kernel's
scratch is printed beside k_vel_epoch_g<16>'s, not bounded: what the extra live
state (status, counts, the record cursor) costs had not been measured when
this was written; the figures are in the commit message."""
import pytest

from test_kernel_resources import HAVE_HIPCC, kernel_usage


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_screened_velocity_kernels():
    u = kernel_usage("csrc/uwvk_vel.hip", ("_ZN12_GLOBAL__N_1", "_ZN4uwvk"), flags=[])
    lane = [n for n in u if "k_vel_epoch_track" in n]
    row16 = [n for n in u if "k_vel_epoch_g_trackILi16E" in n]
    row32 = [n for n in u if "k_vel_epoch_g_trackILi32E" in n]
    plain16 = [n for n in u if "k_vel_epoch_gILi16E" in n]
    assert len(lane) == 1 and len(row16) == 1 and len(row32) == 1 and len(plain16) == 1, sorted(u)
    for name in (lane[0], row16[0], row32[0], plain16[0]):
        print(name, u[name])
    assert u[lane[0]]["scratch"] == 0, u[lane[0]]
    assert u[row16[0]]["occupancy"] >= 1, u[row16[0]]
    print("ScratchSize [bytes/lane]: k_vel_epoch_g_track<16> %d, k_vel_epoch_g<16> %d"
          % (u[row16[0]]["scratch"], u[plain16[0]]["scratch"]))
