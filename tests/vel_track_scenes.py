"""The screening cases of uwvk_vel_run_log_track, shared by
tests/test_vel_track_scenes.py (CPU: each case matters on the oracle) and
tests/test_gpu_vel_track.py (the HIP kernels).  All on vel_scenes.dense_events
at batch 9 with the bad sample in instance 5: the second row of the second wave
of the 16-lane-row kernel (instances 4..7 share that wave).

A case: where the non-finite value goes (array, epoch, component, value) and the
`skip` of uwvk.vel_log.play_vel_log that replays, on a batch of one, what the
screened run does for that instance."""
import numpy as np

import vel_scenes as VS
from uwvk import abi

B, J = 9, 5

CASES = dict(
    dvl_nan=dict(array="dvl", epoch=5, comp=1, value=np.nan, skip=dict(dvl=[5]), applied=(1, 0)),
    pressure_inf=dict(array="pressure", epoch=6, comp=None, value=np.inf, skip=dict(pressure=[6]), applied=(0, 1)),
    # the documented hole of the plain run: a bad sample in the run's last step
    dvl_nan_last_epoch=dict(array="dvl", epoch=11, comp=2, value=np.nan, skip=dict(dvl=[11]), applied=(1, 0)),
    gyro_nan=dict(array="gyro", epoch=4, comp=2, value=np.nan, skip=dict(predict=[4]), applied=(0, 0)),
    efforts_inf=dict(array="efforts", epoch=8, comp=0, value=np.inf, skip=dict(predict=[8]), applied=(0, 0)),
)
UPDATE_CASES = ("dvl_nan", "pressure_inf", "dvl_nan_last_epoch")
INPUT_CASES = ("gyro_nan", "efforts_inf")


def clean():
    return VS.dense_events(B)


def poison(log, case, j=J):
    """a copy of `log` with the case's non-finite value in instance j"""
    c = CASES[case] if isinstance(case, str) else case
    out = dict(log)
    a = log[c["array"]].copy()
    if c["array"] in ("gyro", "efforts"):
        a[c["epoch"], j, c["comp"]] = c["value"]
    elif c["array"] == "dvl":
        assert log["flags"][c["epoch"]] & abi.EV_DVL
        a[log["dvl_index"][c["epoch"]], j, c["comp"]] = c["value"]
    else:
        assert log["flags"][c["epoch"]] & abi.EV_PRESSURE
        a[log["pressure_index"][c["epoch"]], j] = c["value"]
    out[c["array"]] = a
    return out


# two instances of one wave of the row kernel skipping their predict at different epochs
PAIR = ((4, 3), (5, 4))  # (instance, epoch)


def poison_pair(log):
    out = dict(log)
    out["gyro"] = log["gyro"].copy()
    for j, e in PAIR:
        out["gyro"][e, j, 0] = np.nan
    return out
