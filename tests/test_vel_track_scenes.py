"""The scenes of tests/test_gpu_vel_track.py are meaningful before anything runs
on a GPU (CPU, the C oracle): skipping the predict, the DVL update or the
pressure update that each screening case of tests/vel_track_scenes.py leaves
out moves that instance's result by at least 1e-3 sigma (the convention of
tests/test_pose_model_scenes.py), so a kernel that did not skip, or skipped
something else, cannot pass unnoticed; the poisoned logs differ from the clean
one in that one entry alone; the clean scenes raise no status."""
import numpy as np
import pytest

import oracle_ctypes as O
import vel_scenes as VS
import vel_track_scenes as TS
from uwvk import abi, synth
from uwvk.vel_log import play_vel_log

MIN_SHIFT = 1e-3  # in the oracle's sigma


def played(log, skip=None):
    o = VS.start(O.OracleVelBatch(1), log)
    play_vel_log(o, log, skip=skip)
    return o.get_state(model=True)


def shift(a, b):
    """largest |x_a - x_b| in b's sigma"""
    return float(np.max(np.abs(a[0] - b[0]) / np.sqrt(np.diagonal(b[1], axis1=1, axis2=2))))


@pytest.mark.parametrize("case", sorted(TS.CASES))
def test_the_skipped_step_matters(case):
    c = TS.CASES[case]
    one = VS.take(TS.clean(), TS.J)
    full, skipped = played(one), played(one, c["skip"])
    s = shift(skipped, full)
    print("%s: skipping moves instance %d by %.3g sigma" % (case, TS.J, s))
    assert s >= MIN_SHIFT, (case, s)
    assert np.isfinite(skipped[0]).all() and np.isfinite(skipped[1]).all()


def test_the_pair_of_skipped_predicts_matters():
    log = TS.clean()
    for j, e in TS.PAIR:
        one = VS.take(log, j)
        s = shift(played(one, dict(predict=[e])), played(one))
        print("instance %d without the predict of epoch %d: %.3g sigma" % (j, e, s))
        assert s >= MIN_SHIFT, (j, e, s)
    # and the two epochs are not interchangeable
    one = VS.take(log, TS.PAIR[0][0])
    assert shift(played(one, dict(predict=[TS.PAIR[0][1]])), played(one, dict(predict=[TS.PAIR[1][1]]))) >= MIN_SHIFT


@pytest.mark.parametrize("case", sorted(TS.CASES))
def test_poison_touches_one_entry(case):
    c, log = TS.CASES[case], TS.clean()
    bad = TS.poison(log, case)
    for k in ("flags", "gyro", "efforts", "dvl_index", "dvl", "pressure_index", "pressure"):
        diff = ~((log[k] == bad[k]) | (np.isnan(log[k]) & np.isnan(bad[k]))) if k == c["array"] else log[k] != bad[k]
        assert diff.sum() == (k == c["array"]), (k, diff.sum())
    assert not np.isfinite(bad[c["array"]]).all() and np.isfinite(log[c["array"]]).all()
    assert 0 < TS.J < TS.B - 1 and TS.J // 4 == 1 and TS.J % 4 == 1  # second wave, second row of the row kernel
    if c["array"] in ("gyro", "efforts"):
        assert log["flags"][c["epoch"]]  # an event epoch: its updates still run
    else:
        assert c["epoch"] == log["epochs"] - 1 or c["epoch"] + 2 < log["epochs"]


def test_clean_scenes_raise_no_status():
    """OracleVelBatch.run_log raises on any status but UWVK_OK (UWVK_ENOTPD included)"""
    for log in (TS.clean(), VS.tilted(5), VS.dense_events(13)):
        assert np.isfinite(log["gyro"]).all() and np.isfinite(log["dvl"]).all()
        VS.start(O.OracleVelBatch(log["batch"]), log).run_log(log)
    log = VS.add_events(synth.make_vel_log(5, 4100), [4095, 4096])
    assert (log["flags"][[4095, 4096]] == abi.EV_DVL | abi.EV_PRESSURE).all()
    o = VS.start(O.OracleVelBatch(5), log)
    o.run_log(log, 4000, 100)  # the stretch around the launch boundary
