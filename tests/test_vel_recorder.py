"""VelLogRecorder / play_vel_log (uwvk.vel_log, CPU): vel_scenes.dense_events is
driven call by call into a recorder and, in parallel, into an OracleVelBatch;
the recorded log is the scene's (up to the row order of the shuffled samples)
and, played onto a second oracle, gives bitwise the direct one; play_vel_log
with a `skip` agrees with the hand-written loop; what a log cannot express
raises."""
import numpy as np
import pytest

import oracle_ctypes as O
import vel_scenes as VS
from uwvk import abi
from uwvk.vel_log import VelLogRecorder, play_vel_log

B = 3


def drive(fs, log):
    """the scene's calls, in run_log's order, on every object of fs"""
    for e in range(log["epochs"]):
        for f in fs:
            f.set_gyro(log["gyro"][e])
            f.set_efforts(log["efforts"][e])
            f.predict(log["dt"])
            if log["flags"][e] & abi.EV_DVL:
                f.update_dvl(log["dvl"][log["dvl_index"][e]], log["dvl_cov"])
            if log["flags"][e] & abi.EV_PRESSURE:
                f.update_pressure(log["pressure"][log["pressure_index"][e]], log["pressure_cov"])


def same(a, b):
    for u, v in zip(a.get_state(model=True), b.get_state(model=True)):
        np.testing.assert_array_equal(u, v)


def test_recorded_log_replays_bitwise():
    scene = VS.dense_events(B)
    direct, rec = VS.start(O.OracleVelBatch(B), scene), VelLogRecorder(B, scene["dt"])
    drive((direct, rec), scene)
    log = rec.log()
    assert log["epochs"] == scene["epochs"] and log["batch"] == B and log["dt"] == scene["dt"]
    np.testing.assert_array_equal(log["flags"], scene["flags"])
    for k in ("gyro", "efforts", "dvl_cov"):
        np.testing.assert_array_equal(log[k], scene[k])
    assert log["pressure_cov"] == scene["pressure_cov"]
    for kind, bit in (("dvl", abi.EV_DVL), ("pressure", abi.EV_PRESSURE)):
        at = np.flatnonzero(scene["flags"] & bit)
        np.testing.assert_array_equal(log[kind + "_index"][at], np.arange(len(at)))  # rows in event order
        assert (np.delete(log[kind + "_index"], at) == -1).all()
        np.testing.assert_array_equal(log[kind], scene[kind][scene[kind + "_index"][at]])
    played = VS.start(O.OracleVelBatch(B), scene)
    issued = play_vel_log(played, log)
    same(played, direct)
    counts = [(scene["flags"] & bit != 0).sum() for bit in (abi.EV_DVL, abi.EV_PRESSURE)]
    np.testing.assert_array_equal(issued, np.tile(counts, (B, 1)))
    native = VS.start(O.OracleVelBatch(B), scene)
    native.run_log({**scene, **log})  # the oracle's own driver loop on the recorded arrays
    same(native, direct)
    # adjacent ranges compose
    parts = VS.start(O.OracleVelBatch(B), scene)
    play_vel_log(parts, log, 0, 5)
    play_vel_log(parts, log, 5)
    same(parts, direct)


def test_play_with_skip_is_the_hand_written_loop():
    scene = VS.dense_events(1)
    E = scene["epochs"]
    assert scene["flags"][5] & abi.EV_DVL and scene["flags"][6] & abi.EV_PRESSURE
    hand, played = (VS.start(O.OracleVelBatch(1), scene) for _ in range(2))
    for e in range(E):
        if e != 4:
            hand.set_gyro(scene["gyro"][e])
            hand.set_efforts(scene["efforts"][e])
            hand.predict(scene["dt"])
        if scene["flags"][e] & abi.EV_DVL and e != 5:
            hand.update_dvl(scene["dvl"][scene["dvl_index"][e]], scene["dvl_cov"])
        if scene["flags"][e] & abi.EV_PRESSURE and e != 6:
            hand.update_pressure(scene["pressure"][scene["pressure_index"][e]], scene["pressure_cov"])
    issued = play_vel_log(played, scene, skip=dict(predict=[4], dvl={5: [0]}, pressure=[6]))
    same(played, hand)
    np.testing.assert_array_equal(issued, [[(scene["flags"] & abi.EV_DVL != 0).sum() - 1,
                                            (scene["flags"] & abi.EV_PRESSURE != 0).sum() - 1]])
    full = VS.start(O.OracleVelBatch(1), scene)
    play_vel_log(full, scene)
    assert (full.get_state()[0] != hand.get_state()[0]).any()


def test_play_with_masks_in_a_batch():
    """a mask per epoch leaves exactly the masked-out instances without that update"""
    scene = VS.dense_events(B)
    mask = np.array([1, 0, 1], np.uint8)
    played = VS.start(O.OracleVelBatch(B), scene)
    issued = play_vel_log(played, scene, skip=dict(dvl={5: mask}))
    n = (scene["flags"] & abi.EV_DVL != 0).sum()
    np.testing.assert_array_equal(issued[:, 0], [n, n - 1, n])
    for k in range(B):
        one = VS.take(scene, k)
        alone = VS.start(O.OracleVelBatch(1), one)
        play_vel_log(alone, one, skip=None if mask[k] else dict(dvl=[5]))
        for u, v in zip(alone.get_state(model=True), played.get_state(model=True)):
            np.testing.assert_array_equal(u[0], v[k])
    with pytest.raises(ValueError):
        play_vel_log(VS.start(O.OracleVelBatch(B), scene), scene, skip=dict(predict=[4]))


def test_what_a_log_cannot_express():
    scene = VS.dense_events(B)
    w, tau, z, R = scene["gyro"][0], scene["efforts"][0], scene["dvl"][0], scene["dvl_cov"]
    zp, Rp = scene["pressure"][0], scene["pressure_cov"]

    def opened():
        r = VelLogRecorder(B, 0.02)
        r.set_gyro(w)
        r.set_efforts(tau)
        r.predict(0.02)
        return r

    with pytest.raises(ValueError):
        VelLogRecorder(B, 0.02).predict(0.02)          # no inputs yet
    with pytest.raises(ValueError):
        opened().predict(0.01)                         # dt changes
    r = VelLogRecorder(B, 0.02)
    r.set_gyro(w)
    r.set_efforts(tau)
    with pytest.raises(ValueError):
        r.update_dvl(z, R)                             # before the first predict
    with pytest.raises(ValueError):
        opened().update_dvl(z, R, mask=np.ones(B, np.uint8))
    with pytest.raises(ValueError):
        opened().update_dvl(z, cov=np.tile(R, (B, 1, 1)))
    r = opened()
    r.update_dvl(z, R)
    with pytest.raises(ValueError):
        r.update_dvl(z, R)                             # twice in one epoch
    r.update_pressure(zp, Rp)
    r.predict(0.02)
    with pytest.raises(ValueError):
        r.update_dvl(z, 2 * R)                         # the covariance changes
    r.update_pressure(zp, Rp)
    with pytest.raises(ValueError):
        r.update_dvl(z, R)                             # DVL after the epoch's pressure
    log = r.log()
    assert log["epochs"] == 2 and list(log["flags"]) == [6, 4] and log["dvl"].shape == (1, B, 3)
    empty = VelLogRecorder(B, 0.02).log()
    assert empty["epochs"] == 0 and empty["gyro"].shape == (0, B, 3) and empty["dvl"].shape == (0, B, 3)
