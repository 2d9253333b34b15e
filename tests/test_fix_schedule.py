"""Position-fix ingestion (uwvk_schedule_fixes, uwvk.mission.schedule_fixes and
the xy / z / geo arguments of build_pose_log) on the CPU: the native placement
is held bit-exact to a numpy restatement of the rule of uwvk_schedule_streams
(release at the first epoch at or after the stamp, per-sensor queue, drops
counted), and a mission with fixes survives save / load."""
import os

import numpy as np
import pytest

from uwvk import abi, engine, mission, synth

BITS = (abi.FIX_XY, abi.FIX_Z, abi.FIX_GEO)


def ref_place(imu, t, eps):
    """numpy restatement of the per-sensor placement rule."""
    E = len(imu)
    idx = np.full(E, -1, np.int32)
    nxt, row, dropped = 0, 0, 0
    for ts in t:
        if not ts >= imu[0] - eps:
            dropped += 1
            continue
        e = int(np.searchsorted(imu, ts - eps, side="left"))
        at = max(e, nxt)
        if at >= E:
            dropped += 1
            continue
        idx[at] = row
        row += 1
        nxt = at + 1
    return idx, dropped


def test_schedule_fixes_matches_numpy_restatement():
    rng = np.random.default_rng(11)
    E, dt = 2000, 1e-3
    imu = 20.0 + np.arange(E) * dt + rng.uniform(-2e-5, 2e-5, E)
    streams = []
    for n in (25, 40, 9):
        t = np.sort(rng.uniform(imu[0] - 0.01, imu[-1] + 0.01, n))
        t[4:6] = t[4]            # two samples in one epoch: the second is queued
        t[-2:] = imu[-1] + 0.005  # past the last epoch: dropped
        t[0] = imu[0] - 0.005     # before the first stamp: dropped
        streams.append(t)
    s = mission.schedule_fixes(imu, *streams, time_epsilon=1e-9)
    flags = np.zeros(E, np.uint32)
    for j, (k, bit) in enumerate(zip(mission.FIXES, BITS)):
        idx, dropped = ref_place(imu, streams[j], 1e-9)
        np.testing.assert_array_equal(s[k + "_index"], idx)
        assert s["dropped"][j] == dropped >= 3 and s["kept"][j] == len(streams[j]) - dropped
        flags[idx >= 0] |= bit
        at = np.flatnonzero(idx >= 0)
        np.testing.assert_array_equal(idx[at], np.arange(len(at)))  # rows are the kept samples, in order
    np.testing.assert_array_equal(s["flags"], flags)
    assert s["flags"].dtype == np.uint32 and not (s["flags"] & ~np.uint32(7)).any()


def test_two_samples_in_one_epoch_are_queued():
    imu = np.arange(10) * 0.1
    s = mission.schedule_fixes(imu, xy_t=[0.31, 0.32, 0.33], z_t=[0.31])
    np.testing.assert_array_equal(np.flatnonzero(s["xy_index"] >= 0), [4, 5, 6])
    np.testing.assert_array_equal(s["xy_index"][4:7], [0, 1, 2])
    np.testing.assert_array_equal(np.flatnonzero(s["z_index"] >= 0), [4])
    assert s["flags"][4] == abi.FIX_XY | abi.FIX_Z and s["flags"][5] == abi.FIX_XY
    assert (s["geo_index"] == -1).all()
    assert list(s["kept"]) == [3, 1, 0] and not s["dropped"].any()


def test_early_and_late_samples_are_dropped_and_counted():
    imu = 5.0 + np.arange(4) * 0.1
    s = mission.schedule_fixes(imu, xy_t=[4.0, 5.0, 5.21, 5.22, 9.0], geo_t=[1.0, 2.0])
    # 4.0 early; 5.0 -> epoch 0; 5.21 -> epoch 3 (the last); 5.22 queued past it; 9.0 late
    np.testing.assert_array_equal(s["xy_index"], [0, -1, -1, 1])
    assert list(s["kept"]) == [2, 0, 0] and list(s["dropped"]) == [3, 0, 2]
    np.testing.assert_array_equal(s["flags"], [abi.FIX_XY, 0, 0, abi.FIX_XY])


def test_schedule_fixes_rejects_bad_streams():
    imu = np.arange(100) * 1e-3
    with pytest.raises(engine.UWVKError) as e:
        mission.schedule_fixes(imu, xy_t=[0.05, 0.01])  # not ascending
    assert e.value.code == 1
    with pytest.raises(engine.UWVKError) as e:
        mission.schedule_fixes(imu, geo_t=[0.01, np.nan, 0.02])
    assert e.value.code == 1
    with pytest.raises(engine.UWVKError) as e:
        mission.schedule_fixes(imu[::-1], z_t=[0.01])
    assert e.value.code == 1
    with pytest.raises(engine.UWVKError) as e:
        mission.schedule_fixes(imu, z_t=[0.01], time_epsilon=-1.0)
    assert e.value.code == 1


def _mission(batch, epochs, with_fixes):
    log = synth.make_pose_log(batch, epochs, "C3")
    E, dt = log["epochs"], log["dt"]
    imu = np.arange(1, E + 1) * dt
    k = np.arange(1, E + 1)
    dvl_t = k[(log["flags"] & abi.EV_DVL) != 0] * dt
    kw = {}
    if with_fixes:
        rng = np.random.default_rng(5)
        xy_t = np.array([-1.0, imu[3], imu[3] + 1e-7, imu[40] - 0.4 * dt, imu[-1] + 1.0])  # early, two queued, one late
        kw = dict(xy=(xy_t, rng.normal(size=(5, batch, 2)), np.diag([0.25, 0.36])),
                  z=(imu[[10, 40]], rng.normal(size=(2,)), 0.04),  # broadcast to the batch
                  geo=(imu[[99]], rng.normal(size=(1, 2)), np.eye(2) * 1e-12), gps_in_body=(0.1, 0.0, -0.5))
    return mission.build_pose_log(batch, imu, log["gyro"], log["acc"], log["acc_cov"],
                                  dvl=(dvl_t, log["dvl"], log["dvl_cov"]), **kw), kw


def test_build_pose_log_with_fixes_and_save_load(tmp_path):
    B = 3
    m, kw = _mission(B, 100, True)
    fx = m["fixes"]
    np.testing.assert_array_equal(np.flatnonzero(fx["xy_index"] >= 0), [3, 4, 40])
    assert list(fx["kept"]) == [3, 2, 1] and list(fx["dropped"]) == [2, 0, 0]
    # the unplaced rows (the early first and the late last sample) are gone
    np.testing.assert_array_equal(fx["xy"], kw["xy"][1][1:4])
    assert fx["xy"].shape == (3, B, 2) and fx["z"].shape == (2, B) and fx["geo"].shape == (1, B, 2)
    np.testing.assert_array_equal(fx["z"], np.repeat(kw["z"][1][:, None], B, 1))
    assert fx["flags"][40] == abi.FIX_XY | abi.FIX_Z and fx["flags"][99] == abi.FIX_GEO
    np.testing.assert_array_equal(fx["gps_in_body"], [0.1, 0.0, -0.5])
    p = os.path.join(tmp_path, "m.npz")
    mission.save(p, m)
    r = mission.load(p)
    for k in mission._ARRAYS:
        np.testing.assert_array_equal(np.asarray(r[k]), np.asarray(m[k]))
    assert sorted(r["fixes"]) == sorted(fx)
    for k in fx:
        np.testing.assert_array_equal(np.asarray(r["fixes"][k]), np.asarray(fx[k]))
        assert np.asarray(r["fixes"][k]).dtype == np.asarray(fx[k]).dtype, k


def test_build_pose_log_without_fixes_is_unchanged(tmp_path):
    m, _ = _mission(2, 60, False)
    assert "fixes" not in m
    p = os.path.join(tmp_path, "m.npz")
    mission.save(p, m)
    with np.load(p) as z:
        assert not [k for k in z.files if k.startswith("fixes")]
    r = mission.load(p)
    assert "fixes" not in r
    for k in mission._ARRAYS:
        np.testing.assert_array_equal(np.asarray(r[k]), np.asarray(m[k]))
