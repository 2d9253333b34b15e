"""Delayed XY ingestion (uwvk_schedule_delayed, uwvk.mission.schedule_delayed and
the delayed_xy argument of build_pose_log) on the CPU: the native placement is
held bit-exact to a Python restatement of the rule (latch epoch L: the first
epoch at or after the stamp; arrival epoch A: the largest of the first epoch at
or after the arrival, L + 1 and the next free arrival epoch; early and late
samples dropped and counted), and a mission with delayed rows survives
save / load."""
import os

import numpy as np
import pytest

from uwvk import engine, mission, synth


def ref_place(imu, stamp, arrival, eps):
    """Python restatement of the placement rule of uwvk_schedule_delayed."""
    E = len(imu)
    index = np.full(E, -1, np.int32)
    latch, nxt, dropped = [], 0, 0
    for ts, ta in zip(stamp, arrival):
        if not ts >= imu[0] - eps:
            dropped += 1
            continue
        L = int(np.searchsorted(imu, ts - eps, side="left"))
        A = max(int(np.searchsorted(imu, ta - eps, side="left")), L + 1, nxt)
        if A >= E:
            dropped += 1
            continue
        index[A] = len(latch)
        latch.append(L)
        nxt = A + 1
    return index, np.array(latch, np.int32), dropped


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_schedule_delayed_matches_restatement(seed):
    rng = np.random.default_rng(seed)
    E, dt = 2000, 1e-3
    imu = 20.0 + np.arange(E) * dt + rng.uniform(-2e-5, 2e-5, E)
    n = 60
    stamp = np.sort(np.concatenate([rng.uniform(imu[0] - 0.02, imu[-1] + 0.01, n - 3),
                                    [imu[0] - 0.01, imu[-1] + 0.005, imu[-1] + 0.006]]))  # one early, two late
    # delays from none to many epochs; ascending arrivals (a later sample never overtakes)
    arrival = np.maximum.accumulate(stamp + rng.choice([0.0, 2e-4, 5e-3, 0.08], n))
    s = mission.schedule_delayed(imu, stamp, arrival, time_epsilon=1e-9)
    index, latch, dropped = ref_place(imu, stamp, arrival, 1e-9)
    np.testing.assert_array_equal(s["index"], index)
    np.testing.assert_array_equal(s["latch_epoch"], latch)
    assert s["dropped"] == dropped >= 2 and s["kept"] == n - dropped == len(latch)
    at = np.flatnonzero(index >= 0)
    np.testing.assert_array_equal(index[at], np.arange(len(at)))  # rows are the kept samples, in order
    assert (at > latch).all() and s["index"].dtype == np.int32 and s["latch_epoch"].dtype == np.int32


def test_stamp_and_arrival_in_one_interval_arrive_one_epoch_later():
    imu = np.arange(10) * 0.1
    s = mission.schedule_delayed(imu, [0.31], [0.35])
    assert list(s["latch_epoch"]) == [4] and list(np.flatnonzero(s["index"] >= 0)) == [5]
    s = mission.schedule_delayed(imu, [0.31], [0.31])  # no delay at all: still L + 1
    assert list(s["latch_epoch"]) == [4] and s["index"][5] == 0 and (s["kept"], s["dropped"]) == (1, 0)


def test_two_arrivals_in_one_epoch_are_queued():
    imu = np.arange(10) * 0.1
    s = mission.schedule_delayed(imu, [0.11, 0.21, 0.22], [0.55, 0.56, 0.57])
    np.testing.assert_array_equal(s["latch_epoch"], [2, 3, 3])  # two rows share a latch epoch
    np.testing.assert_array_equal(np.flatnonzero(s["index"] >= 0), [6, 7, 8])
    np.testing.assert_array_equal(s["index"][6:9], [0, 1, 2])
    assert (s["kept"], s["dropped"]) == (3, 0)


def test_leading_and_trailing_drops():
    imu = 5.0 + np.arange(4) * 0.1
    # stamped early; kept (L 0, A 2); latch on the last epoch, nowhere to arrive; arrival past the end
    s = mission.schedule_delayed(imu, [4.0, 5.0, 5.3, 5.31], [4.5, 5.15, 5.3, 9.0])
    np.testing.assert_array_equal(s["index"], [-1, -1, 0, -1])
    np.testing.assert_array_equal(s["latch_epoch"], [0])
    assert (s["kept"], s["dropped"]) == (1, 3)
    s = mission.schedule_delayed(imu, [], [])
    assert (s["kept"], s["dropped"]) == (0, 0) and (s["index"] == -1).all() and len(s["latch_epoch"]) == 0


def test_schedule_delayed_rejects_bad_streams():
    imu = np.arange(100) * 1e-3
    bad = dict(arrival_before_stamp=([0.01, 0.02], [0.03, 0.015]), unsorted_stamps=([0.02, 0.01], [0.03, 0.04]),
               unsorted_arrivals=([0.01, 0.02], [0.05, 0.04]), nan_stamp=([0.01, np.nan], [0.02, 0.03]))
    for name, (st, at) in bad.items():
        with pytest.raises(engine.UWVKError) as e:
            mission.schedule_delayed(imu, st, at)
        assert e.value.code == 1, name
    with pytest.raises(engine.UWVKError) as e:
        mission.schedule_delayed(imu[::-1], [0.01], [0.02])
    assert e.value.code == 1
    with pytest.raises(engine.UWVKError) as e:
        mission.schedule_delayed(imu, [0.01], [0.02], time_epsilon=-1.0)
    assert e.value.code == 1


def _mission(batch, epochs, with_delayed):
    log = synth.make_pose_log(batch, epochs, "C3")
    E, dt = log["epochs"], log["dt"]
    imu = np.arange(1, E + 1) * dt
    kw = {}
    if with_delayed:
        rng = np.random.default_rng(6)
        stamp = np.array([-1.0, imu[3], imu[20] - 0.4 * dt, imu[20], imu[-1]])  # early, ..., no epoch left to arrive
        arrival = np.array([0.5 * dt, imu[10], imu[50], imu[50], imu[-1] + 1.0])
        kw = dict(delayed_xy=(stamp, arrival, rng.normal(size=(5, batch, 2)), np.diag([0.25, 0.36])))
    return mission.build_pose_log(batch, imu, log["gyro"], log["acc"], log["acc_cov"], **kw), kw


def test_build_pose_log_with_delayed_and_save_load(tmp_path):
    B = 3
    m, kw = _mission(B, 100, True)
    d = m["delayed"]
    np.testing.assert_array_equal(d["latch_epoch"], [3, 20, 20])
    np.testing.assert_array_equal(np.flatnonzero(d["index"] >= 0), [10, 50, 51])
    assert (int(d["kept"]), int(d["dropped"])) == (3, 2)
    np.testing.assert_array_equal(d["xy"], kw["delayed_xy"][2][1:4])  # the dropped first and last rows are gone
    assert d["xy"].shape == (3, B, 2) and d["xy_cov"].shape == (2, 2) and "fixes" not in m
    p = os.path.join(tmp_path, "m.npz")
    mission.save(p, m)
    r = mission.load(p)
    for k in mission._ARRAYS:
        np.testing.assert_array_equal(np.asarray(r[k]), np.asarray(m[k]))
    assert sorted(r["delayed"]) == sorted(d) and "fixes" not in r
    for k in d:
        np.testing.assert_array_equal(np.asarray(r["delayed"][k]), np.asarray(d[k]))
        assert np.asarray(r["delayed"][k]).dtype == np.asarray(d[k]).dtype, k


def test_delayed_xy_broadcasts_to_the_batch():
    B = 4
    log = synth.make_pose_log(B, 30, "C3")
    imu = np.arange(1, 31) * log["dt"]
    mu = np.array([[1.0, 2.0], [3.0, 4.0]])
    m = mission.build_pose_log(B, imu, log["gyro"], log["acc"], log["acc_cov"],
                               delayed_xy=(imu[[2, 5]], imu[[9, 9]], mu, np.eye(2)))
    np.testing.assert_array_equal(m["delayed"]["xy"], np.repeat(mu[:, None], B, 1))
    np.testing.assert_array_equal(np.flatnonzero(m["delayed"]["index"] >= 0), [9, 10])


def test_a_file_without_delayed_rows_still_loads(tmp_path):
    m, _ = _mission(2, 60, False)
    assert "delayed" not in m
    p = os.path.join(tmp_path, "m.npz")
    mission.save(p, m)
    with np.load(p) as z:
        assert not [k for k in z.files if k.startswith("delayed")]
    r = mission.load(p)
    assert "delayed" not in r and "fixes" not in r
    for k in mission._ARRAYS:
        np.testing.assert_array_equal(np.asarray(r[k]), np.asarray(m[k]))
