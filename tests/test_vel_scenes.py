"""The VelocityUKF scenes of tests/vel_scenes.py are valid before anything
runs on a GPU: on each the C oracle and the numpy twin agree to the twin
tolerance, no step fails its factorisation, and the property each scene is
built for holds (the event pattern, the tilted quaternion, the mixed mean
iteration counts inside every group of 4 instances)."""
import numpy as np
import pytest

import numpy_twin as T
import oracle_ctypes as O
import vel_scenes as VS
from helpers import cov_err
from uwvk import abi

TOL = 1e-10  # oracle against twin, in the oracle's sigma (tests/test_oracle_twin.py)
B = 8


def twin(log, i):
    t = T.VelTwin(log["x0"][i], log["P0"][i], T.UWV.from_abi(VS.uwv(log)))
    if log["Q"] is not None:
        t.set_process_noise(log["Q"])
    t.set_gyro(log["gyro"][0][i])
    return t


def twin_run(t, log, i):
    for e in range(log["epochs"]):
        t.set_gyro(log["gyro"][e][i])
        t.set_efforts(log["efforts"][e][i])
        t.predict(log["dt"])  # numpy's Cholesky raises on a non-positive pivot
        if log["flags"][e] & abi.EV_DVL:
            t.update_dvl(log["dvl"][log["dvl_index"][e]][i], log["dvl_cov"])
        if log["flags"][e] & abi.EV_PRESSURE:
            t.update_pressure(log["pressure"][log["pressure_index"][e]][i], log["pressure_cov"])
    return t


@pytest.mark.parametrize("scene", sorted(VS.SCENES))
def test_oracle_matches_twin(scene):
    log = VS.SCENES[scene](B)
    o = VS.start(O.OracleVelBatch(B), log)
    o.run_log(log)  # raises on any status but UWVK_OK (UWVK_ENOTPD included)
    steps = VS.start(O.OracleVelBatch(B), log)
    steps.run_log_steps(log)  # the per-call API asserts UWVK_OK at every step
    xo, Po, mo = o.get_state(model=True)
    for a, b in zip(steps.get_state(model=True), (xo, Po, mo)):
        np.testing.assert_array_equal(a, b)
    sd = np.sqrt(np.diagonal(Po, axis1=1, axis2=2))
    for i in range(B):
        t = twin_run(twin(log, i), log, i)
        es = np.max(np.abs(t.mu - xo[i]) / sd[i])
        ec = cov_err(t.P[None], Po[i:i + 1]).max()
        print("%s instance %d: state %.3g cov %.3g model %.3g" % (scene, i, es, ec, np.abs(t.model - mo[i]).max()))
        assert es < TOL and ec < TOL, (i, es, ec)
        np.testing.assert_allclose(t.model, mo[i], rtol=0, atol=1e-12)


def test_instances_do_not_depend_on_the_batch():
    """instance i of a batch is instance 0 of the batch that starts at i"""
    for make in VS.SCENES.values():
        a, b = make(7), make(2, first=5)
        for k in ("gyro", "efforts", "dvl", "pressure"):
            np.testing.assert_array_equal(a[k][:, 5:7], b[k])
        np.testing.assert_array_equal(a["P0"][5:7], b["P0"])
        one = VS.take(a, 5)
        np.testing.assert_array_equal(one["dvl"], b["dvl"][:, :1])
        assert one["batch"] == 1 and one["x0"].shape == (1, 4)


def test_dense_events_pattern():
    log = VS.dense_events(3)
    f, E = log["flags"], log["epochs"]
    dvl, prs = (f & abi.EV_DVL) != 0, (f & abi.EV_PRESSURE) != 0
    assert E == 12 and f[0] and f[-1] and (f == 0).any()
    np.testing.assert_array_equal(np.diff(np.flatnonzero(dvl)), 3)
    np.testing.assert_array_equal(np.diff(np.flatnonzero(prs)), 2)
    np.testing.assert_array_equal(np.diff(np.flatnonzero(dvl & prs)), 6)
    for index, sel, rows in ((log["dvl_index"], dvl, log["dvl"]), (log["pressure_index"], prs, log["pressure"])):
        used = index[sel]
        assert (index[~sel] == -1).all() and len(set(used)) == sel.sum()
        # neither the epoch nor the event's ordinal: at most one event coincides with either
        assert (used == np.arange(E)[sel]).sum() <= 1 and (used == np.arange(sel.sum())).sum() <= 1
        assert used.min() >= 0 and used.max() < len(rows)
        assert (np.diff(used) < 0).all()  # stored in reverse event order: a sorted read is wrong everywhere


def test_tilted_quaternion_and_inputs():
    log = VS.tilted(B)
    o = VS.start(O.OracleVelBatch(B), log)
    o.run_log(log)
    q = o.get_state(model=True)[2][:, 3:7]
    assert np.abs(q).min() >= 0.1, q
    o = VS.start(O.OracleVelBatch(B), log)
    o.run_log(log, 0, 50)
    assert np.abs(o.get_state(model=True)[2][:, 3:7]).min() >= 0.1
    for S in (log["dvl_cov"], log["Q"], *log["P0"]):
        assert np.allclose(S, S.T) and np.linalg.eigvalsh(S).min() > 0
        assert (np.abs(S[~np.eye(len(S), dtype=bool)]) > 1e-3 * np.abs(np.diag(S)).min()).all()  # full
    assert np.abs(log["P0"][1:] - log["P0"][:1]).max() > 1e-4  # differs per instance
    u = VS.uwv(log)
    assert u.weight != u.buoyancy and all(u.distance_body2centerofgravity[:])


def test_mixed_spread_splits_every_group_of_four():
    """The first predict's first-pass shift |mean(X - X_0)| of the iterative mean
    (ukfom's threshold: 1e-6) is above the threshold for some instances and
    below it for others of each group of 4: the filters that share a wave of
    the 16-lane-row kernel leave the mean loop after different pass counts."""
    log = VS.mixed_spread(B)
    shift = np.empty(B)
    for i in range(B):
        t = twin(log, i)
        t.set_gyro(log["gyro"][0][i])
        t.set_efforts(log["efforts"][0][i])
        X = t.process(T.sigma_points(t.lay, t.mu, t.P), log["dt"])
        shift[i] = np.linalg.norm((X - X[0]).mean(axis=0))
    print("first-pass shifts", shift)
    g = shift.reshape(-1, 4)
    assert (g.max(axis=1) > 1e-5).all() and (g.min(axis=1) < 1e-7).all(), g  # a decade clear on both sides
