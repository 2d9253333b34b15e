"""The scenes of tests/pose_config_scenes.py (a configuration and a sensor set-up
in which no two numbers are alike) are valid before anything runs on a GPU.

 * the configuration is what it claims: every group of numbers the default
   leaves equal is pairwise >= 1.5x apart, every tau >= 100 dt;
 * the conditions the scenes are built for hold: SPD covariances with
   correlations of 0.2 .. 0.6, a pressure lever arm, 1 / 4 / 8 cells with
   non-monotone weights, every DVL, pressure and efforts update and every ADCP
   cell accepted (the oracle's counts), |v_z| >= 0.4 in the dive, the halves of
   every pair wave of far() on different sides of the latitude branch;
 * the C oracle and the numpy twin agree on every scene, both layouts and
   both SO3 sides, to the bounds of tests/test_pose_model_scenes.py: 1e-10 for
   init, a predict and single calls, 1e-8 over a log;
 * each feature matters: reverted, permuted or swapped, it moves the oracle's
   result by at least 1e-3 (the larger of mean in sigma and covariance in
   sqrt(P_ii P_jj), minimum over instances and layouts); where a layout cannot
   see it (the parameter taus and instabilities at 26 DOF) the result is
   bitwise the same.

Measured figures: DESIGN.md section 10."""
import numpy as np
import pytest

import numpy_twin as T
import oracle_ctypes as O
import pose_config_scenes as CS
import pose_gate_scenes as GS
from helpers import cov_err, state_err
from test_pose_model_scenes import err, twin_run_log
from uwvk import abi, synth

TOL = 1e-10      # oracle against twin: init, a predict, single calls (tests/test_pose_model_scenes.py)
TOL_LOG = 1e-8   # oracle against twin over a log
MATTERS = 1e-3   # 1e6 x the single-step tolerance of the GPU tests
B = 2
DOFS = (53, 26)


@pytest.fixture(params=["right", "left"])
def side(request):
    right = request.param == "right"
    prev = T.SO3_RIGHT
    T.SO3_RIGHT = right
    with O.so3_side(right):
        yield request.param
    T.SO3_RIGHT = prev


# ---- the configuration is what it claims -------------------------------------------
def test_config_is_distinct():
    c, d = CS.distinct_config(), synth.default_pose_config()
    for name, v in CS.config_numbers(c).items():
        v = np.sort(np.asarray(v, float))
        assert (v[1:] / v[:-1] >= 1.5 - 1e-12).all(), (name, v)
    rw = np.array(c.rotation_rate.randomwalk[:])
    assert rw[1] / rw[0] >= 6 - 1e-12 and rw[2] / rw[0] >= 15 - 1e-12
    assert min(CS.TAUS.values()) >= 100 * CS.COARSE_DT
    assert np.all(c.rotation_rate.bias_offset[:]) and np.all(c.acceleration.bias_offset[:])
    for a, b in ((c.water_velocity, d.water_velocity), (c.hydrostatics, d.hydrostatics)):
        for k in ("limits", "adcp_bias_limits", "scale", "water_density", "water_density_limits",
                  "atmospheric_pressure"):
            if hasattr(a, k):
                assert getattr(a, k) != getattr(b, k), k
    assert c.location.latitude < -0.5
    names = [n for n, _, _ in CS.alterations()]
    assert len(set(names)) == len(names) >= 9
    for n, alt, _ in CS.alterations():  # one feature each: the altered config is another config
        assert bytes(alt) != bytes(c), n


def test_sensor_setup_conditions():
    for name, S in list(CS.FULL_COVS.items()) + [("xy", CS.XY_COV), ("geo", CS.GEO_COV)]:
        np.linalg.cholesky(S)
        np.testing.assert_array_equal(S, S.T)
        sd = np.sqrt(np.diag(S))
        corr = (S / np.outer(sd, sd))[~np.eye(len(S), dtype=bool)]
        assert (corr >= 0.2 - 1e-12).all() and (corr <= 0.6 + 1e-12).all(), (name, corr)
        assert sd.max() / sd.min() >= 1.5, name
        for i in range(6):
            Ri = CS.per_instance(S, i)
            np.linalg.cholesky(Ri)
            assert not np.allclose(Ri / Ri[0, 0], S / S[0, 0], rtol=1e-3)
    assert CS.XY_COV[1, 1] / CS.XY_COV[0, 0] == pytest.approx(4.0) and CS.PRESSURE_LEVER.all() and CS.GEO_LEVER.all()
    for cells, w in CS.CELL_WEIGHTS.items():
        assert len(w) == cells and (w >= 0).all() and (w <= 1).all()
        if cells > 1:
            assert (np.diff(w) > 0).any() and (np.diff(w) < 0).any()
    log = CS.full_log(3, 40)
    one = CS.full_log(1, 40, first=2)
    for k in ("gyro", "acc", "dvl", "efforts"):
        np.testing.assert_array_equal(one[k][:, 0], log[k][:, 2])


def test_far_branch_sides():
    """B = 6: the halves of every pair wave on different sides of the 64 km branch"""
    log = CS.far(CS.full_log(6, 4))
    lib = CS.library_branch(log["pos0"][:, 0])
    assert sorted(set(CS.far_shift(6))) == sorted(CS.FAR_SHIFTS)
    assert sum(lib[2 * u] != lib[2 * u + 1] for u in range(3)) >= 2
    # a metre of prior (the sigma points' spread) puts no point on the other side
    assert (np.abs(np.abs(log["pos0"][:, 0] / T.radii(CS.LATITUDE)[0]) - CS.BRANCH_AT) > 1e-4).all()
    np.testing.assert_array_equal(lib, [False, True, False, True, True, False])


# ---- oracle against twin -----------------------------------------------------------------
@pytest.mark.parametrize("dof", DOFS)
def test_init_noise_and_predict(dof, side):
    """init_from_config with the mounting, Q from the config (the orientation
    block turned by the mounting), one predict from the tilted attitude (turned
    again by the attitude): the predict shows Q"""
    log = CS.full_log(B, 4, dof)
    o = CS.start(O.OraclePoseBatch(B, dof), log)
    ts = CS.twins_of(log, dof)
    xo, Po = o.get_state()
    for i, t in enumerate(ts):
        np.testing.assert_allclose(t.mu, xo[i], rtol=0, atol=1e-15)
        np.testing.assert_allclose(t.P, Po[i], rtol=0, atol=1e-15 * np.abs(Po[i]).max())
        q = t.Q[3:6, 3:6]
        assert np.abs(q[~np.eye(3, dtype=bool)]).max() > 0.05 * np.abs(np.diag(q)).max()  # anisotropic, turned
    o.set_rotation_rate(log["gyro"][0])
    o.predict(log["dt"])
    for i, t in enumerate(ts):
        t.w = log["gyro"][0][i]
        t.predict(log["dt"])
    e = err(o, ts, dof)
    print("init + predict dof %d %s oracle against twin: mean %.3g cov %.3g" % (dof, side, e[0], e[1]))
    assert max(e) < TOL, e


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_instance"])
@pytest.mark.parametrize("dof", DOFS)
def test_single_calls(dof, shared, side):
    log, calls = CS.single_calls(B, dof, shared=shared, right=side == "right")
    worst = {}
    for name, kind, mu, cov, extra, vo in calls:
        o = CS.single_state(O.OraclePoseBatch(B, dof), log)
        ts = CS.twins_of(log, dof)
        for i, t in enumerate(ts):
            for e in range(CS.SINGLE_EPOCHS):
                t.w = log["gyro"][e][i]
                t.predict(log["dt"])
                t.update("acceleration", log["acc"][e][i], log["acc_cov"])
            t.update("velocity", log["dvl"][-1][i], log["dvl_cov"])
            t.w = log["gyro"][CS.SINGLE_EPOCHS][i]
        assert max(err(o, ts, dof)) < TOL
        acc = o.update(kind, mu, cov, extra=extra, only_vel=vo)
        assert acc.all(), (name, acc)
        for i, t in enumerate(ts):
            t.update(kind, mu[i], cov if shared else cov[i], extra=None if extra is None else GS.extra_of(
                kind, extra, i), only_vel=bool(vo))
        worst[name] = err(o, ts, dof)
        assert max(worst[name]) < TOL, (name, worst[name])
    print("single calls dof %d %s %s oracle against twin: %s" % (
        dof, side, "shared" if shared else "per instance",
        ", ".join("%s %.2g/%.2g" % ((k,) + v) for k, v in worst.items())))


def scenes(dof, right):
    """{name: (log, config or None)} of every log scene, B = 2"""
    base = CS.full_log(B, dof=dof, right=right)
    out = dict(full=(base, None), cells1=(CS.full_log(B, dof=dof, cells=1, right=right), None),
               cells8=(CS.full_log(B, dof=dof, cells=8, right=right), None),
               dive=(CS.dive_log(B, dof=dof, right=right), None), coarse=(CS.coarse(base), None),
               velocity_only=(CS.full_log(B, dof=dof, right=right, velocity_only=True), None),
               far_a=(CS.far(CS.tight(CS.coarse(CS.full_log(B, dof=dof, first=1)))), None),
               far_b=(CS.far(CS.tight(CS.coarse(CS.full_log(B, dof=dof, first=3)))), None))
    for lat, cfg in CS.lat_variants():
        out["lat%g" % lat] = (CS.cut(base, 40), cfg)
    return out


SCENES = ("full", "cells1", "cells8", "dive", "velocity_only", "coarse", "far_a", "far_b", "lat0", "lat-0.6", "lat1.4")


@pytest.mark.parametrize("dof", DOFS)
@pytest.mark.parametrize("scene", SCENES)
def test_logs(scene, dof, side):
    log, cfg = scenes(dof, side == "right")[scene]
    o = CS.start_scene(O.OraclePoseBatch(B, dof), log, cfg)
    ts = CS.twins_of(log, dof, cfg)
    counts = o.run_log(log)
    for i, t in enumerate(ts):
        twin_run_log(t, log, i)
    e = err(o, ts, dof)
    print("%s dof %d %s oracle against twin: mean %.3g cov %.3g, accepts %s" % (scene, dof, side, e[0], e[1],
                                                                                counts.tolist()))
    assert max(e) < TOL_LOG, e
    want = CS.expected_counts(log)
    np.testing.assert_array_equal(counts[:, [0, 1, 3]], [[want[0], want[1], want[3]]] * B)
    if scene in ("full", "cells1", "cells8", "dive", "velocity_only"):
        cells = log["adcp_cells"]
        assert want == ([1, 1, cells, 4] if scene == "dive" else [2, 2, cells, 5])
        assert (counts[:, 2] == cells).all(), counts  # every cell at ADCP_D2
    if scene == "dive":
        assert (np.abs(log["x0"][:, 9]) >= CS.DIVE_VZ).all() and log["x0"][0, 9] * log["x0"][1, 9] < 0
        vz = o.get_state()[0][:, 9]
        print("dive: v_z at the end %s" % vz)
        assert (vz * log["x0"][:, 9] > 0).all()  # every instance still moves the way it started
    if scene.startswith("far"):
        assert CS.library_branch(log["pos0"][:, 0]).tolist() == dict(far_a=[True, False], far_b=[True, True])[scene]


@pytest.mark.parametrize("dof", DOFS)
def test_fixes_piecewise(dof, side):
    log = CS.full_log(B, dof=dof, right=side == "right")
    fx = CS.fixes_for(log, dof)
    f = fx["flags"]
    assert [int(((f & b) != 0).sum()) for b in (CS.XY, CS.Z, CS.GEO)] == [2, 1, 2]
    xo, Po, acc, facc = CS.oracle_run_fixes(log, fx, dof)
    ts = CS.twins_of(log, dof)
    cuts = CS.fix_cuts(log, fx)
    for i, t in enumerate(ts):
        for a, b in zip(cuts[:-1], cuts[1:]):
            seg = dict(log)
            for k in ("flags", "gyro", "acc", "dvl_index", "pressure_index", "adcp_index", "efforts_index"):
                seg[k] = log[k][a:b]
            seg["epochs"] = b - a
            twin_run_log(t, seg, i)
            e = b - 1
            if f[e] & CS.XY:
                t.update("xy", fx["xy"][fx["xy_index"][e]][i], fx["xy_cov"])
            if f[e] & CS.Z:
                t.update("z", fx["z"][fx["z_index"][e]][i:i + 1], fx["z_cov"].reshape(1, 1))
            if f[e] & CS.GEO:
                t.update("geographic", fx["geo"][fx["geo_index"][e]][i], fx["geo_cov"], extra=fx["gps_in_body"])
    es = max(state_err(t.mu[None], xo[i:i + 1], Po[i:i + 1], dof).max() for i, t in enumerate(ts))
    ec = max(cov_err(t.P[None], Po[i:i + 1]).max() for i, t in enumerate(ts))
    print("fixes dof %d %s oracle against twin: mean %.3g cov %.3g, fix accepts %s" % (dof, side, es, ec,
                                                                                      facc.tolist()))
    assert max(es, ec) < TOL_LOG
    np.testing.assert_array_equal(facc, [[2, 1, 2]] * B)
    # the fixes are in the result
    o = CS.start(O.OraclePoseBatch(B, dof), log)
    o.run_log(log)
    assert state_err(o.get_state()[0], xo, Po, dof).min() > MATTERS


# ---- each feature matters ------------------------------------------------------------------
def end_state(log, dof, cfg=None, start=None):
    o = O.OraclePoseBatch(log["batch"], dof)
    if start is None:
        CS.start_scene(o, log, cfg)
    else:
        start(o)
    o.run_log(log)
    return o.get_state()


def moved(ref, alt, dof, rows=slice(None)):
    """per instance: (mean in sigma, covariance in sqrt(P_ii P_jj)) of alt against ref"""
    (xr, Pr), (xa, Pa) = ref, alt
    return state_err(xa, xr, Pr, dof)[rows], cov_err(Pa, Pr)[rows]


def check_teeth(name, results, unseen=()):
    """results: {dof: (ref, alt[, rows])}"""
    line = []
    for dof, r in results.items():
        if dof in unseen:
            for u, v in zip(r[0], r[1]):
                np.testing.assert_array_equal(u, v, err_msg="%s at %d DOF" % (name, dof))
            line.append("dof %d bitwise" % dof)
            continue
        es, ec = moved(r[0], r[1], dof, *r[2:])
        line.append("dof %d mean %.3g cov %.3g" % (dof, es.min(), ec.min()))
        assert (np.maximum(es, ec) >= MATTERS).all(), (name, dof, es, ec)
    print("%s (min over instances): %s" % (name, ", ".join(line)))


@pytest.mark.parametrize("name", [n for n, _, _ in CS.alterations()])
def test_each_config_feature_matters(name):
    _, cfg, seen26 = next(a for a in CS.alterations() if a[0] == name)
    res = {}
    for dof in DOFS:
        log = CS.full_log(B, dof=dof)
        res[dof] = (end_state(log, dof), end_state(log, dof, cfg))
    check_teeth(name, res, () if seen26 else (26,))


def test_mounting_rotation_in_q_matters():
    res = {}
    for dof in DOFS:
        log = CS.full_log(B, dof=dof)
        res[dof] = (end_state(log, dof), end_state(log, dof, start=lambda o, log=log: CS.start(o, log, mount_q=False)))
    check_teeth("mounting left out of Q", res)


@pytest.mark.parametrize("name", sorted(CS.FULL_COVS) + ["pressure_lever", "cell_weights"])
def test_each_sensor_feature_matters(name):
    res = {}
    for dof in DOFS:
        log = CS.full_log(B, dof=dof, cells=8 if name == "cell_weights" else 4)
        if name in CS.FULL_COVS:
            alt = CS.diagonal_of(log, name)
        elif name == "pressure_lever":
            alt = dict(log, pressure_sensor_in_imu=np.zeros(3))
        else:  # the 4-cell weights, twice
            alt = dict(log, adcp_cell_weighting=np.tile(CS.FOUR_CELL_WEIGHTS, 2))
        res[dof] = (end_state(log, dof), end_state(alt, dof))
    check_teeth(name, res)


def test_far_matters():
    """x subtracted again, every shifted instance: the latitude is in the result"""
    res = {}
    for dof in DOFS:
        base = CS.tight(CS.coarse(CS.full_log(5, dof=dof)))
        log = CS.far(base)
        x, P = end_state(log, dof)
        x[:, 0] -= log["shift"]
        res[dof] = (end_state(base, dof), (x, P), log["shift"] != 0)
    check_teeth("far", res)


def test_dive_matters():
    """The level start of the same log: the covariance alone counts (the mean
    differs by the dive itself), and the water velocity variances grow"""
    for dof in DOFS:
        log = CS.dive_log(B, dof=dof)
        x0, P0 = CS.level_start(log)
        ref = end_state(log, dof)
        alt = end_state(log, dof, start=lambda o: CS.start_from_state(o, x0, P0, log["dt"]))
        ec = cov_err(alt[1], ref[1])
        d = abi.layout(dof)["d_wv"]
        print("dive dof %d against the level start: cov %.3g (min over instances)" % (dof, ec.min()))
        assert (ec >= MATTERS).all(), (dof, ec)
        print("water velocity variance, dive / level: %s" % (ref[1][:, d, d] / alt[1][:, d, d]))
