"""The PoseUKF edge scenes of tests/pose_scenes.py are valid before anything
runs on a GPU.

Wide priors: on every scene, layout and SO3 side the C oracle and the numpy
twin agree to the twin tolerance after every step of the window and after each
single call of pose_scenes.single_calls; the orientation steps of the sigma
points fall on the sides of so3_exp_psp's and so3_log_psp's thresholds the
scene is built for (and do not with make_pose_log's own prior: the check
guards the GPU tests).

Indefinite Sigma: the first non-positive pivot of every scene sits at the
stated index with the stated sign, the parameter block stays decoupled, and
the oracle's predict refuses every negative-pivot scene with UWVK_ENOTPD.

Measured (oracle against twin, max over instances, steps, layouts and sides,
in the oracle's sigma): wide 5.3e-11, straddle 2.6e-11, narrow 5.7e-12,
big_step 5.2e-12, far_step 2.3e-12; the single calls 1.3e-11."""
import copy
import ctypes as C

import numpy as np
import pytest

import numpy_twin as T
import oracle_ctypes as O
import pose_scenes as PS
from helpers import cov_err, pivots, state_err
from uwvk import abi, synth

TOL = 1e-10  # oracle against twin, in the oracle's sigma (tests/test_oracle_twin.py)
B = 4
ENOTPD = 3
SCENES = sorted(PS.SCENE_SD)


@pytest.fixture(params=["right", "left"])
def side(request):
    right = request.param == "right"
    prev = T.SO3_RIGHT
    T.SO3_RIGHT = right
    with O.so3_side(right):
        yield request.param
    T.SO3_RIGHT = prev


twin = PS.twin


def err(o, ts, dof):
    xo, Po = o.get_state()
    es = max(state_err(t.mu[None], xo[i:i + 1], Po[i:i + 1], dof).max() for i, t in enumerate(ts))
    ec = max(cov_err(t.P[None], Po[i:i + 1]).max() for i, t in enumerate(ts))
    return max(es, ec)


@pytest.mark.parametrize("dof", [53, 26])
@pytest.mark.parametrize("scene", SCENES)
def test_oracle_matches_twin(scene, dof, side):
    log = PS.make(scene, B, dof)
    o = PS.start(O.OraclePoseBatch(B, dof), log)
    ts = [twin(log, i, dof) for i in range(B)]
    worst = err(o, ts, dof)
    assert worst < 1e-14
    after_predict = None
    for e in range(log["epochs"]):
        o.set_rotation_rate(log["gyro"][e])
        o.predict(log["dt"])
        for i, t in enumerate(ts):
            t.w = log["gyro"][e][i]
            t.predict(log["dt"])
        worst = max(worst, err(o, ts, dof))
        if e == 0:
            after_predict = copy.deepcopy(ts)
        o.update("acceleration", log["acc"][e], log["acc_cov"])
        for i, t in enumerate(ts):
            t.update("acceleration", log["acc"][e][i], log["acc_cov"])
        worst = max(worst, err(o, ts, dof))
        if log["flags"][e] & abi.EV_DVL:
            z = log["dvl"][log["dvl_index"][e]]
            o.update("velocity", z, log["dvl_cov"])
            for i, t in enumerate(ts):
                t.update("velocity", z[i], log["dvl_cov"])
            worst = max(worst, err(o, ts, dof))
    print("%s dof %d %s: window %.3g" % (scene, dof, side, worst))
    assert worst < TOL
    # the whole window in one native call: bitwise the per-call loop
    whole = PS.start(O.OraclePoseBatch(B, dof), log)
    whole.run_log(log)
    for a, b in zip(whole.get_state(), o.get_state()):
        np.testing.assert_array_equal(a, b)
    # each single call from the state after the first predict
    worst = 0.0
    for n, (name, kind, mu, cov, extra, vo) in enumerate(PS.single_calls(log, after_predict_mean(log, dof))):
        o = PS.start(O.OraclePoseBatch(B, dof), log)
        o.set_rotation_rate(log["gyro"][0])
        o.predict(log["dt"])
        ao = o.update(kind, mu, cov, extra=extra, only_vel=vo)
        ts = copy.deepcopy(after_predict)
        for i, t in enumerate(ts):
            ex = extra[i] if kind in ("water_velocity", "delayed_xy") else extra
            at = t.update(kind, mu[i], cov, extra=ex, only_vel=bool(vo))
            assert bool(at) == bool(ao[i]), (name, i)
        worst = max(worst, err(o, ts, dof))
        assert worst < TOL, (name, worst)
    print("%s dof %d %s: single calls %.3g" % (scene, dof, side, worst))


def after_predict_mean(log, dof):
    o = PS.start(O.OraclePoseBatch(log["batch"], dof), log)
    o.set_rotation_rate(log["gyro"][0])
    o.predict(log["dt"])
    return o.get_state()[0]


def branch_sides(scene, log, dof):
    """Asserts the condition `scene` is built for on the oracle's Sigma before
    the first predict, before epoch 0's acceleration update and before the DVL
    update of pose_scenes.dvl_epoch(scene); returns the norms it looked at."""
    o = PS.start(O.OraclePoseBatch(log["batch"], dof), log)
    seen = []

    def look(where):
        P = o.get_state()[1]
        c = np.array([PS.ori_column_norms(Pi) for Pi in P])
        seen.append((where, c.max(axis=1)))
        margin = 1.1
        if scene == "wide":
            assert (c.max(axis=1) > margin * PS.EXP_SERIES_BELOW).all(), (where, c.max(axis=1))
            if where != "dvl":  # every orientation column above both thresholds
                assert (np.sort(c, axis=1)[:, -3:] > margin * PS.EXP_SERIES_BELOW).all(), where
        elif scene == "straddle" and where != "dvl":
            top = np.sort(c, axis=1)[:, -3:]
            assert (top[:, 0] < PS.LOG_SERIES_BELOW / margin).all(), (where, top)  # the series for both maps
            assert ((top[:, 1] > margin * PS.LOG_SERIES_BELOW) & (top[:, 1] < PS.EXP_SERIES_BELOW / margin)).all(), \
                (where, top)  # the library for log only
            assert (top[:, 2] > margin * PS.EXP_SERIES_BELOW).all(), (where, top)  # the library for both
        elif scene in ("narrow", "big_step") or (scene == "far_step" and where == "predict"):
            # (far_step's rotation of 2.56 rad turns the gyro-bias prior into 0.12 rad of orientation)
            assert (c.max(axis=1) < 0.1 / margin).all(), (where, c.max(axis=1))

    look("predict")
    for e in range(PS.dvl_epoch(scene) + 1):
        o.set_rotation_rate(log["gyro"][e])
        o.predict(log["dt"])
        if e == 0:
            look("acceleration")
        o.update("acceleration", log["acc"][e], log["acc_cov"])
    look("dvl")
    return seen


@pytest.mark.parametrize("dof", [53, 26])
@pytest.mark.parametrize("scene", SCENES)
def test_orientation_steps_take_the_branches(scene, dof, side):
    for where, c in branch_sides(scene, PS.make(scene, 8, dof), dof):
        print(scene, dof, side, where, np.round(c, 3))


@pytest.mark.parametrize("scene", ["wide", "straddle"])
def test_branch_check_fails_on_the_default_prior(scene):
    """the guard is live: the scene with make_pose_log's own rot_cov does not pass it"""
    log = PS.make(scene, 8)
    log["rot_cov"] = PS.make("narrow", 8)["rot_cov"]
    with pytest.raises(AssertionError):
        branch_sides(scene, log, 53)


def test_big_step_rotation():
    log = PS.make("big_step", B)
    step = np.linalg.norm(log["gyro"], axis=2) * log["dt"]
    assert step.min() > 1.1 * PS.EXP_SERIES_BELOW and log["dt"] == 0.1
    np.testing.assert_allclose(log["gyro"].mean(axis=(0, 1)), PS.BIG_GYRO, atol=1e-3)
    far = PS.make("far_step", B)
    step = np.linalg.norm(far["gyro"], axis=2) * far["dt"]
    assert 2.5 < step.min() and step.max() < 3.0  # the series' first dropped term above 1e-9, below pi
    u = 0.25 * step.min() ** 2
    assert u ** 6 / 6227020800.0 > 1e-9
    assert (np.linalg.norm(PS.make("wide", B)["gyro"], axis=2) * 1e-3).max() < 0.01  # elsewhere: the series


def test_wide_double_cover_and_dvl_epoch():
    w, n = PS.make("wide", 6), PS.make("narrow", 6)
    np.testing.assert_array_equal(w["rot0"][1::2], -n["rot0"][1::2])
    np.testing.assert_array_equal(w["rot0"][0::2], n["rot0"][0::2])
    for k in ("gyro", "acc", "dvl", "pos0"):
        np.testing.assert_array_equal(w[k], n[k])
    assert np.flatnonzero(w["flags"] & abi.EV_DVL).tolist() == [PS.DVL_EPOCH] and w["epochs"] <= 6
    assert w["dvl"].shape == (1, 6, 3) and w["dvl_index"][PS.DVL_EPOCH] == 0
    assert len({tuple(np.diag(c)) for c in w["rot_cov"]}) == 3  # the prior differs per instance


def test_instances_do_not_depend_on_the_batch():
    for scene in SCENES:
        a, b = PS.make(scene, 7), PS.make(scene, 2, first=5)
        for k in PS.PER_INSTANCE_EPOCH_MAJOR:
            np.testing.assert_array_equal(a[k][:, 5:7], b[k])
        for k in PS.PER_INSTANCE:
            np.testing.assert_array_equal(a[k][5:7], b[k])
    w, n = PS.make("wide", 4), PS.make("narrow", 4)
    m = PS.mix([(n, 0), (w, 2), (w, 3), (n, 1)])
    assert m["batch"] == 4 and m["gyro"].shape == w["gyro"].shape
    np.testing.assert_array_equal(m["rot_cov"][1], w["rot_cov"][2])
    np.testing.assert_array_equal(m["rot_cov"][3], n["rot_cov"][1])
    np.testing.assert_array_equal(m["acc"][:, 2], w["acc"][:, 3])


# ---- indefinite Sigma -------------------------------------------------------
def predict_codes(dof, x, P, log):
    """or_pose_predict's return code per instance from (x, P)"""
    o = O.OraclePoseBatch(len(x), dof)
    o.init_from_state(x, P, *PS.state_handles(dof))
    o.set_process_noise_from_config(synth.default_pose_config(), log["dt"])
    o.set_rotation_rate(log["gyro"][PS.HEALTHY_EPOCHS])
    return [o.L.or_pose_predict(o.ptr(i), C.c_double(log["dt"])) for i in range(len(x))]


@pytest.mark.parametrize("dof", [53, 26])
def test_healthy_state(dof):
    log, x, P = PS.healthy_state(6, dof)
    for Pi in P:
        assert np.array_equal(Pi, Pi.T) and len(pivots(Pi)) == dof and (pivots(Pi) > 0).all()
        off = Pi[:19, :19] - np.diag(np.diag(Pi[:19, :19]))
        assert (np.abs(off) > 0).sum() > 100  # the updates coupled the kinematic block
        if dof == 53:
            assert PS.param_block_decoupled(Pi)
    assert predict_codes(dof, x, P, log) == [0] * 6


@pytest.mark.parametrize("dof", [53, 26])
def test_indefinite_scenes(dof):
    log, x, P = PS.healthy_state(2, dof)
    for name, (build, p, sign) in sorted(PS.indefinite_scenes(dof).items()):
        Pb = build(P[1])
        d = pivots(Pb)
        assert np.array_equal(Pb, Pb.T) and np.isfinite(Pb).all()
        assert len(d) == p + 1 and (d[:p] > 0).all(), (name, d)
        assert (d[p] < 0) if sign < 0 else (d[p] == 0.0), (name, d[p])
        if dof == 53:
            assert PS.param_block_decoupled(Pb), name  # still PD- and pair-eligible
        if sign < 0:
            codes = predict_codes(dof, x, np.stack([P[0], Pb]), log)
            assert codes == [0, ENOTPD], (name, codes)


def test_scaling_one_pivot_to_zero_is_not_an_exact_zero():
    """why the zero-pivot scenes zero a row and column instead: L diag(D) L^T
    with D[p] = 0 leaves a pivot of rounding size and either sign"""
    _, _, P = PS.healthy_state(1, 53)
    L = np.linalg.cholesky(P[0])
    D = np.ones(53)
    D[14] = 0.0
    d = pivots(0.5 * ((L * D) @ L.T + ((L * D) @ L.T).T))
    assert len(d) < 53 or (d > 0).all()
    assert not (len(d) == 15 and d[14] == 0.0)


@pytest.mark.parametrize("factor", PS.Z_VARIANCE_FACTORS)
@pytest.mark.parametrize("dof", [53, 26])
def test_negative_z_variance(dof, factor):
    """The run-time case of tests/test_gpu_pose_edges.py: a z update whose
    variance is factor * P[2, 2] < 0, then a predict.  The update's own
    factorisation sees the healthy Sigma.
    -0.5: S = P[2, 2] / 2, Sigma - C K^T has P[2, 2] - 2 P[2, 2] < 0 at pivot 2:
          the oracle returns UWVK_ENOTPD from the update (its re-spread factors
          the reduced Sigma, which it leaves in place) and again from the predict.
    -1.5: S = -P[2, 2] / 2 < 0, so Sigma - C K^T = Sigma + 2 c c^T / P[2, 2] (c:
          column 2) GROWS and stays positive definite: UWVK_OK from both calls."""
    log, x, P = PS.healthy_state(2, dof)
    o = O.OraclePoseBatch(2, dof)
    o.init_from_state(x, P, *PS.state_handles(dof))
    o.set_process_noise_from_config(synth.default_pose_config(), log["dt"])
    o.set_rotation_rate(log["gyro"][PS.HEALTHY_EPOCHS])
    acc = C.c_int(0)
    codes = [o.L.or_pose_update_z(o.ptr(i), O.dp(x[i, 2:3] + 0.01), O.dp(np.array([R])), C.byref(acc))
             for i, R in enumerate((0.01, factor * P[1, 2, 2]))]
    d = pivots(o.get_state()[1][1])
    assert (pivots(o.get_state()[1][0]) > 0).all()
    after = [o.L.or_pose_predict(o.ptr(i), C.c_double(log["dt"])) for i in range(2)]
    if PS.z_variance_breaks_sigma(factor):
        assert codes == [0, ENOTPD] and after == [0, ENOTPD]
        assert len(d) == 3 and d[2] < 0, d
    else:
        assert codes == [0, 0] and after == [0, 0]
        assert len(d) == dof and (d > 0).all() and abs(d[2] / P[1, 2, 2] - 3.0) < 1e-6


signed_window = PS.signed_window


@pytest.mark.parametrize("dof", [53, 26])
def test_signed_twin_is_the_twin_on_a_healthy_sigma(dof):
    log, x, P = PS.healthy_state(2, dof)
    o = O.OraclePoseBatch(2, dof)
    o.init_from_state(x, P, *PS.state_handles(dof))
    o.set_process_noise_from_config(synth.default_pose_config(), log["dt"])
    o.run_log(log, 0, PS.NOTPD_WINDOW)
    xo, Po = o.get_state()
    mu, Pt = signed_window(log, x[1], P[1], 1, dof)
    assert state_err(mu[None], xo[1:], Po[1:], dof).max() < TOL and cov_err(Pt[None], Po[1:]).max() < TOL


@pytest.mark.parametrize("dof", [53, 26])
def test_undetected_pivots_stay_beyond_k(dof):
    """EXPECT_FLAG of tests/test_gpu_pose_edges.py says run_log over the window
    raises UWVK_ST_NOTPD iff the first non-positive pivot p of the initial
    Sigma is below the predict's k = 15.  For p >= 15 that needs every later
    step of the window to meet its first non-positive pivot at or beyond its
    own k too: shown here on the signed-weight restatement of the PSP steps.
    (The last acceleration update heals the gravity pivot, p = 18; the decoupled
    zero variance turns positive with the first predict's Q.)"""
    log, x, P = PS.healthy_state(2, dof)
    for name, (build, p, sign) in sorted(PS.indefinite_scenes(dof).items()):
        if p < PS.PSP_K["predict"]:
            continue
        seen = []

        def look(step, Pt):
            seen.append(PS.first_bad_pivot(Pt))
            assert seen[-1] >= PS.PSP_K[step], (name, step, seen)
        mu, Pt = signed_window(log, x[1], build(P[1]), 1, dof, look)
        assert len(seen) == 2 * PS.NOTPD_WINDOW + 1 and seen[0] == p
        assert np.isfinite(mu).all() and np.isfinite(Pt).all()
        print(dof, name, seen)
