"""The scenes of tests/pose_model_scenes.py (general vehicle model, mounted IMU,
tilted attitude) are valid before anything runs on a GPU.

 * the model is what it claims: dense, non-symmetric in every off-diagonal
   pair, well conditioned, W != B, general centres;
 * the C oracle and the numpy twin agree on every scene, both layouts and
   both SO3 sides, to the tolerances of tests/test_oracle_twin.py: init with
   the mounting 1e-15 / 1e-18, single calls and the sequence full -> predict
   -> velocity-only 1e-10, model_log 1e-8;
 * calcEfforts restated a third time, in Fossen's matrix form, agrees with
   numpy_twin.UWV.efforts on the general model to 1e-12 relative: the row /
   column convention is pinned independently of both filters;
 * each feature matters: with one feature of the scene taken away the
   oracle's result moves by at least 1e-3 (sigma units, 1e6 times the GPU
   tests' single-step tolerance), so a kernel that ignores or mixes up that
   feature cannot pass tests/test_gpu_pose_model.py;
 * with synth.default_uwv() the three transpositions are bitwise invisible.

Measured (max over instances, layouts and sides, in the oracle's sigma):
oracle against twin: init with the mounting 6.9e-18 / 6.6e-24 absolute (mean /
covariance), single full 1.9e-13 / 1.8e-13, single velocity-only 1.8e-13 /
1.8e-13, the sequence 2.5e-13 / 1.8e-13, model_log 1.6e-9 / 1.4e-11;
Fossen form against the twin 5.0e-15 relative.
Sensitivity of the oracle to each alteration (what the call does to the
filter, see effect_difference; the larger of mean and covariance, minimum
over instances and layouts; full / velocity-only):
  M^T 1.8 / 6.7, Dl^T 0.12 / 0.11, Dq^T 0.68 / 1.1, diagonals only 1.3 / 1.7,
  cog = 0 6.9 / 18, cob = 0 9.5 / 23, W = B 13 / 15, imu = 0 2.8 / 14,
  level attitude 7.8 / 3.5, identity mounting rotation 0.10 / 0.089;
  the minimum over all of them: 0.089;
model_log's end state: diagonals only 60, imu = 0 18 (minimum over layouts).
The scene went through two changes to get there: with the constructor's
velocity prior of 1 m/s a velocity-only update cuts that variance 1e4-fold
and oracle and twin part by 8e-11 (single call) and 6.5e-7 (log); so
tilted_state narrows the prior with one DVL and one accelerometer sample, and
model_log has a DVL epoch before its first velocity-only efforts epoch."""
import numpy as np
import pytest

import numpy_twin as T
import oracle_ctypes as O
import pose_model_scenes as MS
from helpers import cov_err, state_err
from uwvk import abi, synth

TOL = 1e-10      # oracle against twin: init, single calls, the sequence (tests/test_oracle_twin.py)
TOL_LOG = 1e-8   # oracle against twin over a log (tests/test_oracle_twin.py::test_run_log_matches_twin)
MATTERS = 1e-3   # 1e6 x the single-step tolerance of the GPU tests
B = 2


@pytest.fixture(params=["right", "left"])
def side(request):
    right = request.param == "right"
    prev = T.SO3_RIGHT
    T.SO3_RIGHT = right
    with O.so3_side(right):
        yield request.param
    T.SO3_RIGHT = prev


def err(o, ts, dof):
    xo, Po = o.get_state()
    es = max(state_err(t.mu[None], xo[i:i + 1], Po[i:i + 1], dof).max() for i, t in enumerate(ts))
    ec = max(cov_err(t.P[None], Po[i:i + 1]).max() for i, t in enumerate(ts))
    return float(es), float(ec)


# ---- the scene is what it claims -------------------------------------------------
def test_model_is_general():
    base = (1.3, 0.7, 1.5)
    for A, A0, f in zip(MS.general_arrays(), synth.uwv_arrays(synth.default_uwv()), base):
        np.testing.assert_array_equal(np.diag(A), f * np.diag(A0))
        off = ~np.eye(6, dtype=bool)
        sc = np.sqrt(np.outer(np.diag(A), np.diag(A)))[off]
        assert (np.abs(A - A.T)[off] >= 0.06 * sc * (1 - 1e-12)).all()
        assert np.abs(A - A.T)[off].min() > 0.2  # against tolerances of 1e-9
        # dense: every entry inside rows / columns {0, 1, 5} and in {2, 3, 4}
        assert (np.abs(A)[off] >= 0.01 * sc * (1 - 1e-9)).all() and np.abs(A)[off].min() > 0.03
        assert np.linalg.eigvalsh(0.5 * (A + A.T)).min() > 0.5 * np.diag(A).min()
        assert np.linalg.cond(A) < 50
    u = MS.general_uwv()
    assert u.weight != u.buoyancy
    cog, cob = np.array(u.distance_body2centerofgravity[:]), np.array(u.distance_body2centerofbuoyancy[:])
    assert cog.all() and cob.all() and np.linalg.norm(np.cross(cog, cob)) > 1e-4
    ib, q = MS.mounting()
    assert abs(np.linalg.norm(q) - 1) < 1e-15 and 2 * np.arccos(q[0]) > 0.5 and ib[:3].all()
    np.testing.assert_array_equal(ib[3:], q)


@pytest.mark.parametrize("dof", [53, 26])
def test_tilted_state_contract(dof):
    x, P = MS.tilted_state(3, dof)
    L = abi.layout(dof)
    for i in range(3):
        R = T.qmat(x[i, 3:7])
        roll, pitch = np.arctan2(R[2, 1], R[2, 2]), -np.arcsin(R[2, 0])
        assert 0.09 < abs(roll) < 0.41 and 0.09 < abs(pitch) < 0.41, (roll, pitch)
        assert np.abs(x[i, 7:10]).min() > 0.02 and np.abs(x[i, 10:13]).min() > 1e-3
        assert np.abs(x[i, L["s_wv"]:L["s_wv"] + 2]).min() > 1e-3
        np.linalg.cholesky(P[i])
        np.testing.assert_array_equal(P[i], P[i].T)
        for blk in (slice(12, 15), slice(15, 18)):  # the rotated bias blocks are not diagonal
            c = P[i, blk, blk] / np.sqrt(np.outer(np.diag(P[i, blk, blk]), np.diag(P[i, blk, blk])))
            assert np.abs(c[~np.eye(3, dtype=bool)]).min() > 0.05
        if dof == 53:  # the overlaid blocks, column-major, are not symmetric
            for k, A in zip((L["s_inertia"], L["s_lin"], L["s_quad"]), MS.general_arrays()):
                blk = x[i, k:k + 9].reshape(3, 3, order="F")
                np.testing.assert_array_equal(blk, A[np.ix_(MS.IDX, MS.IDX)])
                assert np.abs(blk - blk.T)[~np.eye(3, dtype=bool)].min() > 0.3
    # instance i depends on (seed, i) alone
    x1, P1 = MS.tilted_state(1, dof, first=2)
    np.testing.assert_array_equal(x1[0], x[2])
    np.testing.assert_array_equal(P1[0], P[2])
    w = MS.rates(3)
    assert (np.abs(w) > 0.05).all() and (np.linalg.norm(w, axis=1) < 1.0).all()


def test_model_log_contract():
    log = MS.model_log(3)
    f = log["flags"]
    at = np.flatnonzero(f & abi.EV_EFFORTS)
    assert log["epochs"] == 200 and len(at) == 5 and at[0] <= 3 and (np.diff(at) >= 40).all()
    vo = (f[at] & abi.EV_EFFORTS_VELOCITY_ONLY) != 0
    assert vo.tolist() == [False, True, False, True, False]
    for bit in (abi.EV_DVL, abi.EV_PRESSURE, abi.EV_ADCP):
        assert (f & bit).any()
    assert sorted(log["efforts_index"][at]) == list(range(5)) and log["efforts"].shape == (5, 3, 6)
    assert (log["efforts_index"][f & abi.EV_EFFORTS == 0] == -1).all()
    assert log["dvl_index"].max() == len(log["dvl"]) - 1
    one = MS.model_log(1, first=2)
    for k in ("gyro", "acc", "dvl", "efforts"):
        np.testing.assert_array_equal(one[k][:, 0], log[k][:, 2])
    np.testing.assert_array_equal(one["rot0"][0], log["rot0"][2])
    assert np.abs(log["gyro"].mean(axis=(0, 1))).min() > 0.15  # a body rate of a few tenths of a rad/s


# ---- oracle against twin ---------------------------------------------------------
@pytest.mark.parametrize("dof", [53, 26])
def test_init_with_mounting_identical(dof):
    log = MS.model_log(B, 4, dof)
    o = MS.start_log(O.OraclePoseBatch(B, dof), log)
    xo, Po = o.get_state()
    worst = [0.0, 0.0]
    for i in range(B):
        t = MS.twin_from_log(log, i, dof)
        np.testing.assert_allclose(t.mu, xo[i], rtol=0, atol=1e-15)
        np.testing.assert_allclose(t.P, Po[i], rtol=0, atol=1e-18)
        worst = [max(worst[0], np.abs(t.mu - xo[i]).max()), max(worst[1], np.abs(t.P - Po[i]).max())]
    print("init with the mounting, dof %d: mean %.3g cov %.3g (absolute)" % (dof, worst[0], worst[1]))
    # the mounting is in the result: turned bias offsets, non-diagonal bias blocks
    R = T.qmat(MS.mounting()[1])
    L = abi.layout(dof)
    np.testing.assert_allclose(xo[0, L["s_bg"]:L["s_bg"] + 3], R @ np.array(MS.GYRO_BIAS_OFFSET), rtol=0, atol=1e-17)
    np.testing.assert_allclose(xo[0, L["s_ba"]:L["s_ba"] + 3], R @ np.array(MS.ACC_BIAS_OFFSET), rtol=0, atol=1e-16)
    assert np.abs(Po[0, 12:15, 12:15][~np.eye(3, dtype=bool)]).min() > 1e-11
    assert np.abs(Po[0, 15:18, 15:18][~np.eye(3, dtype=bool)]).min() > 1e-9


@pytest.mark.parametrize("dof", [53, 26])
def test_twin_defaults_are_the_identity_mounting(dof):
    """imu_in_body = None and the identity 7-vector give the same twin, bitwise
    (and so does q_imu_in_body = None against the identity quaternion up to the
    rounding of R D R^T with R = I, which is exact)."""
    log = synth.make_pose_log(1, 1, "C3", dof=dof)
    cfg, uwv = T.cfg_dict(MS.model_config()), T.UWV.from_abi(MS.general_uwv())
    ident = np.array([0.0, 0, 0, 1, 0, 0, 0])
    a = T.PoseTwin.from_config(dof, log["pos0"][0], log["pos_cov"][0], log["rot0"][0], log["rot_cov"][0], cfg, uwv)
    b = T.PoseTwin.from_config(dof, log["pos0"][0], log["pos_cov"][0], log["rot0"][0], log["rot_cov"][0], cfg, uwv,
                               imu_in_body=ident)
    a.set_noise_from_config(cfg, 1e-3)
    b.set_noise_from_config(cfg, 1e-3, q_imu_in_body=ident[3:])
    for u, v in ((a.mu, b.mu), (a.P, b.P), (a.Q, b.Q), (a.p["imu_in_body"], b.p["imu_in_body"]),
                 (a.p["gyro_bias_offset"], b.p["gyro_bias_offset"]), (a.p["acc_bias_offset"], b.p["acc_bias_offset"])):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("dof", [53, 26])
@pytest.mark.parametrize("name", ["full", "vel", "sequence"])
def test_oracle_matches_twin_efforts_calls(name, dof, side):
    calls = MS.efforts_calls(B)
    x, P = MS.tilted_state(B, dof)
    o = MS.start_state(O.OraclePoseBatch(B, dof), B, dof)
    ts = [MS.twin_from_state(x, P, i, dof) for i in range(B)]
    np.testing.assert_array_equal(o.get_state()[0], x)
    w = MS.rates(B)
    worst = (0.0, 0.0)
    for z, R, vo in (calls[name] if name == "sequence" else [calls[name]]):
        o.predict(MS.DT)
        for i, t in enumerate(ts):
            t.w = w[i]
            t.predict(MS.DT)
        worst = tuple(map(max, worst, err(o, ts, dof)))
        o.update("efforts", z, R, only_vel=vo)
        for i, t in enumerate(ts):
            t.update("efforts", z[i], R, only_vel=bool(vo))
        worst = tuple(map(max, worst, err(o, ts, dof)))
    print("%s dof %d %s oracle against twin: mean %.3g cov %.3g" % ((name, dof, side) + worst))
    assert max(worst) < TOL, worst


def twin_run_log(t, log, i):
    for e in range(log["epochs"]):
        f = log["flags"][e]
        t.w = log["gyro"][e][i]
        t.predict(log["dt"])
        t.update("acceleration", log["acc"][e][i], log["acc_cov"])
        if f & abi.EV_DVL:
            t.update("velocity", log["dvl"][log["dvl_index"][e]][i], log["dvl_cov"])
        if f & abi.EV_PRESSURE:
            t.update("pressure", log["pressure"][log["pressure_index"][e]][i:i + 1],
                     np.array([[log["pressure_cov"]]]), extra=log["pressure_sensor_in_imu"])
        if f & abi.EV_ADCP:
            for c in range(log["adcp_cells"]):
                t.update("water_velocity", log["adcp"][log["adcp_index"][e]][c][i], log["adcp_cov"],
                         extra=log["adcp_cell_weighting"][c])
        if f & abi.EV_EFFORTS:
            t.update("efforts", log["efforts"][log["efforts_index"][e]][i], log["efforts_cov"],
                     only_vel=bool(f & abi.EV_EFFORTS_VELOCITY_ONLY))


@pytest.mark.parametrize("dof", [53, 26])
def test_oracle_matches_twin_model_log(dof, side):
    log = MS.model_log(B, dof=dof)
    o = MS.start_log(O.OraclePoseBatch(B, dof), log)
    ts = [MS.twin_from_log(log, i, dof) for i in range(B)]
    counts = o.run_log(log)
    for i, t in enumerate(ts):
        twin_run_log(t, log, i)
    e = err(o, ts, dof)
    print("model_log dof %d %s oracle against twin: mean %.3g cov %.3g, accepts %s" % (dof, side, e[0], e[1],
                                                                                      counts.tolist()))
    assert max(e) < TOL_LOG, e
    assert (counts[:, 0] == 2).all() and (counts[:, 1] == 2).all() and (counts[:, 3] == 5).all()


# ---- calcEfforts a third time: Fossen's matrix form ------------------------------
def fossen_efforts(M, Dl, Dq, W, Bu, cog, cob, acc6, nu, q):
    """tau = M a + C(nu) nu + Dl nu + Dq |nu| nu + g(q), C(nu) = [[0, -S(a)], [-S(a), -S(b)]],
    a = M11 v + M12 w, b = M21 v + M22 w; g through the rotation matrix."""
    def S(u):
        return np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    v, w = nu[:3], nu[3:]
    a = M[:3, :3] @ v + M[:3, 3:] @ w
    b = M[3:, :3] @ v + M[3:, 3:] @ w
    Cm = np.block([[np.zeros((3, 3)), -S(a)], [-S(a), -S(b)]])
    Rnb = T.qmat(q).T  # nav -> body
    fg, fb = Rnb @ np.array([0.0, 0.0, -W]), Rnb @ np.array([0.0, 0.0, Bu])
    g = -np.concatenate([fg + fb, S(cog) @ fg + S(cob) @ fb])
    return M @ acc6 + Cm @ nu + Dl @ nu + Dq @ (np.abs(nu) * nu) + g


def test_efforts_against_fossen_form():
    u = T.UWV.from_abi(MS.general_uwv())
    rng = np.random.default_rng(MS.SEED)
    worst = 0.0
    for _ in range(100):
        acc6, nu = rng.standard_normal(6), rng.standard_normal(6) * np.array([1, 1, 1, 0.5, 0.5, 0.5])
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        got = u.efforts(acc6, nu, q)
        ref = fossen_efforts(u.M, u.Dl, u.Dq, u.W, u.B, u.cog, u.cob, acc6, nu, q)
        worst = max(worst, np.abs(got - ref).max() / np.abs(ref).max())
        # and the transposed model is another model: the form tells them apart
        alt = fossen_efforts(u.M.T, u.Dl, u.Dq, u.W, u.B, u.cog, u.cob, acc6, nu, q)
        assert np.abs(alt - ref).max() > 1e-3 * np.abs(ref).max()
    print("UWV.efforts against the Fossen form: %.3g relative" % worst)
    assert worst < 1e-12


# ---- each feature matters --------------------------------------------------------
KIN_T = list(range(19)) + list(range(46, 53))   # the 26 kinematic tangent DOFs of the 53
KIN_S = list(range(20)) + list(range(47, 54))


def kin(x, P, dof):
    """the kinematic part of (x, P) in the 26-DOF layout"""
    if dof == 26:
        return x, P
    return x[:, KIN_S], P[:, KIN_T][:, :, KIN_T]


def call_effect(dof, form, **alter):
    """the oracle from start_state(**alter): (x, P) after the predict and after
    the scene's single call `form`, kinematic part"""
    z, R, vo = MS.efforts_calls(B)[form]
    o = MS.start_state(O.OraclePoseBatch(B, dof), B, dof, **alter)
    o.predict(MS.DT)
    pre = kin(*o.get_state(), dof)
    o.update("efforts", z, R, only_vel=vo)
    return pre + kin(*o.get_state(), dof)


def effect_difference(ref, alt, skip=()):
    """What the call did to the altered filter against what it did to the
    unaltered one, per instance: (mean, covariance) in the units of state_err /
    cov_err of the unaltered result.  Where the alteration leaves the prior
    alone this is state_err / cov_err of the two results; where it changes the
    prior too (the overlaid blocks, the attitude, the turned bias offsets) the
    prior's own difference does not count.  skip: tangent DOFs left out."""
    keep = np.array([d for d in range(26) if d not in skip])

    def moved(x0, P0, x1, P1):
        d = np.zeros((len(x0), 26))
        vec = np.array([k for k in range(26) if not 3 <= k < 6])
        sto = np.where(vec < 3, vec, vec + 1)
        d[:, vec] = x1[:, sto] - x0[:, sto]
        d[:, 3:6] = T.so3_log(T.qmul(T.qconj(x0[:, 3:7]), x1[:, 3:7]))
        return d, P1 - P0
    (dr, Dr), (da, Da) = moved(*ref), moved(*alt)
    sd = np.sqrt(np.diagonal(ref[3], axis1=1, axis2=2))
    sd[:, 3:6] = sd[:, 3:6].min(axis=1, keepdims=True)  # as state_err: the smallest orientation sigma
    em = (np.abs(da - dr) / sd)[:, keep].max(axis=1)
    ec = (np.abs(Da - Dr) / (sd[:, :, None] * sd[:, None, :]))[:, keep][:, :, keep].max(axis=(1, 2))
    return em, ec


ALTERATIONS = {
    "Mt": dict(uwv="Mt"), "Dlt": dict(uwv="Dlt"), "Dqt": dict(uwv="Dqt"), "diagonal": dict(uwv="diagonal"),
    "cog0": dict(uwv="cog0"), "cob0": dict(uwv="cob0"), "W=B": dict(uwv="W=B"),
    "imu0": dict(lever=(0.0, 0.0, 0.0)), "level": dict(level=True), "mount_identity": dict(rotvec=(0.0, 0.0, 0.0)),
}
# tangent DOFs whose prior the alteration itself sets: not counted
SKIP = {"level": (3, 4, 5), "mount_identity": tuple(range(12, 18))}


def _alter(name):
    kw = dict(ALTERATIONS[name])
    if "uwv" in kw:
        kw["uwv"] = MS.altered_uwv(kw["uwv"])
    return kw


@pytest.mark.parametrize("name", sorted(ALTERATIONS))
def test_each_feature_matters(name):
    """One feature of the scene taken away: what the single call does to the
    filter moves by at least 1e-3 sigma, in its mean or its covariance, in the
    full or the velocity-only form, for every instance and both layouts."""
    for dof in (53, 26):
        best = np.zeros(B)
        line = []
        for form in ("full", "vel"):
            em, ec = effect_difference(call_effect(dof, form), call_effect(dof, form, **_alter(name)),
                                       SKIP.get(name, ()))
            best = np.maximum(best, np.maximum(em, ec))
            line.append("%s mean %.3g cov %.3g" % (form, em.min(), ec.min()))
        print("%s dof %d (min over instances): %s" % (name, dof, ", ".join(line)))
        assert (best >= MATTERS).all(), (name, dof, best)


@pytest.mark.parametrize("name", ["diagonal", "imu0"])
def test_each_feature_matters_in_model_log(name):
    for dof in (53, 26):
        log = MS.model_log(B, dof=dof)
        ends = []
        for kw in ({}, _alter(name)):
            o = MS.start_log(O.OraclePoseBatch(B, dof), log, **kw)
            o.run_log(log)
            ends.append(kin(*o.get_state(), dof))
        (xr, Pr), (xa, Pa) = ends
        es, ec = state_err(xa, xr, Pr, 26), cov_err(Pa, Pr)
        print("%s dof %d model_log end state (min over instances): mean %.3g cov %.3g" % (name, dof, es.min(),
                                                                                          ec.min()))
        assert (np.maximum(es, ec) >= MATTERS).all(), (name, dof, es, ec)


# ---- the degenerate case is really degenerate ------------------------------------
@pytest.mark.parametrize("form", ["full", "vel"])
def test_default_model_hides_transposes(form):
    """With synth.default_uwv() (diagonal matrices) the three transpositions
    give bitwise the same oracle result: why no earlier test could see them."""
    M, Dl, Dq = synth.uwv_arrays(synth.default_uwv())
    u0 = synth.default_uwv()
    kw = dict(weight=u0.weight, buoyancy=u0.buoyancy, cog=u0.distance_body2centerofgravity[:],
              cob=u0.distance_body2centerofbuoyancy[:])
    ref = call_effect(53, form, uwv=MS.make_uwv(M, Dl, Dq, **kw))
    for Ma, Dla, Dqa in ((M.T, Dl, Dq), (M, Dl.T, Dq), (M, Dl, Dq.T)):
        for u, v in zip(ref, call_effect(53, form, uwv=MS.make_uwv(Ma, Dla, Dqa, **kw))):
            np.testing.assert_array_equal(u, v)
    # while on the general model each of them is seen (test_each_feature_matters)
    gen = call_effect(53, form)
    assert not np.array_equal(gen[2], ref[2])
