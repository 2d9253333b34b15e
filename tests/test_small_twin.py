"""Two independent CPU restatements of the small filters agree: the C oracle
(oracle/uwvk_small_oracle.c) and the numpy twin (oracle/numpy_twin.py) for the
S2 manifold, BottomUKF, IndirectPoseUKF and the marker-augmented visual update
of PoseUKF and IndirectPoseUKF.

The twin takes S2 through the rotation matrix R_x and the visual model through
composed rotation matrices; the oracle (and the HIP code written beside it)
use two basis vectors and step-wise quaternion sandwiches.  Agreement to TOL,
in units of the oracle's standard deviations, guards the formulas both share
with the kernels.  The scenes of tests/test_gpu_small_edges.py are the scenes
checked here (each must agree to SCENE_TOL before a GPU test may rely on it)."""
import numpy as np
import pytest

import numpy_twin as T
import oracle_ctypes as O
import visual_scene as V
from helpers import cov_err, pose_setup, state_err
from small_scenes import (BOTTOM_Q, bottom_err, bottom_sequence, ipose_err, ipose_large_error_run, ipose_small_run,
                          limit_tilt, per_instance_fcov)

L = O.lib()
DP = O.DP
TOL = 1e-10        # as tests/test_oracle_twin.py
SCENE_TOL = 1e-11  # a scene the GPU edge tests use must agree to this


@pytest.fixture(params=["right", "left"])
def side(request):
    right = request.param == "right"
    prev = T.SO3_RIGHT
    T.SO3_RIGHT = right
    with O.so3_side(right):
        yield right
    T.SO3_RIGHT = prev


# ---------------------------------------------------------------------------
# S2 operators
# ---------------------------------------------------------------------------
def _cap(rng, n, zmin):
    out = np.empty((0, 3))
    while len(out) < n:
        v = V.unit(rng.standard_normal((2 * n, 3)))
        out = np.concatenate([out, v[v[:, 2] > zmin]])
    return out[:n]


def test_s2_operators_over_the_sphere():
    """[+], [-] and the normalising constructor over the cap x_z > -0.9,
    |d| <= 1.5: absolute 1e-13."""
    rng = np.random.default_rng(7)
    n = 2000
    x, y = _cap(rng, n, -0.9), _cap(rng, n, -0.9)
    d = rng.uniform(-1.0, 1.0, (n, 2))
    d *= (rng.uniform(0, 1.5, n) / np.linalg.norm(d, axis=1))[:, None]
    v = rng.standard_normal((n, 3)) * rng.uniform(0.1, 10.0, (n, 1))
    po, mo, fo = np.zeros((n, 3)), np.zeros((n, 2)), np.zeros((n, 3))
    for i in range(n):
        L.or_s2_boxplus(O.dp(x[i]), O.dp(d[i]), O.C.c_double(1.0), po[i].ctypes.data_as(DP))
        L.or_s2_boxminus(O.dp(y[i]), O.dp(x[i]), mo[i].ctypes.data_as(DP))
        L.or_s2_from_vector(O.dp(v[i]), fo[i].ctypes.data_as(DP))
    ep = np.abs(T.s2_plus(x, d) - po).max()
    em = np.abs(T.s2_minus(y, x) - mo).max()
    ef = np.abs(T.s2_from(v) - fo).max()
    print("s2 oracle-twin: plus %.2e minus %.2e from %.2e" % (ep, em, ef))
    assert max(ep, em, ef) < 1e-13
    # the twin's own consistency: R_x is a rotation taking e3 to x
    R = T.s2_rot(x)
    assert np.abs(R @ np.array([0, 0, 1.0]) - x).max() < 1e-14
    assert np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max() < 1e-13


# ---------------------------------------------------------------------------
# BottomUKF
# ---------------------------------------------------------------------------
class BottomTwinBatch:
    """The twin behind the oracle wrapper's batch interface."""

    def __init__(self, B):
        self.batch = B

    def init(self, x, P):
        self.f = [T.BottomTwin(x[i], P[i]) for i in range(self.batch)]

    def set_process_noise(self, Q):
        for f in self.f:
            f.Q = np.array(Q, float)

    def set_velocity(self, v):
        for f, vi in zip(self.f, np.broadcast_to(v, (self.batch, 3))):
            f.velocity = np.array(vi, float)

    def predict(self, dt):
        for f in self.f:
            f.predict(dt)

    def update_range(self, z, cov, d, o):
        for f, zi, ci in zip(self.f, z, np.broadcast_to(cov, (self.batch,))):
            f.update_range(zi, ci, d, o)

    def update_normal(self, z, cov):
        for f, zi, ci in zip(self.f, z, np.broadcast_to(cov, (self.batch, 2, 2))):
            f.update_normal(zi, ci)

    def get_state(self):
        return np.stack([f.mu for f in self.f]), np.stack([f.P for f in self.f])


def _bottom_pair(B, x, P):
    o, t = O.OracleBottomBatch(B), BottomTwinBatch(B)
    for f in (o, t):
        f.init(x, P)
        f.set_process_noise(BOTTOM_Q)
    return o, t


@pytest.mark.parametrize("per_instance_cov,tilt,state_tilt",
                         [(False, 0.03, 0.1), (True, 0.03, 0.1), (True, 0.5, 0.5)],
                         ids=["shared_cov", "per_instance_cov", "tilted_60deg"])
def test_bottom_sequence(per_instance_cov, tilt, state_tilt):
    """30 steps at B = 5.  tilted_60deg: state and measured normals up to 60
    degrees from +e3 (the scene of the GPU large-error test)."""
    B = 5
    x, P = V.bottom_state(B, tilt=state_tilt)
    x[:, 1:] = limit_tilt(x[:, 1:])
    o, t = _bottom_pair(B, x, P)
    bottom_sequence((o, t), B, per_instance_cov=per_instance_cov, tilt=tilt)
    es, ec = bottom_err(*t.get_state(), *o.get_state())
    print("bottom sequence oracle-twin: state %.2e cov %.2e" % (es, ec))
    assert es < SCENE_TOL and ec < SCENE_TOL


def test_bottom_single_steps_steep_normals():
    """One predict, one range and one normal update from normals down to 38
    degrees below the equator (steep normals only in single steps: under the
    downward beams h_range is ill-conditioned there)."""
    rng = np.random.default_rng(9)
    B = 12
    x, P = V.bottom_state(B, seed=6)
    x[:, 1:] = _cap(rng, B, -0.6)
    zn = V.unit(x[:, 1:] + rng.normal(0, 0.05, (B, 3)))
    worst = 0.0
    for step in ("predict", "range", "normal"):
        o, t = _bottom_pair(B, x, P)
        if step == "predict":
            for f in (o, t):
                f.set_velocity(np.array([0.5, -0.2, 0.1]))
                f.predict(0.2)
        elif step == "range":
            for f in (o, t):
                f.update_range(np.full(B, 11.0), 0.02, [0.0, 0.0, -1.0], [0.1, 0.0, 0.0])
        else:
            for f in (o, t):
                f.update_normal(zn, np.array([[4e-4, 1e-4], [1e-4, 6e-4]]))
        es, ec = bottom_err(*t.get_state(), *o.get_state())
        worst = max(worst, es, ec)
    print("bottom single steps (steep) oracle-twin: %.2e" % worst)
    assert worst < TOL


# ---------------------------------------------------------------------------
# IndirectPoseUKF
# ---------------------------------------------------------------------------
class IPoseTwinBatch:
    def __init__(self, B):
        self.batch = B

    def init(self, pos_std, ori_std, tau, ipe=None, ips=None):
        self.f = [T.IndirectPoseTwin(pos_std, ori_std, tau, None if ipe is None else ipe[i], ips)
                  for i in range(self.batch)]

    def set_pose_reference(self, ref):
        for f, r in zip(self.f, ref):
            f.ref = np.array(r, float)

    def set_process_noise(self, Q):
        for f in self.f:
            f.Q = np.array(Q, float)

    def predict(self, dt):
        for f in self.f:
            f.predict(dt)

    def update_visual(self, px, fcov, fpos, marker, cm, cam, cib):
        nf = px.shape[1]
        fc = np.broadcast_to(fcov, (self.batch, nf, 2, 2))
        mk = np.broadcast_to(marker, (self.batch, 7))
        for i, f in enumerate(self.f):
            f.update_visual(px[i], fc[i], fpos, mk[i], cm, cam, cib)

    def get_corrected_pose(self):
        return np.stack([f.corrected_pose() for f in self.f])

    def get_state(self):
        return np.stack([f.mu for f in self.f]), np.stack([f.P for f in self.f])


def test_ipose_small_scene_per_instance_feature_cov(side):
    """the 0.02 rad scene with differing per-instance pixel covariances (the
    scene of the GPU shared-versus-per-instance test)"""
    B = 5
    o, t = O.OracleIndirectPoseBatch(B), IPoseTwinBatch(B)
    ipose_small_run((o, t), B, per_instance_fcov(B, 4))
    es, ec = ipose_err(*t.get_state(), *o.get_state())
    print("ipose small scene, per-instance cov, side=%s oracle-twin: state %.2e cov %.2e" % (side, es, ec))
    assert es < SCENE_TOL and ec < SCENE_TOL


@pytest.mark.parametrize("steps", [2, 4])
@pytest.mark.parametrize("nf", [1, 4, 7])
def test_ipose_predict_and_visual_large_errors(nf, steps, side):
    """Orientation errors of about 0.5 rad, the dense Q (whose orientation block
    predict rotates by the mean's rotation), 4 (or 2) predicts alternating with
    as many visual updates, then 5 predicts; also the scene of the GPU large-error and feature-count tests."""
    B = 5
    corners = {1: V.CORNERS[:1], 4: V.CORNERS, 7: V.CORNERS7}[nf]
    o, t = O.OracleIndirectPoseBatch(B), IPoseTwinBatch(B)
    q_err = ipose_large_error_run((o, t), B, corners, steps)
    assert np.median(2 * np.arccos(np.abs(q_err[:, 0]))) > 0.3
    (xo, Po), (xt, Pt) = o.get_state(), t.get_state()
    if nf >= 4:  # the estimate is far from identity (one bearing alone does not fix the orientation)
        assert (2 * np.arccos(np.abs(xo[:, 3])) > 0.1).all()
    es, ec = ipose_err(xt, Pt, xo, Po)
    ep = np.abs(t.get_corrected_pose() - o.get_corrected_pose()).max()
    print("ipose nf=%d side=%s oracle-twin: state %.2e cov %.2e corrected pose %.2e" % (nf, side, es, ec, ep))
    assert es < SCENE_TOL and ec < SCENE_TOL and ep < 1e-12
    # then 5 more predicts from the far-from-identity estimate (the rotated Q block alone)
    for k in range(5):
        o.predict(0.1)
        t.predict(0.1)
    es, ec = ipose_err(*t.get_state(), *o.get_state())
    print("  + 5 predicts: state %.2e cov %.2e" % (es, ec))
    assert es < SCENE_TOL and ec < SCENE_TOL


# ---------------------------------------------------------------------------
# PoseUKF visual-landmark update (n = 59 and n = 32)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dof,nf", [(53, 4), (26, 4), (53, 7), (53, 1)])
def test_pose_visual_update(dof, nf, side):
    """After a 60-epoch run_log (as test_gpu_pose_visual_landmark), two calls."""
    B = 2
    corners = {1: V.CORNERS[:1], 4: V.CORNERS, 7: V.CORNERS7}[nf]
    cfg, uwv, log = pose_setup(B, dof=dof, epochs=60)
    o = O.OraclePoseBatch(B, dof)
    o.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    o.set_process_noise_from_config(cfg, log["dt"])
    o.run_log(log)
    x0, P0 = o.get_state()
    true_t, true_q, marker, px = V.pose_scene(x0, corners=corners)
    fcov, fpos, cm, cam, cib = V.visual_common(B, corners, V.SEVEN_PIXEL_VAR if nf == 7 else 0.09)
    tw = []
    for i in range(B):
        t = T.PoseTwin.from_config(dof, log["pos0"][i], log["pos_cov"][i], log["rot0"][i], log["rot_cov"][i],
                                   T.cfg_dict(cfg), T.UWV.from_abi(uwv))
        t.mu, t.P = x0[i].copy(), P0[i].copy()  # the oracle's state after the log: the visual update alone
        tw.append(t)
    for rep in range(2):
        o.update_visual(px, fcov, fpos, marker, cm, cam, cib)
        for i, t in enumerate(tw):
            t.update_visual(px[i], fcov, fpos, marker[i], cm, cam, cib)
    xo, Po = o.get_state()
    xt, Pt = np.stack([t.mu for t in tw]), np.stack([t.P for t in tw])
    assert np.abs(xo - x0).max() > 1e-3  # the update did something
    es, ec = float(state_err(xt, xo, Po, dof).max()), float(cov_err(Pt, Po).max())
    print("pose visual dof=%d nf=%d side=%s oracle-twin: state %.2e cov %.2e" % (dof, nf, side, es, ec))
    assert es < SCENE_TOL and ec < SCENE_TOL
