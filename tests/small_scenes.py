"""Seeded scenes and sequences shared by the small-filter tests: the CPU
oracle-twin comparison (tests/test_small_twin.py) checks every scene that the
GPU edge tests (tests/test_gpu_small_edges.py) then run against the oracle.
A filter here is any batch object with the oracle wrapper's methods."""
import numpy as np

import visual_scene as V
from helpers import cov_err, qlog_err

BEAMS = [(V.unit([0.5, 0.0, -0.866]), [0.1, 0.0, 0.0]), (V.unit([-0.5, 0.0, -0.866]), [-0.1, 0.0, 0.0]),
         (V.unit([0.0, 0.5, -0.866]), [0.0, 0.1, 0.0]), (V.unit([0.0, -0.5, -0.866]), [0.0, -0.1, 0.0])]
BOTTOM_Q = np.diag([0.02, 0.001, 0.001])


def bottom_err(xa, Pa, xo, Po):
    """(state, covariance) error in the oracle's standard deviations."""
    e = np.abs(xa[:, 0] - xo[:, 0]) / np.sqrt(Po[:, 0, 0])
    ang = np.linalg.norm(np.cross(xa[:, 1:], xo[:, 1:]), axis=1)  # sin of the angle
    e = np.maximum(e, ang / np.sqrt(np.minimum(Po[:, 1, 1], Po[:, 2, 2])))
    return float(e.max()), float(cov_err(Pa, Po).max())


def bottom_sequence(filters, B, steps=30, seed=3, per_instance_cov=False, tilt=0.03):
    """The predict / range / normal sequence of test_gpu_bottom_sequence on every
    filter of `filters` (batch objects with the oracle wrapper's methods)."""
    rng = np.random.default_rng(seed)
    for step in range(steps):
        v = np.c_[rng.normal(0.5, 0.1, B), rng.normal(0, 0.1, B), rng.normal(0, 0.05, B)]
        for f in filters:
            f.set_velocity(v)
            f.predict(0.2)
        d, bo = BEAMS[step % 4]
        z = 10.0 / 0.866 + rng.normal(0, 0.05, B)
        cov = rng.uniform(0.01, 0.03, B)
        for f in filters:
            f.update_range(z, cov, d, bo)
        if step % 5 == 4:
            zn = V.unit(np.c_[rng.normal(0, tilt, (B, 2)), np.ones(B)])
            if per_instance_cov:
                A = rng.normal(0, 0.01, (B, 2, 2))
                cn = A @ np.swapaxes(A, 1, 2) + np.eye(2) * rng.uniform(2e-4, 8e-4, (B, 1, 1))
            else:
                cn = np.eye(2) * 4e-4
            for f in filters:
                f.update_normal(zn, cn)


def limit_tilt(n, deg=60.0):
    """pull normals further than `deg` from +e3 back onto that cone"""
    n = V.unit(n)
    c = np.cos(np.radians(deg))
    far = n[:, 2] < c
    h = V.unit(np.c_[n[:, :2], np.zeros(len(n))])
    n[far] = c * np.array([0, 0, 1.0]) + np.sqrt(1 - c * c) * h[far]
    return n


def ipose_q():
    """the dense 6x6 process noise of test_gpu_ipose_process_noise"""
    A = np.random.default_rng(4).normal(0, 1, (6, 6)) * np.r_[[0.1] * 3, [0.01] * 3][:, None]
    return A @ A.T + np.diag([1e-3] * 3 + [1e-5] * 3)


IPOSE_INIT = dict(pos_std=[0.1, 0.1, 0.2], ori_std=[0.3, 0.3, 0.3], tau=20.0, init_pos_std=[0.5, 0.5, 0.5])


def ipose_err(xa, Pa, xo, Po):
    sd = np.sqrt(np.diagonal(Po, axis1=1, axis2=2))
    e = (np.abs(xa[:, :3] - xo[:, :3]) / sd[:, :3]).max()
    e = max(e, (qlog_err(xa[:, 3:], xo[:, 3:]) / sd[:, 3:].min(axis=1)).max())
    return float(e), float(cov_err(Pa, Po).max())


def ipose_large_error_run(filters, B, corners, steps=4, seed=11):
    """0.3 rad scene, dense Q: alternate predict and visual update.  Pixel
    variance 25 px^2, not the small scene's 0.09: see visual_scene.LARGE_ERROR_PIXEL_VAR."""
    ref, p_err, q_err, marker, px = V.ipose_scene(B, seed=seed, q_sigma=0.3, corners=corners)
    fcov, fpos, cm, cam, cib = V.visual_common(B, corners, V.LARGE_ERROR_PIXEL_VAR)
    ipe = np.random.default_rng(2).normal(0, 0.1, (B, 3))
    for f in filters:
        f.init(IPOSE_INIT["pos_std"], IPOSE_INIT["ori_std"], IPOSE_INIT["tau"], ipe, IPOSE_INIT["init_pos_std"])
        f.set_process_noise(ipose_q())
        f.set_pose_reference(ref)
    for step in range(steps):
        for f in filters:
            f.predict(0.1)
            f.update_visual(px, fcov, fpos, marker, cm, cam, cib)
    return q_err


def per_instance_fcov(B, nf, seed=31):
    """differing SPD pixel covariances [B, nf, 2, 2] (px^2)"""
    rng = np.random.default_rng(seed)
    A = rng.normal(0, 0.2, (B, nf, 2, 2))
    return A @ np.swapaxes(A, -1, -2) + np.eye(2) * rng.uniform(0.05, 0.2, (B, nf, 1, 1))


def ipose_small_run(filters, B, fcov=None, steps=2, seed=11):
    """the 0.02 rad scene of test_gpu_ipose_predict_and_visual with the dense Q;
    fcov: None (the shared 0.09 px^2) or per-instance covariances"""
    ref, p_err, q_err, marker, px = V.ipose_scene(B, seed=seed)
    shared, fpos, cm, cam, cib = V.visual_common(B)
    ipe = np.random.default_rng(2).normal(0, 0.1, (B, 3))
    for f in filters:
        f.init([0.1, 0.1, 0.2], [0.01, 0.01, 0.02], 20.0, ipe, [0.5, 0.5, 0.5])
        f.set_process_noise(ipose_q())
        f.set_pose_reference(ref)
    for step in range(steps):
        for f in filters:
            f.predict(0.1)
            f.update_visual(px, shared if fcov is None else fcov, fpos, marker, cm, cam, cib)
