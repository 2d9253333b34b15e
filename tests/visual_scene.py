"""Synthetic marker scenes for the visual-landmark updates and the seeded
states of the small filters (test helper).

A square marker (4 corners, half size 0.2 m) 3 m ahead of the camera; the
camera looks along the body x axis (camera z forward, x right, y down).
Image coordinates are the undistorted pinhole projection of the true corners
plus seeded pixel noise."""
import numpy as np

CAMERA = np.array([600.0, 620.0, 320.0, 240.0])  # fx, fy, cx, cy
CORNERS = 0.2 * np.array([[1.0, 1.0, 0.0], [-1.0, 1.0, 0.0], [-1.0, -1.0, 0.0], [1.0, -1.0, 0.0]])


def qmul(a, b):
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx], -1)


def qrot(q, v):
    qv = np.concatenate([np.zeros(v.shape[:-1] + (1,)), v], -1)
    qc = q * np.array([1.0, -1.0, -1.0, -1.0])
    return qmul(qmul(q, qv), qc)[..., 1:]


def qexp(rv):
    th = np.linalg.norm(rv, axis=-1, keepdims=True)
    s = np.where(th > 0, np.sin(th / 2) / np.where(th > 0, th, 1), 0.5)
    return np.concatenate([np.cos(th / 2), s * rv], -1)


def mat_to_quat(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.copysign(np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2, R[2, 1] - R[1, 2])
    y = np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2, R[0, 2] - R[2, 0])
    z = np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2, R[1, 0] - R[0, 1])
    return np.array([w, x, y, z])


# camera in body/IMU: 10 cm ahead, z_cam = x_body, x_cam = -y_body, y_cam = -z_body
CAM_IN_BODY = np.concatenate([[0.1, 0.0, 0.05], mat_to_quat(np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0],
                                                                      [0.0, -1.0, 0.0]]))])


def project(body_t, body_q, marker, cam_in_body=CAM_IN_BODY, corners=CORNERS, camera=CAMERA):
    """pixel coordinates [batch, 4, 2] of the corners for true body poses [batch, 3/4]."""
    fn = qrot(marker[..., None, 3:], corners[None]) + marker[..., None, :3]
    t = qrot(body_q[:, None] * np.array([1.0, -1.0, -1.0, -1.0]), fn - body_t[:, None])
    w = t - cam_in_body[:3]
    fc = qrot(np.broadcast_to(cam_in_body[3:] * np.array([1.0, -1.0, -1.0, -1.0]), w.shape[:-1] + (4,)), w)
    u = camera[0] * fc[..., 0] / fc[..., 2] + camera[2]
    v = camera[1] * fc[..., 1] / fc[..., 2] + camera[3]
    return np.stack([u, v], -1), fc[..., 2]


def marker_ahead(body_t, body_q, dist=3.0):
    """marker pose [batch, 7] dist metres ahead of each body pose, facing it."""
    ahead = body_t + qrot(body_q, np.broadcast_to([dist, 0.0, 0.0], body_t.shape))
    return np.concatenate([ahead, body_q], -1)


def pixel_noise(batch, seed, sigma=0.5, nf=4):
    return sigma * np.random.default_rng(seed).standard_normal((batch, nf, 2))


# three more marker points, one per side, for the 7-feature updates
CORNERS7 = np.concatenate([CORNERS, 0.2 * np.array([[0.0, 1.0, 0.0], [-1.0, 0.3, 0.0], [0.4, -1.0, 0.0]])])


# ---- seeded scenes shared by the small-filter tests (CPU twin and GPU) ------
def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def bottom_state(B, seed=5, tilt=0.1):
    """BottomUKF states: distance about 10 m, normals about +e3 (tilt: std of the
    tangent of the inclination per axis), random SPD covariances."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 4))
    x[:, 0] = 10.0 + rng.uniform(-1, 1, B)
    x[:, 1:] = unit(np.c_[rng.normal(0, tilt, (B, 2)), np.ones(B)])
    P = np.zeros((B, 3, 3))
    for i in range(B):
        A = rng.normal(0, 1, (3, 3)) * [0.3, 0.05, 0.05]
        P[i] = A @ A.T + np.diag([0.05, 0.003, 0.003])
    return x, P


def ipose_scene(B, seed=11, q_sigma=0.02, corners=CORNERS):
    """IndirectPoseUKF: reference poses, true pose errors (orientation error
    N(0, q_sigma) rad per axis), a marker ahead of each true body pose and its
    noisy pixels.  q_sigma = 0.3 is the large-error scene (|error| about 0.5 rad)."""
    rng = np.random.default_rng(seed)
    ref_t = rng.normal(0, 5, (B, 3))
    ref_q = qexp(rng.normal(0, 0.3, (B, 3)))
    p_err = rng.normal(0, 0.3, (B, 3))
    q_err = qexp(rng.normal(0, q_sigma, (B, 3)))
    body_t = ref_t + qrot(ref_q, p_err)
    body_q = qmul(ref_q, q_err)
    marker = marker_ahead(body_t, body_q)
    px, zc = project(body_t, body_q, marker, corners=corners)
    assert (zc > 1.0).all()
    px = px + pixel_noise(B, seed + 1, 0.3, len(corners))
    ref = np.concatenate([ref_t, ref_q], 1)
    return ref, p_err, q_err, marker, px


# pixel variance of the large-error scenes (q_sigma = 0.3 with an orientation
# prior of 0.3 rad): at 0.09 px^2 one update shrinks the variance about 1e6-fold,
# Sigma - C K^T cancels that many digits, and two correct fp64 restatements then
# differ by up to 5e-10 sigma (some seeds lose positive definiteness altogether);
# at 25 px^2 they agree to 1e-12 (tests/test_small_twin.py)
LARGE_ERROR_PIXEL_VAR = 25.0


# the 7-feature PoseUKF scene: 14 bearing updates at 0.09 px^2 leave the two
# restatements 1.8e-11 sigma apart, at 4 px^2 they agree to 1e-12
SEVEN_PIXEL_VAR = 4.0


def visual_common(B, corners=CORNERS, pixel_var=0.09):
    fcov = np.tile(np.eye(2) * pixel_var, (len(corners), 1, 1))
    cov_marker = np.diag([1e-4] * 3 + [1e-5] * 3)
    return fcov, corners, cov_marker, CAMERA, CAM_IN_BODY


def pose_scene(x, seed=21, corners=CORNERS):
    """marker ahead of each (perturbed) PoseUKF estimate; true pose = estimate + offset"""
    B = len(x)
    rng = np.random.default_rng(seed)
    true_t = x[:, :3] + rng.normal(0, 0.2, (B, 3))
    true_q = qmul(qexp(rng.normal(0, 0.01, (B, 3))), x[:, 3:7])
    marker = marker_ahead(true_t, true_q)
    px, zc = project(true_t, true_q, marker, corners=corners)
    assert (zc > 1.0).all()
    return true_t, true_q, marker, px + pixel_noise(B, seed + 1, 0.3, len(corners))
