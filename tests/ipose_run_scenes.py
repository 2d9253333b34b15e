"""Recorded IndirectPoseUKF logs shared by the run tests (CPU: recorder and
uwvk_ipose_log_check; GPU: uwvk_ipose_run_log), and the list of faults that
uwvk_ipose_log_check names.

The scene is visual_scene.ipose_scene (0.02 rad) with small_scenes.ipose_q():
every epoch moves the reference poses and the markers by the same nav-frame
offset, so the geometry, and with it the recorded pixels, stays valid while
pose_ref changes; each visual row draws its own pixel noise."""
import numpy as np

import small_scenes as S
import visual_scene as V
from uwvk.small import IPoseLogRecorder

ROWS6 = (0, 1, 2, 1, 0, 2)                       # visual rows of the six-epoch log
DTS6 = (0.1, 0.05, 0.2, 0.1, 0.15, 0.1)
EINVAL, ENAN, ENOTINIT = 1, 2, 7


def init(f, B, seed=11):
    """IPoseCase.make's initial state (tests/test_gpu_small_edges.py) on any batch object"""
    ref = V.ipose_scene(B, seed)[0]
    f.init([0.1, 0.1, 0.2], [0.01, 0.01, 0.02], 20.0, np.random.default_rng(2).normal(0, 0.1, (B, 3)), [0.5, 0.5, 0.5])
    f.set_process_noise(S.ipose_q())
    f.set_pose_reference(ref)
    return f


def drive(filters, B, rows=ROWS6, dts=DTS6, fcov=None, shared_marker=False, moving_ref=True, seed=11):
    """The call sequence on every object of `filters` (a recorder among them):
    per epoch set_pose_reference, predict(dt), rows[e] visual updates.
    fcov: None (the shared 0.09 px^2) or [B][nf][2][2]; shared_marker: every
    instance watches marker 0 from reference pose 0."""
    ref, _, _, marker, px = V.ipose_scene(B, seed)
    # 4 px^2, not 0.09: rows follow each other without a predict between, and at 0.09 px^2 the
    # second of two such updates loses positive definiteness on the oracle for some batches
    # (visual_scene.LARGE_ERROR_PIXEL_VAR explains the cancellation)
    shared, fpos, cm, cam, cib = V.visual_common(B, pixel_var=V.SEVEN_PIXEL_VAR)
    if shared_marker:
        ref, px = np.tile(ref[0], (B, 1)), np.tile(px[0], (B, 1, 1))
    rng = np.random.default_rng(seed + 100)
    for e, n in enumerate(rows):
        d = np.array([0.3, -0.2, 0.05]) * e if moving_ref else np.zeros(3)
        r = ref + np.r_[d, np.zeros(4)]
        for f in filters:
            f.set_pose_reference(r)
            f.predict(dts[e % len(dts)])
        for k in range(n):
            z = px + rng.normal(0, 0.2, px.shape)
            m = (marker[0] if shared_marker else marker) + np.r_[d, np.zeros(4)]
            for f in filters:
                f.update_visual(z, shared if fcov is None else fcov, fpos, m, cm, cam, cib)


def record(B, **kw):
    rec = IPoseLogRecorder(B)
    drive((rec,), B, **kw)
    return rec.log()


def copy_log(log):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in log.items()}


def per_instance(log):
    """the same log with feature_cov and marker_pose as per-instance arrays of identical rows"""
    out, B = copy_log(log), log["batch"]
    V_, nf = len(log["features"]), log["n_features"]
    if out["feature_cov"] is None:
        out["feature_cov"] = np.ascontiguousarray(np.broadcast_to(log["shared_feature_cov"], (V_, B, nf, 4)))
        out["shared_feature_cov"] = None
    if out["marker_pose"] is None:
        out["marker_pose"] = np.ascontiguousarray(np.broadcast_to(log["shared_marker_pose"][:, None], (V_, B, 7)))
        out["shared_marker_pose"] = None
    return out


# ---- the faults of uwvk_ipose_log_check -------------------------------------
# On the six-epoch log with shared covariance and marker and a dt per epoch
# (rows 0 | 1 2 | 3 | - | 4 5 of epochs 1, 2, 3, 5).  A case is (name,
# mutate(struct, host arrays), first, count, expected code); the host arrays are
# the ones the struct points into, so a mutation in place is seen through it.
def _set(field, value):
    return lambda s, h: setattr(s, field, value)


def _at(name, idx, value):
    def m(s, h):
        h[name].reshape(-1)[idx] = value
    return m


def _arr(field, idx, value):
    def m(s, h):
        getattr(s, field)[idx] = value
    return m


def _dt(value):
    def m(s, h):
        s.dt_epoch, s.dt = None, value
    return m


def _both(a, b):
    def m(s, h):
        setattr(s, a, None)
        setattr(s, b, None)
    return m


NAN, INF = float("nan"), float("inf")
FAULTS = [
    ("first negative", None, -1, 2, EINVAL),
    ("count negative", None, 0, -1, EINVAL),
    ("range past epochs", None, 4, 3, EINVAL),
    ("first past epochs", None, 7, 0, EINVAL),
    ("dt zero", _dt(0.0), 0, 6, EINVAL),
    ("dt negative", _dt(-0.1), 0, 6, EINVAL),
    ("dt NaN", _dt(NAN), 0, 6, EINVAL),
    ("dt_epoch entry zero", _at("dt_epoch", 3, 0.0), 0, 6, EINVAL),
    ("dt_epoch entry NaN", _at("dt_epoch", 2, NAN), 2, 1, EINVAL),
    ("offset decreases", _at("visual_offset", 3, 0), 0, 6, EINVAL),
    ("offset negative", _at("visual_offset", 0, -1), 0, 6, EINVAL),
    ("offset past n_visual", _at("visual_offset", 6, 7), 0, 6, EINVAL),
    ("no offsets but rows", _set("visual_offset", None), 0, 6, EINVAL),
    ("n_visual negative", _set("n_visual", -1), 0, 0, EINVAL),
    ("no features per row", _set("n_features", 0), 0, 6, EINVAL),
    ("features NULL", _set("features", None), 1, 1, EINVAL),
    ("feature_positions NULL", _set("feature_positions", None), 1, 1, EINVAL),
    ("no feature covariance", _both("feature_cov", "shared_feature_cov"), 1, 1, EINVAL),
    ("no marker pose", _both("marker_pose", "shared_marker_pose"), 1, 1, EINVAL),
    ("dt Inf", _dt(INF), 0, 6, ENAN),
    ("dt_epoch entry Inf", _at("dt_epoch", 5, INF), 0, 6, ENAN),
    ("shared_feature_cov NaN", _at("shared_feature_cov", 5, NAN), 0, 6, ENAN),
    ("feature_positions Inf", _at("feature_positions", 2, INF), 0, 6, ENAN),
    ("shared_marker_pose NaN in a row of the range", _at("shared_marker_pose", 3 * 7 + 4, NAN), 3, 1, ENAN),
    ("cov_marker_pose NaN", _arr("cov_marker_pose", 7, NAN), 0, 6, ENAN),
    ("camera NaN", _arr("camera", 1, NAN), 0, 6, ENAN),
    ("camera_in_body Inf", _arr("camera_in_body", 6, INF), 0, 6, ENAN),
]
# faults outside [first, first + count), or in inputs that no row of the range uses: UWVK_OK
OUTSIDE = [
    ("dt_epoch entry zero outside", _at("dt_epoch", 3, 0.0), 0, 3),
    ("dt_epoch entry Inf outside", _at("dt_epoch", 0, INF), 1, 5),
    ("offset garbage outside", _at("visual_offset", 6, -5), 0, 5),
    ("offset decreases outside", _at("visual_offset", 0, 9), 1, 2),
    ("shared_marker_pose NaN in a row outside", _at("shared_marker_pose", 3 * 7 + 4, NAN), 0, 3),
    ("shared_marker_pose NaN in a later row", _at("shared_marker_pose", 0, NAN), 2, 4),
    ("features NULL, no row in the range", _set("features", None), 4, 1),
    ("camera NaN, no row in the range", _arr("camera", 0, NAN), 0, 1),
    ("no features per row, no row in the range", _set("n_features", 0), 4, 1),
    ("unused dt negative beside dt_epoch", _set("dt", -1.0), 0, 6),
]


def fault_log(B=2):
    log = record(B, shared_marker=True)
    assert log["dt_epoch"] is not None and log["shared_feature_cov"] is not None
    assert log["shared_marker_pose"] is not None and list(log["visual_offset"]) == [0, 0, 1, 3, 4, 4, 6]
    return log
