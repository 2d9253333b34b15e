"""Scenes of uwvk_pose_run_log_visual (test helper, CPU): a short C3 log with
visual-landmark rows at chosen epochs, built from the oracle's own cut run.  The
oracle runs the log to each visual epoch; there V.pose_scene puts a marker ahead
of the oracle's current estimate (it asserts zc > 1) and gives the noisy pixels
of a true pose near it; the oracle integrates the row and goes on.  What comes
back is the log, the visual dict (uwvk.engine.pose_visual_struct's layout), the
oracle's final state and, per row, how far the row moved the oracle's estimate
in units of its standard deviation before the row.

A scene is built once per argument set and shared: callers copy what they change."""
import functools

import numpy as np

import oracle_ctypes as O
import visual_scene as V
from helpers import state_err
from uwvk import synth

EPOCHS = 24
# (epoch, rows): one row, two rows, one row on the adjacent epoch, one on the last epoch
ROWS_AT = ((5, 1), (11, 2), (12, 1), (23, 1))
NF = 4
MOVE_SIGMA = 1e-3  # the bar of a scene: every row moves the oracle by at least this many sigma


def offsets(rows_at, epochs):
    """The CSR row offsets [epochs + 1] of rows_at = ((epoch, rows), ...)."""
    per = np.zeros(epochs, np.int64)
    for e, n in rows_at:
        per[e] += n
    return np.concatenate([[0], np.cumsum(per)]).astype(np.int64)


def init(f, log, dof):
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    f.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    f.set_process_noise_from_config(cfg, log["dt"])


def row_args(vis, r, B):
    """update_visual's arguments of row r (the shared arrays passed as shared)."""
    nf = vis["n_features"]
    fcov = vis["shared_feature_cov"].reshape(nf, 2, 2) if vis.get("feature_cov") is None else \
        vis["feature_cov"][r].reshape(B, nf, 2, 2)
    marker = vis["shared_marker_pose"][r] if vis.get("marker_pose") is None else vis["marker_pose"][r]
    return (vis["features"][r], fcov, vis["feature_positions"], marker, vis["cov_marker_pose"], vis["camera"],
            vis["camera_in_imu"])


def finite_mask(vis, r, B):
    """[batch] uint8: the instances whose payload of row r is finite."""
    ok = np.isfinite(vis["features"][r].reshape(B, -1)).all(1)
    if vis.get("feature_cov") is not None:
        ok &= np.isfinite(vis["feature_cov"][r].reshape(B, -1)).all(1)
    if vis.get("marker_pose") is not None:
        ok &= np.isfinite(vis["marker_pose"][r].reshape(B, -1)).all(1)
    return ok.astype(np.uint8)


def per_instance(vis, B):
    """The same rows with the feature covariance and the marker pose per instance."""
    out = dict(vis)
    n, nf = len(vis["features"]), vis["n_features"]
    if vis.get("feature_cov") is None:
        out["feature_cov"] = np.ascontiguousarray(np.broadcast_to(vis["shared_feature_cov"].reshape(1, 1, nf, 4),
                                                                  (n, B, nf, 4)))
        out["shared_feature_cov"] = None
    if vis.get("marker_pose") is None:
        out["marker_pose"] = np.ascontiguousarray(np.broadcast_to(vis["shared_marker_pose"][:, None], (n, B, 7)))
        out["shared_marker_pose"] = None
    return out


def copy_visual(vis):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vis.items()}


def cuts_of(off, first, end, extra=()):
    """The cut points of [first, end): after every epoch with a row, and after every epoch of `extra`."""
    ev = {e + 1 for e in range(first, end) if off[e + 1] > off[e]} | {e + 1 for e in extra if first <= e < end}
    return sorted({first, end} | ev)


@functools.lru_cache(maxsize=None)
def scene(B, dof=53, right=True, rows_at=ROWS_AT, epochs=EPOCHS, nf=NF, shared_marker=False):
    """dict(log, visual, x, P, moves [rows][batch], acc): see the module's docstring.
    shared_marker: one marker pose per row, the one ahead of instance 0's true
    pose, seen by every instance (their poses lie within the initial spread of
    each other; the projection asserts zc > 1)."""
    corners = V.CORNERS[:nf]
    log = synth.make_pose_log(B, epochs, "C3", dof=dof)
    off = offsets(rows_at, epochs)
    fcov, fpos, cm, cam, cib = V.visual_common(B, corners)
    feats, markers, moves = [], [], []
    acc = np.zeros((B, 4), np.uint32)
    with O.so3_side(right):
        o = O.OraclePoseBatch(B, dof)
        init(o, log, dof)
        cuts = cuts_of(off, 0, epochs)
        for a, b in zip(cuts[:-1], cuts[1:]):
            acc += o.run_log(log, a, b - a)
            for r in range(off[b - 1], off[b]):
                x0, P0 = o.get_state()
                true_t, true_q, marker, px = V.pose_scene(x0, seed=21 + 2 * r, corners=corners)
                if shared_marker:
                    marker = np.ascontiguousarray(np.broadcast_to(marker[0], marker.shape))
                    px, zc = V.project(true_t, true_q, marker, corners=corners)
                    assert (zc > 1.0).all()
                    px = px + V.pixel_noise(B, 22 + 2 * r, 0.3, nf)
                o.update_visual(px, fcov, fpos, marker, cm, cam, cib)  # raises if the oracle's update fails
                x1, _ = o.get_state()
                moves.append(state_err(x1, x0, P0, dof))
                feats.append(px)
                markers.append(marker)
        x, P = o.get_state()
    vis = dict(visual_offset=off, n_features=nf, features=np.array(feats).reshape(-1, B, nf, 2),
               feature_cov=None, shared_feature_cov=fcov.reshape(nf, 4).copy(), feature_positions=np.array(fpos),
               cov_marker_pose=np.array(cm), camera=np.array(cam), camera_in_imu=np.array(cib))
    if shared_marker:
        vis.update(marker_pose=None, shared_marker_pose=np.array(markers)[:, 0].copy())
    else:
        vis.update(marker_pose=np.array(markers).reshape(-1, B, 7), shared_marker_pose=None)
    return dict(log=log, visual=vis, x=x, P=P, moves=np.array(moves).reshape(-1, B), acc=acc)


MANY_ROWS = 66  # more than one launch's 64 rows (aug::kVisRunRows) on one epoch


@functools.lru_cache(maxsize=None)
def many_rows_scene(B=2, dof=26, rows=MANY_ROWS):
    """One epoch (5) of a 12-epoch log with `rows` one-feature rows: the row of
    scene(..., rows_at=((5, 1),), nf=1) again and again with fresh pixel noise
    (0.3 px), so the geometry that pose_scene checked (zc > 1) holds for all."""
    one = scene(B, dof, True, rows_at=((5, 1),), epochs=12, nf=1)
    vis = copy_visual(one["visual"])
    noise = 0.3 * np.random.default_rng(77).standard_normal((rows, B, 1, 2))
    noise[0] = 0.0
    vis["features"] = vis["features"][:1] + noise
    vis["marker_pose"] = np.ascontiguousarray(np.broadcast_to(vis["marker_pose"][:1], (rows, B, 7)))
    vis["visual_offset"] = offsets(((5, rows),), 12)
    sc = dict(log=one["log"], visual=vis)
    sc["x"], sc["P"] = oracle_cut_run(sc, B, dof)  # raises if an update of the oracle fails
    return sc


def oracle_cut_run(sc, B, dof, right=True):
    """The oracle over the scene once more through row_args (what the GPU tests
    compare against comes from the same arguments the single calls get)."""
    log, vis = sc["log"], sc["visual"]
    off = vis["visual_offset"]
    with O.so3_side(right):
        o = O.OraclePoseBatch(B, dof)
        init(o, log, dof)
        cuts = cuts_of(off, 0, log["epochs"])
        for a, b in zip(cuts[:-1], cuts[1:]):
            o.run_log(log, a, b - a)
            for r in range(off[b - 1], off[b]):
                o.update_visual(*row_args(vis, r, B))
        return o.get_state()


# ---- uwvk_pose_visual_check: one valid visual struct and its faults --------
EINVAL, ENAN = 1, 2
NAN, INF = float("nan"), float("inf")
CHECK_EPOCHS = 6


def check_visual(B=2, nf=3, per_inst=False):
    """A 6-epoch visual dict with rows (0 | 1 2 | 3 | - | 4 5) of epochs 1, 2, 3,
    5, the shared forms of the covariance and the marker pose (per_inst: the
    per-instance ones).  The payload values do not matter to the check."""
    rng = np.random.default_rng(3)
    n = 6
    vis = dict(visual_offset=np.array([0, 0, 1, 3, 4, 4, 6], np.int64), n_features=nf,
               features=rng.normal(300, 50, (n, B, nf, 2)), feature_cov=None,
               shared_feature_cov=np.tile(np.eye(2).reshape(4) * 0.09, (nf, 1)),
               feature_positions=rng.normal(0, 0.2, (nf, 3)), marker_pose=None,
               shared_marker_pose=np.tile([3.0, 0, 0, 1, 0, 0, 0], (n, 1)),
               cov_marker_pose=np.diag([1e-4] * 3 + [1e-5] * 3), camera=V.CAMERA.copy(), camera_in_imu=V.CAM_IN_BODY.copy())
    return per_instance(vis, B) if per_inst else vis


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


def _both(a, b):
    def m(s, h):
        setattr(s, a, None)
        setattr(s, b, None)
    return m


# (name, mutate(struct, host arrays), first, count, expected code)
FAULTS = [
    ("first negative", None, -1, 2, EINVAL),
    ("count negative", None, 0, -1, EINVAL),
    ("range past epochs", None, 4, 3, EINVAL),
    ("first past epochs", None, 7, 0, EINVAL),
    ("offset decreases", _at("visual_offset", 3, 0), 0, 6, EINVAL),
    ("offset negative", _at("visual_offset", 0, -1), 0, 6, EINVAL),
    ("offset past n_visual", _at("visual_offset", 6, 7), 0, 6, EINVAL),
    ("no offsets but rows", _set("visual_offset", None), 0, 6, EINVAL),
    ("n_visual negative", _set("n_visual", -1), 0, 0, EINVAL),
    ("no features per row", _set("n_features", 0), 0, 6, EINVAL),
    ("negative features per row", _set("n_features", -2), 1, 1, EINVAL),
    ("features NULL", _set("features", None), 1, 1, EINVAL),
    ("feature_positions NULL", _set("feature_positions", None), 1, 1, EINVAL),
    ("no feature covariance", _both("feature_cov", "shared_feature_cov"), 1, 1, EINVAL),
    ("no marker pose", _both("marker_pose", "shared_marker_pose"), 1, 1, EINVAL),
    ("shared_feature_cov NaN", _at("shared_feature_cov", 5, NAN), 0, 6, ENAN),
    ("shared_feature_cov Inf", _at("shared_feature_cov", 0, INF), 5, 1, ENAN),
    ("feature_positions Inf", _at("feature_positions", 2, INF), 0, 6, ENAN),
    ("shared_marker_pose NaN in a row of the range", _at("shared_marker_pose", 3 * 7 + 4, NAN), 3, 1, ENAN),
    ("cov_marker_pose NaN", _arr("cov_marker_pose", 7, NAN), 0, 6, ENAN),
    ("camera NaN", _arr("camera", 1, NAN), 0, 6, ENAN),
    ("camera_in_imu Inf", _arr("camera_in_imu", 6, INF), 0, 6, ENAN),
]
# faults outside [first, first + count), or in inputs that no row of the range uses: UWVK_OK
OUTSIDE = [
    ("offset garbage outside", _at("visual_offset", 6, -5), 0, 5),
    ("offset decreases outside", _at("visual_offset", 0, 9), 1, 2),
    ("shared_marker_pose NaN in a row outside", _at("shared_marker_pose", 3 * 7 + 4, NAN), 0, 3),
    ("shared_marker_pose NaN in a later row", _at("shared_marker_pose", 0, NAN), 2, 4),
    ("features NULL, no row in the range", _set("features", None), 4, 1),
    ("camera NaN, no row in the range", _arr("camera", 0, NAN), 0, 1),
    ("no features per row, no row in the range", _set("n_features", 0), 4, 1),
    ("feature_positions Inf, no row in the range", _at("feature_positions", 0, INF), 0, 1),
]
