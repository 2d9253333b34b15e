"""Batched BottomUKF (BottomUKF.hpp:26-53) and IndirectPoseUKF
(IndirectPoseUKF.hpp:28-86) over the C ABI (uwvk_bottom_* / uwvk_ipose_*).

Like the rest of the package there is no CPU fallback: construction raises
UWVKError(UWVK_EDEVICE) without a gfx950 device.

BottomUKFBatch.run_log runs a device-resident multi-epoch log
(uwvk_bottom_run_log, DeviceBottomLog); BottomLogRecorder turns a call sequence
into such a log's host arrays and play_bottom_log issues a host log as single
calls to any filter object (both pure Python, no device).
IndirectPoseUKFBatch.run_log, DeviceIPoseLog, IPoseLogRecorder and
play_ipose_log are the same for IndirectPoseUKF (uwvk_ipose_run_log)."""
import ctypes as C

import numpy as np

from . import abi
from .engine import VP, DeviceBuffer, _chk, _f64, _p, lib, visual_args


def _per(a, batch, tail):
    a = np.asarray(a, np.float64)
    if a.shape == tuple(tail):
        a = np.broadcast_to(a, (batch,) + tuple(tail))
    return np.ascontiguousarray(a)


class _Small:
    PREFIX = None
    STORE = DOF = None

    def __init__(self, batch, device=0):
        self.L = lib()
        self.batch, self.device = batch, device
        self.h = VP()
        getattr(self.L, self.PREFIX + "_destroy").argtypes = [VP]
        _chk(getattr(self.L, self.PREFIX + "_create")(C.c_int64(batch), device, C.byref(self.h)),
             self.PREFIX + "_create")

    def _fn(self, name):
        return getattr(self.L, "%s_%s" % (self.PREFIX, name))

    def close(self):
        if self.h:
            self._fn("destroy")(self.h)
            self.h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get_state(self):
        x = np.empty((self.batch, self.STORE))
        P = np.empty((self.batch, self.DOF, self.DOF))
        _chk(self._fn("get_state")(self.h, _p(x), _p(P)), "get_state")
        return x, P

    def get_status(self, clear=False):
        out = np.zeros(self.batch, np.uint32)
        _chk(self._fn("get_status")(self.h, _p(out), int(clear)), "get_status")
        return out


class BottomUKFBatch(_Small):
    """Batched BottomUKF: state {distance, normal (S2)}, stored (d, nx, ny, nz)."""
    PREFIX, STORE, DOF = "uwvk_bottom", 4, 3

    def init(self, x, P):
        x, P = _f64(x), _f64(P)
        _chk(self._fn("init")(self.h, _p(x), _p(P)), "bottom_init")

    def set_process_noise(self, Q):
        Q = _f64(Q)
        _chk(self._fn("set_process_noise")(self.h, _p(Q)), "bottom_set_process_noise")

    def set_velocity(self, v):
        v = _per(v, self.batch, (3,))
        _chk(self._fn("set_velocity")(self.h, _p(v)), "bottom_set_velocity")

    def predict(self, dt):
        _chk(self._fn("predict")(self.h, C.c_double(dt)), "bottom_predict")

    def update_range(self, mu, cov, direction, origin, mask=None):
        mu = _per(mu, self.batch, ())
        cv = np.asarray(cov, np.float64)
        shared = cv.ndim == 0
        cvp = None if shared else _per(cv, self.batch, ())
        d, o = _f64(direction), _f64(origin)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        _chk(self._fn("update_range")(self.h, _p(mu), _p(cvp), C.c_double(float(cv) if shared else 0.0), _p(d),
                                      _p(o), _p(m)), "bottom_update_range")

    def update_normal(self, mu, cov, mask=None):
        mu = _per(mu, self.batch, (3,))
        cv = np.asarray(cov, np.float64)
        shared = cv.shape == (2, 2)
        cvp = _f64(cv) if not shared else None
        sc = _f64(cv) if shared else None
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        _chk(self._fn("update_normal")(self.h, _p(mu), _p(cvp), _p(sc), _p(m)), "bottom_update_normal")

    @property
    def stream(self):
        f = self._fn("stream")
        f.restype, f.argtypes = VP, [VP]
        return VP(f(self.h))

    def upload_log(self, log):
        return DeviceBottomLog(log, self.device)

    def synchronize(self):
        _chk(self._fn("synchronize")(self.h), "bottom_synchronize")

    def run_log(self, dlog, first=0, count=None, every=None, sync=True, applied=None, capacity=None, mean=True,
                variance=True):
        """Epochs [first, first + count) of a DeviceBottomLog in one launch per 4096
        epochs (uwvk_bottom_run_log): per epoch set_velocity, predict(dt), the
        flagged beams' range updates in beam order, the normal update.  Bitwise
        the single calls (play_bottom_log on this class).  applied: a
        DeviceBuffer of [batch][2] uint32 the applied range / normal updates are
        added to.  every: a record after each absolute epoch e with
        (e + 1) % every == 0; returns (mean [records][batch][4], variance
        [records][batch][3]) (None for one switched off), read back after the run."""
        if dlog.batch != self.batch:
            raise ValueError("log of batch %d on a filter of batch %d" % (dlog.batch, self.batch))
        count = dlog.epochs - first if count is None else count
        ap = applied.ptr if applied is not None else None
        tr, bufs, n = None, {}, 0
        if every is not None:
            n = int(self.L.uwvk_pose_track_records(C.c_int64(first), C.c_int64(count), C.c_int64(every)))
            cap = n if capacity is None else int(capacity)
            bufs["mean"] = DeviceBuffer.empty(cap * self.batch * 4 * 8, self.device) if mean else None
            bufs["variance"] = DeviceBuffer.empty(cap * self.batch * 3 * 8, self.device) if variance else None
            t = abi.BottomTrack()
            t.every, t.capacity = int(every), cap
            t.mean, t.variance = (bufs[k].ptr if bufs[k] else None for k in ("mean", "variance"))
            tr = C.byref(t)
        _chk(self._fn("run_log")(self.h, C.byref(dlog.s), C.c_int64(first), C.c_int64(count), ap, tr),
             "bottom_run_log")
        if sync:
            self.synchronize()
        if every is None:
            return None
        out = []
        for name, w in (("mean", 4), ("variance", 3)):
            b = bufs[name]
            out.append(None if b is None else
                       (b.read(np.float64, (n, self.batch, w), self.stream) if n else np.empty((0, self.batch, w))))
        return tuple(out)


def bottom_log_struct(log, ptr):
    """abi.BottomLog of a host log (BottomLogRecorder.log()'s layout).  ptr: the
    addresses of its DEVICE arrays {velocity, range, range_var, normal} (None:
    absent).  Returns (struct, the host arrays it points into: keep them alive)."""
    s = abi.BottomLog()
    s.epochs, s.dt, s.beams = int(log["epochs"]), float(log["dt"]), int(log["beams"])
    keep = {k: np.ascontiguousarray(log[k], dtype=t) for k, t in
            (("flags", np.uint32), ("range_index", np.int32), ("normal_index", np.int32))}
    s.flags, s.range_index, s.normal_index = (_p(keep[k]) for k in ("flags", "range_index", "normal_index"))
    nb = min(s.beams, abi.BOTTOM_MAX_BEAMS) if s.beams > 0 else 0
    abi.fill(s.beam_direction, np.asarray(log["beam_direction"], float).reshape(-1)[:3 * nb])
    abi.fill(s.beam_origin, np.asarray(log["beam_origin"], float).reshape(-1)[:3 * nb])
    s.velocity, s.range, s.range_var, s.normal = (ptr.get(k) for k in ("velocity", "range", "range_var", "normal"))
    s.n_range, s.n_normal = len(log["range"]), len(log["normal"])
    s.range_cov = float(log["range_cov"])
    abi.fill(s.normal_cov, np.asarray(log["normal_cov"], float).reshape(-1))
    return s, keep


class DeviceBottomLog:
    """uwvk_bottom_log: the payloads (velocity, range, range_var, normal) in
    device memory, flags and row indices on the host.  `log` is a dict in
    BottomLogRecorder.log()'s layout."""

    def __init__(self, log, device=0):
        self.bufs, ptr = {}, {}
        for name in ("velocity", "range", "range_var", "normal"):
            if log.get(name) is not None:
                self.bufs[name] = DeviceBuffer(np.ascontiguousarray(log[name], dtype=np.float64), device)
                ptr[name] = self.bufs[name].ptr
        self.s, self.host = bottom_log_struct(log, ptr)
        self.epochs = self.s.epochs
        self.batch = int(np.asarray(log["velocity"]).shape[1])


class BottomLogRecorder:
    """Turns a call sequence on the oracle wrapper's BottomUKF methods into the
    host arrays of a uwvk_bottom_log (no device).  Each predict opens an epoch
    with the velocity last set; a new (direction, origin) pair appends a beam.
    What the log cannot express raises ValueError: a dt that changes, a mask, an
    update before the first predict, a per-instance normal covariance or one
    that changes, a ninth beam, a beam updated twice or out of beam order within
    an epoch, a range after the epoch's normal."""

    def __init__(self, batch, dt):
        self.batch, self.dt = int(batch), float(dt)
        self.v = np.zeros((self.batch, 3))
        self.beams = []          # (direction, origin)
        self.epochs = []         # dict(v=, ranges={beam: (z, var, shared)}, normal=)
        self.normal_cov = None

    def set_velocity(self, v):
        self.v = np.array(_per(v, self.batch, (3,)))

    def predict(self, dt):
        if float(dt) != self.dt:
            raise ValueError("predict(%r) in a log of dt = %r" % (dt, self.dt))
        self.epochs.append(dict(v=self.v, ranges={}, normal=None))

    def _open(self, mask):
        if mask is not None:
            raise ValueError("a mask cannot be recorded")
        if not self.epochs:
            raise ValueError("an update before the first predict")
        return self.epochs[-1]

    def update_range(self, mu, cov, direction, origin, mask=None):
        ep = self._open(mask)
        d, o = np.array(direction, float).reshape(3), np.array(origin, float).reshape(3)
        b = next((k for k, (bd, bo) in enumerate(self.beams) if (bd == d).all() and (bo == o).all()), None)
        if b is None:
            if len(self.beams) == abi.BOTTOM_MAX_BEAMS:
                raise ValueError("more than %d beams" % abi.BOTTOM_MAX_BEAMS)
            b = len(self.beams)
        if ep["normal"] is not None:
            raise ValueError("a range update after the epoch's normal update")
        if ep["ranges"] and b <= max(ep["ranges"]):
            raise ValueError("beam %d updated twice or out of beam order in one epoch" % b)
        if b == len(self.beams):
            self.beams.append((d, o))
        cv = np.asarray(cov, np.float64)
        ep["ranges"][b] = (np.array(_per(mu, self.batch, ())), np.array(_per(cv, self.batch, ())), cv.ndim == 0)

    def update_normal(self, mu, cov, mask=None):
        ep = self._open(mask)
        cv = np.asarray(cov, np.float64)
        if cv.shape != (2, 2):
            raise ValueError("a per-instance normal covariance")
        if self.normal_cov is not None and not (self.normal_cov == cv).all():
            raise ValueError("the normal covariance changes")
        if ep["normal"] is not None:
            raise ValueError("two normal updates in one epoch")
        self.normal_cov = cv.copy()
        ep["normal"] = np.array(_per(mu, self.batch, (3,)))

    def log(self):
        E, B, nb = len(self.epochs), self.batch, len(self.beams)
        flags = np.zeros(E, np.uint32)
        ri, ni = np.zeros(E, np.int32), np.zeros(E, np.int32)
        vel = np.zeros((E, B, 3))
        rows, nrm = [], []
        calls = [r for ep in self.epochs for r in ep["ranges"].values()]
        scalars = {float(r[1][0]) for r in calls if r[2]}
        shared = all(r[2] for r in calls) and len(scalars) <= 1  # one scalar covariance throughout
        for e, ep in enumerate(self.epochs):
            vel[e] = ep["v"]
            if ep["ranges"]:
                z, var = np.zeros((nb, B)), np.ones((nb, B))
                for b, (zi, ci, _) in ep["ranges"].items():
                    flags[e] |= abi.bev_beam(b)
                    z[b], var[b] = zi, ci
                ri[e] = len(rows)
                rows.append((z, var))
            if ep["normal"] is not None:
                flags[e] |= abi.BEV_NORMAL
                ni[e] = len(nrm)
                nrm.append(ep["normal"])
        return dict(
            epochs=E, dt=self.dt, flags=flags, velocity=vel, beams=nb,
            beam_direction=np.array([b[0] for b in self.beams]).reshape(nb, 3),
            beam_origin=np.array([b[1] for b in self.beams]).reshape(nb, 3),
            range_index=ri, range=np.array([r[0] for r in rows]).reshape(len(rows), nb, B),
            range_var=None if shared else np.array([r[1] for r in rows]).reshape(len(rows), nb, B),
            range_cov=scalars.pop() if shared and scalars else 0.0,
            normal_index=ni, normal=np.array(nrm).reshape(len(nrm), B, 3),
            normal_cov=np.eye(2) if self.normal_cov is None else self.normal_cov)


def play_bottom_log(filt, log, first=0, count=None):
    """The single calls of epochs [first, first + count) of a host log on any
    filter with the oracle wrapper's methods, in uwvk_bottom_run_log's order, the
    non-finite entries masked as the run skips them: a non-finite range or
    variance masks that instance out of that beam's update, a non-finite or
    zero-length normal out of the normal update (a filter that gets a mask must
    take the `mask` keyword).  A non-finite velocity has no single-call form
    (predict takes no mask): ValueError.  Returns [batch][2], the range and
    normal updates issued to each instance."""
    E = int(log["epochs"])
    count = E - first if count is None else count
    B = np.asarray(log["velocity"]).shape[1]
    issued = np.zeros((B, 2), np.int64)
    rv = log.get("range_var")
    for e in range(first, first + count):
        v = np.asarray(log["velocity"][e], float)
        if not np.isfinite(v).all():
            raise ValueError("epoch %d: a non-finite velocity cannot be played with single calls" % e)
        filt.set_velocity(v)
        filt.predict(float(log["dt"]))
        f = int(log["flags"][e])
        for b in range(int(log["beams"])):
            if not f & abi.bev_beam(b):
                continue
            row = int(log["range_index"][e])
            z = np.array(log["range"][row][b], float)
            good = np.isfinite(z)
            if rv is not None:
                cov = np.array(rv[row][b], float)
                good &= np.isfinite(cov)
                cov[~good] = 1.0
            else:
                cov = float(log["range_cov"])
            z[~good] = 0.0
            kw = {} if good.all() else dict(mask=good)
            filt.update_range(z, cov, log["beam_direction"][b], log["beam_origin"][b], **kw)
            issued[:, 0] += good
        if f & abi.BEV_NORMAL:
            n = np.array(log["normal"][int(log["normal_index"][e])], float)
            good = np.isfinite(n).all(axis=1)
            with np.errstate(invalid="ignore", over="ignore"):
                good &= (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]) > 0.0
            n[~good] = [0.0, 0.0, 1.0]
            kw = {} if good.all() else dict(mask=good)
            filt.update_normal(n, np.asarray(log["normal_cov"], float).reshape(2, 2), **kw)
            issued[:, 1] += good
    return issued


class IndirectPoseUKFBatch(_Small):
    """Batched IndirectPoseUKF: state {position_error, orientation_error}, stored t(3) q(4)."""
    PREFIX, STORE, DOF = "uwvk_ipose", 7, 6

    def init(self, pos_std, ori_std, tau, init_pos_err=None, init_pos_std=None):
        ipe = None if init_pos_err is None else _per(init_pos_err, self.batch, (3,))
        ips = None if init_pos_std is None else _f64(init_pos_std)
        a, b = _f64(pos_std), _f64(ori_std)
        _chk(self._fn("init")(self.h, _p(a), _p(b), C.c_double(tau), _p(ipe), _p(ips)), "ipose_init")

    def set_process_noise(self, Q):
        """setProcessNoiseCovariance [EXT base]: 6x6 shared by the batch."""
        Q = _f64(Q)
        _chk(self._fn("set_process_noise")(self.h, _p(Q)), "ipose_set_process_noise")

    def set_so3_right(self, on=True):
        """UWVK_OPT_SO3_RIGHT of the orientation_error: body frame q exp(d) (the
        default, MTK's SO3::boxplus) or, on=False, nav frame exp(d) q."""
        _chk(self._fn("set_option")(self.h, 5, int(bool(on))), "ipose_set_option")

    def set_pose_reference(self, pose):
        pose = _per(pose, self.batch, (7,))
        _chk(self._fn("set_pose_reference")(self.h, _p(pose)), "ipose_set_pose_reference")

    def predict(self, dt):
        _chk(self._fn("predict")(self.h, C.c_double(dt)), "ipose_predict")

    def update_visual(self, features, feature_cov, feature_positions, marker_pose, cov_marker_pose, camera,
                      camera_in_body, mask=None):
        args, keep = visual_args(self.batch, features, feature_cov, feature_positions, marker_pose,
                                 cov_marker_pose, camera, camera_in_body, mask)
        _chk(self._fn("update_visual")(self.h, *args), "ipose_update_visual")

    def get_corrected_pose(self):
        out = np.empty((self.batch, 7))
        _chk(self._fn("get_corrected_pose")(self.h, _p(out)), "ipose_get_corrected_pose")
        return out

    @property
    def stream(self):
        f = self._fn("stream")
        f.restype, f.argtypes = VP, [VP]
        return VP(f(self.h))

    def upload_log(self, log):
        return DeviceIPoseLog(log, self.device)

    def synchronize(self):
        _chk(self._fn("synchronize")(self.h), "ipose_synchronize")

    def run_log(self, dlog, first=0, count=None, every=None, sync=True, applied=None, capacity=None, mean=True,
                variance=True, corrected=True):
        """Epochs [first, first + count) of a DeviceIPoseLog in one launch per 4096
        epochs (uwvk_ipose_run_log): per epoch set_pose_reference, predict(dt of
        that epoch), one update_visual per visual row.  Bitwise the single calls
        (play_ipose_log on this class).  applied: a DeviceBuffer of [batch] uint32
        the applied visual rows are added to.  every: a record after each
        absolute epoch e with (e + 1) % every == 0; returns (mean
        [records][batch][7], variance [records][batch][6], corrected
        [records][batch][7]) (None for one switched off), read back after the run."""
        if dlog.batch != self.batch:
            raise ValueError("log of batch %d on a filter of batch %d" % (dlog.batch, self.batch))
        count = dlog.epochs - first if count is None else count
        ap = applied.ptr if applied is not None else None
        widths = (("mean", 7, mean), ("variance", 6, variance), ("corrected", 7, corrected))
        tr, bufs, n = None, {}, 0
        if every is not None:
            n = int(self.L.uwvk_pose_track_records(C.c_int64(first), C.c_int64(count), C.c_int64(every)))
            cap = n if capacity is None else int(capacity)
            t = abi.IPoseTrack()
            t.every, t.capacity = int(every), cap
            for name, w, on in widths:
                bufs[name] = DeviceBuffer.empty(cap * self.batch * w * 8, self.device) if on else None
                setattr(t, name, bufs[name].ptr if on else None)
            tr = C.byref(t)
        _chk(self._fn("run_log")(self.h, C.byref(dlog.s), C.c_int64(first), C.c_int64(count), ap, tr),
             "ipose_run_log")
        if sync:
            self.synchronize()
        if every is None:
            return None
        out = []
        for name, w, _ in widths:
            b = bufs[name]
            out.append(None if b is None else
                       (b.read(np.float64, (n, self.batch, w), self.stream) if n else np.empty((0, self.batch, w))))
        return tuple(out)


IPOSE_DEVICE_ARRAYS = ("pose_ref", "features", "feature_cov", "marker_pose")


def ipose_log_struct(log, ptr):
    """abi.IPoseLog of a host log (IPoseLogRecorder.log()'s layout).  ptr: the
    addresses of its DEVICE arrays {pose_ref, features, feature_cov, marker_pose}
    (None: absent).  Returns (struct, the host arrays it points into: keep them alive)."""
    s = abi.IPoseLog()
    s.epochs, s.dt = int(log["epochs"]), float(log["dt"])
    s.n_features = int(log["n_features"])
    keep = {}
    for k, t in (("dt_epoch", np.float64), ("visual_offset", np.int64), ("shared_feature_cov", np.float64),
                 ("feature_positions", np.float64), ("shared_marker_pose", np.float64)):
        if log.get(k) is not None:
            keep[k] = np.ascontiguousarray(log[k], dtype=t)
        setattr(s, k, _p(keep.get(k)))
    s.n_visual = 0 if log.get("features") is None else len(log["features"])
    for k in IPOSE_DEVICE_ARRAYS:
        setattr(s, k, ptr.get(k))
    abi.fill(s.cov_marker_pose, np.asarray(log["cov_marker_pose"], float).reshape(-1))
    abi.fill(s.camera, np.asarray(log["camera"], float).reshape(-1))
    abi.fill(s.camera_in_body, np.asarray(log["camera_in_body"], float).reshape(-1))
    return s, keep


class DeviceIPoseLog:
    """uwvk_ipose_log: the payloads (pose_ref, features, feature_cov,
    marker_pose) in device memory, the steps, row offsets and shared inputs on
    the host.  `log` is a dict in IPoseLogRecorder.log()'s layout."""

    def __init__(self, log, device=0):
        self.bufs, ptr = {}, {}
        for name in IPOSE_DEVICE_ARRAYS:
            if log.get(name) is not None and np.asarray(log[name]).size:
                self.bufs[name] = DeviceBuffer(np.ascontiguousarray(log[name], dtype=np.float64), device)
                ptr[name] = self.bufs[name].ptr
        self.s, self.host = ipose_log_struct(log, ptr)
        self.epochs = self.s.epochs
        self.batch = int(log["batch"])


class IPoseLogRecorder:
    """Turns a call sequence on the oracle wrapper's IndirectPoseUKF methods into
    the host arrays of a uwvk_ipose_log (no device).  Each predict opens an epoch
    with the reference last set and its own dt; each update_visual appends a
    visual row to the open epoch.  A feature covariance [nf][2][2] given to
    every row with the same values is the log's shared one, otherwise every row
    gets a per-instance array; a marker pose [7] on every row is the log's
    shared one per row, otherwise per instance.
    What the log cannot express raises ValueError: a mask, an update before the
    first predict, a feature count that changes, feature positions, a marker
    covariance, a camera or a camera pose that change, a reference first set
    after the first predict, or set between an epoch's predict and one of its
    updates (or after the last predict)."""

    def __init__(self, batch):
        self.batch = int(batch)
        self.ref, self.ref_pending = None, False
        self.epochs = []   # dict(ref=, dt=, rows=[(features, fcov, fcov_shared, marker, marker_shared)])
        self.shared = None  # (feature_positions, cov_marker_pose, camera, camera_in_body)

    def set_pose_reference(self, pose):
        if self.ref is None and self.epochs:
            raise ValueError("a reference first set after the first predict")
        self.ref, self.ref_pending = np.array(_per(pose, self.batch, (7,))), True

    def predict(self, dt):
        self.epochs.append(dict(ref=self.ref, dt=float(dt), rows=[]))
        self.ref_pending = False

    def update_visual(self, features, feature_cov, feature_positions, marker_pose, cov_marker_pose, camera,
                      camera_in_body, mask=None):
        if mask is not None:
            raise ValueError("a mask cannot be recorded")
        if not self.epochs:
            raise ValueError("an update before the first predict")
        if self.ref_pending:
            raise ValueError("a reference set between an epoch's predict and its update")
        f = np.array(features, np.float64)
        if f.ndim != 3 or f.shape[0] != self.batch or f.shape[2] != 2 or f.shape[1] < 1:
            raise ValueError("features of shape %r" % (f.shape,))
        nf = f.shape[1]
        shared = (np.array(feature_positions, np.float64).reshape(-1, 3), np.array(cov_marker_pose, np.float64).reshape(36),
                  np.array(camera, np.float64).reshape(4), np.array(camera_in_body, np.float64).reshape(7))
        if len(shared[0]) != nf:
            raise ValueError("%d feature positions for %d features" % (len(shared[0]), nf))
        if self.shared is None:
            self.shared = shared
        elif len(self.shared[0]) != nf:
            raise ValueError("the feature count changes (%d, was %d)" % (nf, len(self.shared[0])))
        elif not all(np.array_equal(a, b) for a, b in zip(self.shared, shared)):
            raise ValueError("feature positions, marker covariance, camera or camera pose change")
        fc = np.array(feature_cov, np.float64)
        fc_shared = fc.shape in ((nf, 2, 2), (nf, 4))
        fc = fc.reshape(nf, 4) if fc_shared else fc.reshape(self.batch, nf, 4)
        mp = np.array(marker_pose, np.float64)
        mp_shared = mp.ndim == 1
        self.epochs[-1]["rows"].append((f, fc, fc_shared, mp.reshape(7) if mp_shared else mp.reshape(self.batch, 7),
                                        mp_shared))

    def log(self):
        if self.ref_pending and self.epochs:
            raise ValueError("a reference set after the last predict")
        E, B = len(self.epochs), self.batch
        rows = [r for ep in self.epochs for r in ep["rows"]]
        V = len(rows)
        nf = len(self.shared[0]) if self.shared else 0
        off = np.zeros(E + 1, np.int64)
        off[1:] = np.cumsum([len(ep["rows"]) for ep in self.epochs])
        fc_shared = V > 0 and all(r[2] and np.array_equal(r[1], rows[0][1]) for r in rows)
        mp_shared = V > 0 and all(r[4] for r in rows)
        dts = np.array([ep["dt"] for ep in self.epochs], np.float64)
        one_dt = E > 0 and (dts == dts[0]).all()
        sh = self.shared or (np.zeros((0, 3)), np.zeros(36), np.zeros(4), np.zeros(7))
        return dict(
            batch=B, epochs=E, dt=float(dts[0]) if one_dt else 0.0, dt_epoch=None if one_dt or E == 0 else dts,
            pose_ref=None if self.ref is None else np.array([ep["ref"] for ep in self.epochs]).reshape(E, B, 7),
            visual_offset=off, n_features=nf,
            features=np.array([r[0] for r in rows]).reshape(V, B, nf, 2),
            feature_cov=None if fc_shared or V == 0 else
            np.array([np.broadcast_to(r[1], (B, nf, 4)) for r in rows]).reshape(V, B, nf, 4),
            shared_feature_cov=rows[0][1].copy() if fc_shared else None,
            feature_positions=sh[0],
            marker_pose=None if mp_shared or V == 0 else
            np.array([np.broadcast_to(r[3], (B, 7)) for r in rows]).reshape(V, B, 7),
            shared_marker_pose=np.array([r[3] for r in rows]).reshape(V, 7) if mp_shared else None,
            cov_marker_pose=sh[1].reshape(6, 6), camera=sh[2], camera_in_body=sh[3])


def play_ipose_log(filt, log, first=0, count=None):
    """The single calls of epochs [first, first + count) of a host log on any
    filter with the oracle wrapper's methods, in uwvk_ipose_run_log's order, the
    non-finite entries handled as the run handles them: an instance with a
    non-finite feature, feature covariance or marker pose at a row is masked out
    of that row's update (a filter that gets a mask must take the `mask`
    keyword); an instance with a non-finite reference keeps the last finite one
    this replay gave it (none yet: ValueError, the handle's own is not
    readable).  Returns [batch], the visual rows issued to each instance."""
    E, B, nf = int(log["epochs"]), int(log["batch"]), int(log["n_features"])
    count = E - first if count is None else count
    issued = np.zeros(B, np.int64)
    cur = None
    for e in range(first, first + count):
        if log.get("pose_ref") is not None:
            ref = np.array(log["pose_ref"][e], float)
            bad = ~np.isfinite(ref).all(axis=1)
            if bad.any():
                if cur is None:
                    raise ValueError("epoch %d: a non-finite reference before any finite one cannot be played" % e)
                ref[bad] = cur[bad]
            cur = ref
            filt.set_pose_reference(ref)
        filt.predict(float(log["dt"] if log.get("dt_epoch") is None else log["dt_epoch"][e]))
        for row in range(int(log["visual_offset"][e]), int(log["visual_offset"][e + 1])):
            f = np.array(log["features"][row], float)
            good = np.isfinite(f).all(axis=(1, 2))
            if log.get("feature_cov") is not None:
                fc = np.array(log["feature_cov"][row], float).reshape(B, nf, 2, 2)
                good &= np.isfinite(fc).all(axis=(1, 2, 3))
                fc[~good] = np.eye(2)
            else:
                fc = np.asarray(log["shared_feature_cov"], float).reshape(nf, 2, 2)
            if log.get("marker_pose") is not None:
                mp = np.array(log["marker_pose"][row], float)
                good &= np.isfinite(mp).all(axis=1)
                mp[~good] = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
            else:
                mp = np.asarray(log["shared_marker_pose"][row], float)
            f[~good] = 0.0
            kw = {} if good.all() else dict(mask=good)
            filt.update_visual(f, fc, log["feature_positions"], mp, log["cov_marker_pose"], log["camera"],
                               log["camera_in_body"], **kw)
            issued += good
    return issued
