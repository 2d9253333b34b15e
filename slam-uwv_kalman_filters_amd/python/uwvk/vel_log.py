"""VelocityUKF logs without a device: VelLogRecorder turns a call sequence on
the batch surface (VelocityUKFBatch / the oracle wrapper: set_gyro,
set_efforts, predict, update_dvl, update_pressure) into the host arrays of a
uwvk_vel_log (synth.make_vel_log's layout, what upload_log takes), and
play_vel_log issues a host log as single calls to any object with that
surface, in uwvk_vel_run_log's order.  Both pure Python; they mirror
BottomLogRecorder / play_bottom_log of uwvk.small."""
import numpy as np

from . import abi


class VelLogRecorder:
    """Each predict opens an epoch with the gyro and efforts last set; the
    updates that follow belong to it.  What the log cannot express raises
    ValueError: a dt that changes, a predict before the first set_gyro or
    set_efforts, an update before the first predict, a mask, a per-instance
    covariance or a shared one that changes, two updates of one kind in an
    epoch, a DVL update after the epoch's pressure update."""

    def __init__(self, batch, dt):
        self.batch, self.dt = int(batch), float(dt)
        self.w = self.tau = None
        self.epochs = []   # dict(w=, tau=, dvl=, pressure=)
        self.cov = dict(dvl=None, pressure=None)

    def set_gyro(self, w):
        self.w = np.array(w, np.float64).reshape(self.batch, 3)

    def set_efforts(self, t):
        self.tau = np.array(t, np.float64).reshape(self.batch, 6)

    def predict(self, dt):
        if float(dt) != self.dt:
            raise ValueError("predict(%r) in a log of dt = %r" % (dt, self.dt))
        if self.w is None or self.tau is None:
            raise ValueError("predict before the first set_gyro / set_efforts")
        self.epochs.append(dict(w=self.w, tau=self.tau, dvl=None, pressure=None))

    def _update(self, kind, m, mu, shared_cov, cov, mask):
        if mask is not None:
            raise ValueError("a mask cannot be recorded")
        if cov is not None or shared_cov is None:
            raise ValueError("the log holds one shared %s covariance" % kind)
        if not self.epochs:
            raise ValueError("an update before the first predict")
        ep = self.epochs[-1]
        if ep[kind] is not None:
            raise ValueError("two %s updates in one epoch" % kind)
        if kind == "dvl" and ep["pressure"] is not None:
            raise ValueError("a DVL update after the epoch's pressure update")
        cv = np.array(shared_cov, np.float64).reshape(m, m)
        if self.cov[kind] is not None and not (self.cov[kind] == cv).all():
            raise ValueError("the %s covariance changes" % kind)
        self.cov[kind] = cv
        ep[kind] = np.array(mu, np.float64).reshape(self.batch, m)

    def update_dvl(self, mu, shared_cov=None, cov=None, mask=None):
        self._update("dvl", 3, mu, shared_cov, cov, mask)

    def update_pressure(self, mu, shared_cov=None, cov=None, mask=None):
        self._update("pressure", 1, mu, shared_cov, cov, mask)

    def log(self):
        E, B = len(self.epochs), self.batch
        flags = np.zeros(E, np.uint32)
        index = dict(dvl=np.full(E, -1, np.int32), pressure=np.full(E, -1, np.int32))
        rows = dict(dvl=[], pressure=[])
        for e, ep in enumerate(self.epochs):
            for kind, bit in (("dvl", abi.EV_DVL), ("pressure", abi.EV_PRESSURE)):
                if ep[kind] is not None:
                    flags[e] |= bit
                    index[kind][e] = len(rows[kind])
                    rows[kind].append(ep[kind])
        dcov, pcov = self.cov["dvl"], self.cov["pressure"]
        return dict(batch=B, epochs=E, dt=self.dt, flags=flags,
                    gyro=np.array([ep["w"] for ep in self.epochs]).reshape(E, B, 3),
                    efforts=np.array([ep["tau"] for ep in self.epochs]).reshape(E, B, 6),
                    dvl_index=index["dvl"], dvl=np.array(rows["dvl"]).reshape(len(rows["dvl"]), B, 3),
                    dvl_cov=np.eye(3) if dcov is None else dcov,
                    pressure_index=index["pressure"],
                    pressure=np.array(rows["pressure"]).reshape(len(rows["pressure"]), B),
                    pressure_cov=1.0 if pcov is None else float(pcov[0, 0]))


def _mask_at(entry, e, batch):
    """skip["dvl"] / skip["pressure"]: {epoch: mask of the instances that DO get
    the update}, or a collection of epochs (the whole batch is left out there)"""
    if entry is None:
        return None
    if isinstance(entry, dict):
        if e not in entry:
            return None
        return np.asarray(entry[e]).reshape(batch).astype(bool)
    return np.zeros(batch, bool) if e in entry else None


def play_vel_log(filt, log, first=0, count=None, skip=None):
    """The single calls of epochs [first, first + count) of a host log on any
    filter with VelocityUKFBatch's methods, in uwvk_vel_run_log's order:
    set_gyro, set_efforts, predict(dt), update_dvl, update_pressure.

    skip (what uwvk_vel_run_log_track leaves out when it screens a sample):
      {"predict": epochs}: at those epochs set_gyro, set_efforts and predict are
        not called (a batch of one: the single calls take no mask);
      {"dvl": {epoch: mask}, "pressure": {epoch: mask}}: the update of that
        epoch is issued with mask= (1 = updated), the masked-out samples
        replaced by zeros; a collection of epochs instead of the dict leaves the
        update out altogether.
    Returns [batch][2], the DVL and pressure updates issued to each instance."""
    E, B = int(log["epochs"]), int(log["batch"])
    count = E - first if count is None else count
    skip = skip or {}
    no_predict = set(int(e) for e in skip.get("predict", ()))
    if no_predict and B != 1:
        raise ValueError("skip['predict'] needs a batch of one (predict takes no mask)")
    issued = np.zeros((B, 2), np.int64)
    for e in range(first, first + count):
        if e not in no_predict:
            filt.set_gyro(log["gyro"][e])
            filt.set_efforts(log["efforts"][e])
            filt.predict(float(log["dt"]))
        f = int(log["flags"][e])
        for col, (kind, bit, m) in enumerate((("dvl", abi.EV_DVL, 3), ("pressure", abi.EV_PRESSURE, 1))):
            if not f & bit:
                continue
            z = np.array(log[kind][int(log[kind + "_index"][e])], np.float64).reshape(B, m)
            cov = np.asarray(log[kind + "_cov"], np.float64).reshape(m, m)
            mask = _mask_at(skip.get(kind), e, B)
            if mask is None:
                getattr(filt, "update_" + kind)(z if m == 3 else z[:, 0], cov)
                issued[:, col] += 1
            elif mask.any():
                z[~mask] = 0.0
                getattr(filt, "update_" + kind)(z if m == 3 else z[:, 0], cov, mask=mask.astype(np.uint8))
                issued[:, col] += mask
    return issued
