"""PoseUKF gate scenes shared by tests/test_pose_gate_scenes.py (CPU: oracle and
numpy twin take the constructed decisions) and tests/test_gpu_pose_gates.py
(the HIP kernels take them too).

The two gated updates, water velocity (ADCP cells) and geographic position
(GPS), accept iff !(d2 > K), d2 = nu^T S^-1 nu, K = 5.991.  Every measurement
here is CONSTRUCTED at a chosen d2 from the filter state (x, P) it will meet:
with the twin's own sigma points and measurement function, zm the predicted
measurement and S = Szz + R,

    z = zm + chol(S) u(theta) sqrt(d2),

mapped back to what the caller passes (GEO: + qrot(q, gps_in_body)[:2], then
nav_to_world; delayed XY: - (mu_xy - latched)).  So the expected decision of
every instance and cell is known before any filter runs.

Targets: K (1 - DELTA) accept, K (1 + DELTA) reject, 0.5 accept, 60 reject.
DELTA = 1e-6 is derived, not measured: a kernel within the single-call
tolerance (1e-9 sigma) has a d2 within a few 1e-9 relative of the oracle's,
and DELTA is 1000 times that.  R is non-diagonal (correlation 0.4 .. 0.5) and
theta differs per instance and cell, so the off-diagonal of S^-1 matters.

Plain numpy, the oracle and the twin; instance i's rows depend on its own
state and targets alone."""
import numpy as np

import numpy_twin as T
import oracle_ctypes as O
import pose_scenes as PS
from uwvk import abi, synth

K = 5.991
DELTA = 1e-6
GATED = ("water_velocity", "geographic")
UNGATED = ("xy", "delayed_xy", "velocity")
CELL_WEIGHTS = (0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0)  # make_pose_log's adcp_cell_weighting
GPS_IN_BODY = np.array([0.5, -0.3, 0.2])


def targets(delta=DELTA):
    """{name: (d2, accepted)}"""
    return {"K-": (K * (1.0 - delta), 1), "K+": (K * (1.0 + delta), 0), "in": (0.5, 1), "out": (60.0, 0)}


def is_threshold(name):
    return name in ("K-", "K+")


def theta(i, c=0):
    """direction angle of instance i, cell / row c: off both axes of the whitened plane"""
    return np.pi / 4 + (np.pi / 2) * ((i + c) % 4) + 0.15 * ((i + 2 * c) % 3 - 1)


def unit(th, m):
    if m == 2:
        return np.array([np.cos(th), np.sin(th)])
    assert m == 3
    return np.array([np.cos(th) * np.cos(0.5), np.sin(th) * np.cos(0.5), np.sin(0.5)])


# ---- the twin's measurement model ------------------------------------------------
def shell(log, i, dof, x, P):
    """instance i of the log as a twin holding (x, P)"""
    t = PS.twin(log, i, dof)
    t.mu, t.P = np.array(x, float), np.array(P, float)
    return t


def model(t, kind, z, R, extra=None):
    """What PoseTwin.update hands to ukf_update for this call: (zz, h, zmanifold,
    gate), zz the measurement in the space of h (GEO: navigation frame, lever
    arm taken off; delayed XY: moved by the displacement since the latch)."""
    got = {}

    def grab(zz, h, Rm, zman, gate=False):
        got.update(zz=np.array(zz, float), h=h, zman=zman, gate=gate)

    t._upd = grab
    try:
        t.update(kind, np.asarray(z, float), R, extra=extra)
    finally:
        del t._upd
    return got["zz"], got["h"], got["zman"], got["gate"]


def predicted(t, h, zman, R):
    """(zm, S) of numpy_twin.ukf_update"""
    Z = h(T.sigma_points(t.lay, t.mu, t.P))
    zm = T.vect_mean(Z) if zman else Z.mean(axis=0)
    dZ = Z - zm
    return zm, 0.5 * dZ.T @ dZ + np.asarray(R, float)


DUMMY = dict(water_velocity=np.zeros(2), geographic=np.array([synth.LAT0, synth.LON0]), xy=np.zeros(2),
             delayed_xy=np.zeros(2), velocity=np.zeros(3))


def build(t, kind, R, d2, th, extra=None):
    """The measurement of `kind` at Mahalanobis distance d2, direction th, for
    the twin's state; extra: cw / gps_in_body / the latched position."""
    _, h, zman, _ = model(t, kind, DUMMY[kind], R, extra)
    zm, S = predicted(t, h, zman, R)
    zz = zm + np.linalg.cholesky(S) @ unit(th, len(zm)) * np.sqrt(d2)
    if kind == "geographic":
        xy = zz + T.qrot(t.mu[3:7], np.asarray(extra, float))[:2]
        lat, lon = T.nav_to_world(t.loc, xy[0], xy[1])
        return np.array([lat, lon])
    if kind == "delayed_xy":
        return zz - (t.mu[0:2] - np.asarray(extra, float))
    return zz


def twin_d2(t, kind, z, R, extra=None, cross=True):
    """d2 of the call on the twin's state; cross=False: without the
    off-diagonal of S^-1 (the fault the threshold scenes must expose)"""
    zz, h, zman, _ = model(t, kind, z, R, extra)
    zm, S = predicted(t, h, zman, R)
    Si = np.linalg.inv(S)
    nu = zz - zm
    return float(nu @ Si @ nu) if cross else float((nu * nu) @ np.diag(Si))


def neighbour_cw(cw):
    """The cell weighting of the neighbouring cell: 0 <-> 1/3, 2/3 <-> 1.  (Not
    1/3 <-> 2/3: while no cell has been accepted the two water velocity states
    share their prior, and d2 is the same for cw and 1 - cw.)"""
    k = int(np.argmin(np.abs(np.array(CELL_WEIGHTS) - cw)))
    return CELL_WEIGHTS[k ^ 1]


# ---- covariances -------------------------------------------------------------------
def cov2(sa, sb, rho):
    return np.array([[sa * sa, rho * sa * sb], [rho * sa * sb, sb * sb]])


def cov_for(kind, i):
    """instance i's measurement covariance, all different; non-diagonal"""
    if kind == "water_velocity":
        return cov2(0.10 + 0.004 * i, 0.12 - 0.003 * i, 0.4 + 0.0125 * i)
    if kind == "geographic":
        return cov2(1.8 + 0.1 * i, 2.2 - 0.05 * i, 0.5 - 0.0125 * i)
    if kind in ("xy", "delayed_xy"):
        return cov2(0.6 + 0.05 * i, 0.8 - 0.02 * i, 0.45)
    assert kind == "velocity"
    A = np.array([[0.3, 0.0, 0.0], [0.12, 0.25 + 0.01 * i, 0.0], [-0.05, 0.1, 0.2]])
    return A @ A.T


ADCP_COV = cov2(0.10, 0.12, 0.45)  # the shared adcp_cov of the log scenes
GEO_COV = cov2(1.0, 1.2, 0.45)    # the shared geo_cov of the fix scene
GEO_LEVER = np.array([1.0, -0.6, 0.3])  # its gps_in_body


# ---- single calls -------------------------------------------------------------------
B_SINGLE = 8
SINGLE_PATTERN = ("K-", "K+", "in", "out", "K+", "K-", "masked", "K-")
MASKED = SINGLE_PATTERN.index("masked")
SINGLE_EPOCHS = 3  # predict + acceleration epochs after the first predict
# added to theta(i): at 0 instance 4's GEO innovation is nearly at right angles to
# the lever arm (d2 moves by 1.2e-2 without it); at 0.7 the least is 6.9e-2
SINGLE_TURN = dict(water_velocity=0.0, geographic=0.7)


def single_state(f, log):
    """The state the single calls are made from, on a batch object (engine or
    oracle wrapper): the first predict of the narrow scene, three predict +
    acceleration epochs, and the scene's DVL sample.  (The DVL update takes
    the velocity variance from 1 to 1e-4 (m/s)^2: only then do the water
    velocity states, prior 0.01, weigh in S, and a wrong cell weighting show.)"""
    PS.start(f, log)
    f.set_rotation_rate(log["gyro"][0])
    f.predict(log["dt"])
    for e in range(1, 1 + SINGLE_EPOCHS):
        f.set_rotation_rate(log["gyro"][e])
        f.predict(log["dt"])
        f.update("acceleration", log["acc"][e], log["acc_cov"])
    f.update("velocity", log["dvl"][0], log["dvl_cov"])
    return f


def single_log(dof):
    return PS.make("narrow", B_SINGLE, dof)


def single_extra(kind, x):
    """the call's extra argument: per-instance cw, the shared lever arm, the latched positions"""
    if kind == "water_velocity":
        return np.array([CELL_WEIGHTS[(i + 1) % 4] for i in range(len(x))])
    if kind == "geographic":
        return GPS_IN_BODY
    if kind == "delayed_xy":
        return x[:, 0:2] - np.array([0.3, -0.2])
    return None


def extra_of(kind, extra, i):
    return extra[i] if kind in ("water_velocity", "delayed_xy") else extra


def single_scene(dof, kind, shared, delta=DELTA):
    """One gated single call, built on the oracle's single_state under the
    current SO3 side: dict(log, kind, mu [B][2], cov ([B][2][2] or shared
    [2][2]), extra, mask, names, d2, accept).  The masked instance carries NaN
    in its value (and its covariance row when per-instance) and mask 0."""
    assert kind in GATED
    log = single_log(dof)
    x, P = single_state(O.OraclePoseBatch(B_SINGLE, dof), log).get_state()
    tg = targets(delta)
    extra = single_extra(kind, x)
    covs = np.array([cov_for(kind, 3 if shared else i) for i in range(B_SINGLE)])
    mu = np.full((B_SINGLE, 2), np.nan)
    d2 = np.full(B_SINGLE, np.nan)
    accept = np.zeros(B_SINGLE, np.uint8)
    for i, name in enumerate(SINGLE_PATTERN):
        if name == "masked":
            continue
        d2[i], accept[i] = tg[name]
        mu[i] = build(shell(log, i, dof, x[i], P[i]), kind, covs[i], d2[i], theta(i) + SINGLE_TURN[kind],
                      extra_of(kind, extra, i))
    mask =(np.arange(B_SINGLE) != MASKED).astype(np.uint8)
    cov = covs[0].copy() if shared else covs.copy()
    if not shared:
        cov[MASKED] = np.nan
    return dict(log=log, kind=kind, mu=mu, cov=cov, covs=covs, extra=extra, mask=mask, names=SINGLE_PATTERN, d2=d2,
                accept=accept, x=x, P=P)


def ungated_scene(dof, kind):
    """xy / delayed_xy / velocity at d2 = 60, per-instance R: accepted by every instance"""
    assert kind in UNGATED
    log = single_log(dof)
    x, P = single_state(O.OraclePoseBatch(B_SINGLE, dof), log).get_state()
    extra = single_extra(kind, x)
    covs = np.array([cov_for(kind, i) for i in range(B_SINGLE)])
    mu = np.array([build(shell(log, i, dof, x[i], P[i]), kind, covs[i], 60.0, theta(i), extra_of(kind, extra, i))
                   for i in range(B_SINGLE)])
    return dict(log=log, kind=kind, mu=mu, cov=covs, covs=covs, extra=extra, mask=None,
                d2=np.full(B_SINGLE, 60.0), accept=np.ones(B_SINGLE, np.uint8), x=x, P=P)


def oracle_single(sc, dof):
    """The oracle through the scene's call from single_state -> (x, P, accepted);
    the masked instance is not called (its row is the state before)."""
    B = B_SINGLE
    o = single_state(O.OraclePoseBatch(B, dof), sc["log"])
    acc = oracle_update(o, sc["kind"], sc["mu"], sc["cov"], sc["extra"], sc["mask"])
    return o.get_state() + (acc,)


def oracle_update(o, kind, mu, cov, extra=None, mask=None):
    """OraclePoseBatch.update with a mask: an instance with mask 0 is not
    called (the wrapper has no mask; its state is put back bitwise)."""
    import ctypes as C
    mu, cov = np.array(mu, float), np.array(cov, float)
    skip = [] if mask is None else [i for i in range(o.batch) if not mask[i]]
    saved = {i: C.string_at(o.ptr(i), o.sz) for i in skip}
    for i in skip:  # finite placeholders for the call that is undone below
        mu[i] = 0.0
        if cov.ndim == mu.ndim + 1:
            cov[i] = np.eye(cov.shape[-1])
    acc = o.update(kind, mu, cov, extra=extra)
    for i, raw in saved.items():
        C.memmove(o.ptr(i), raw, o.sz)
        acc[i] = 0
    return acc


# ---- ADCP cells in a log -------------------------------------------------------------
ADCP_EPOCHS = 10
ADCP_EPOCH = 6
ADCP_DVL_EPOCH = 1
# per instance, the four cells' targets: accept counts 1, 3, 2, 4, 0, 2 -- unlike
# between the halves of every pair unit, cell by cell too; a rejected cell
# followed by an accepted one (instance 0) and the reverse (instance 1)
ADCP_PATTERNS = (("K+", "K-", "out", "K+"), ("K-", "K+", "K-", "K-"), ("K-", "out", "K+", "K-"),
                 ("K-", "in", "K-", "K-"), ("K+", "out", "K+", "K+"), ("in", "K+", "K-", "out"))
ALL_REJECT = ADCP_PATTERNS[4]
ALL_ACCEPT = ADCP_PATTERNS[3]


def adcp_base_log(batch, dof, pressure):
    """make_pose_log(B, 10, "C4", adcp_every=7): ADCP at epoch 6, four cells,
    no pressure or efforts epoch; the shared adcp_cov non-diagonal; one DVL
    sample at epoch 1 (see single_state: the velocity known, the cell
    weighting shows in S).
    pressure: one pressure sample on the ADCP epoch (applied before the cells),
    so that the launch runs the pressure-capable kernels."""
    log = synth.make_pose_log(batch, ADCP_EPOCHS, "C4", dof=dof, adcp_every=7)
    assert np.flatnonzero(log["flags"] & abi.EV_ADCP).tolist() == [ADCP_EPOCH]
    assert not (log["flags"] & (abi.EV_PRESSURE | abi.EV_EFFORTS | abi.EV_DVL)).any()
    assert log["adcp_cells"] == 4 and tuple(log["adcp_cell_weighting"]) == CELL_WEIGHTS
    log["adcp_cov"] = ADCP_COV.copy()
    log["adcp"] = log["adcp"].copy()
    inst = np.arange(batch)
    log["flags"] = log["flags"].copy()
    log["flags"][ADCP_DVL_EPOCH] |= abi.EV_DVL
    log["dvl_index"] = log["dvl_index"].copy()
    log["dvl_index"][ADCP_DVL_EPOCH] = 0
    dvl = np.broadcast_to(log["truth"].dvl[ADCP_DVL_EPOCH + 1], (1, batch, 3)).copy()
    dvl[0] += 0.01 * np.stack([(inst % 3) - 1.0, (inst % 2) - 0.5, (inst % 5) - 2.0], 1)
    log["dvl"] = dvl
    if pressure:
        log["flags"][ADCP_EPOCH] |= abi.EV_PRESSURE
        log["pressure_index"] = log["pressure_index"].copy()
        log["pressure_index"][ADCP_EPOCH] = 0
        log["pressure"] = (log["truth"].pressure[ADCP_EPOCH + 1] + 40.0 * ((inst % 3) - 1.0))[None, :].copy()
    return log


def oracle_epoch_calls(o, log, e, cells=True):
    """epoch e of the log through the oracle's single calls, in run_log's
    order; -> accept counts [B][4] of the epoch.  cells=False stops before the
    ADCP cells."""
    B = log["batch"]
    cnt = np.zeros((B, 4), np.uint32)
    fl = log["flags"][e]
    o.set_rotation_rate(log["gyro"][e])
    o.predict(log["dt"])
    if fl & abi.EV_ACC:
        o.update("acceleration", log["acc"][e], log["acc_cov"])
    if fl & abi.EV_DVL:
        cnt[:, 0] += o.update("velocity", log["dvl"][log["dvl_index"][e]], log["dvl_cov"])
    if fl & abi.EV_PRESSURE:
        cnt[:, 1] += o.update("pressure", log["pressure"][log["pressure_index"][e]][:, None],
                              np.array([[log["pressure_cov"]]]), extra=log["pressure_sensor_in_imu"])
    if cells and fl & abi.EV_ADCP:
        for c in range(log["adcp_cells"]):
            cnt[:, 2] += o.update("water_velocity", log["adcp"][log["adcp_index"][e], c], log["adcp_cov"],
                                  extra=log["adcp_cell_weighting"][c])
    return cnt


def adcp_scene(batch, dof, pressure=False, patterns=ADCP_PATTERNS, delta=DELTA):
    """The log with its ADCP rows rebuilt: the oracle is advanced by single
    calls to the ADCP epoch, and cell c of every instance is built from the
    oracle's state after cell c - 1 was applied or rejected.  -> dict(log,
    names [B][4], d2 [B][4], accept [B][4], counts [B], states: the oracle's
    (x, P) before each cell and after the last)."""
    log = adcp_base_log(batch, dof, pressure)
    tg = targets(delta)
    o = PS.start(O.OraclePoseBatch(batch, dof), log)
    for e in range(ADCP_EPOCH):
        oracle_epoch_calls(o, log, e)
    oracle_epoch_calls(o, log, ADCP_EPOCH, cells=False)
    row = log["adcp_index"][ADCP_EPOCH]
    d2 = np.zeros((batch, 4))
    want = np.zeros((batch, 4), np.uint8)
    got = np.zeros((batch, 4), np.uint8)
    states = []
    for c in range(4):
        x, P = o.get_state()
        states.append((x, P))
        for i in range(batch):
            d2[i, c], want[i, c] = tg[patterns[i][c]]
            log["adcp"][row, c, i] = build(shell(log, i, dof, x[i], P[i]), "water_velocity", log["adcp_cov"],
                                           d2[i, c], theta(i, c), CELL_WEIGHTS[c])
        got[:, c] = o.update("water_velocity", log["adcp"][row, c], log["adcp_cov"], extra=CELL_WEIGHTS[c])
    states.append(o.get_state())
    return dict(log=log, names=[tuple(p) for p in patterns[:batch]], d2=d2, accept=want, oracle_accept=got,
                counts=want.sum(axis=1).astype(np.uint32), states=states)


def without_adcp(log):
    """the log with the ADCP flag cleared"""
    out = dict(log)
    out["flags"] = log["flags"].copy()
    out["flags"][ADCP_EPOCH] &= ~np.uint32(abi.EV_ADCP)
    out["adcp_index"] = log["adcp_index"].copy()
    out["adcp_index"][ADCP_EPOCH] = -1
    return out


# ---- GEO fixes in run_log_fixes ---------------------------------------------------------
XY, Z, GEO = 1, 2, 4
GEO_EPOCHS = 12
GEO_PLAN = ((2, XY | Z | GEO), (6, GEO), (11, GEO))  # after XY and Z of its epoch; alone; on the last epoch
# per instance, the three GEO rows' targets: accept counts 2, 1, 3, 0, 2, 1 (four
# values for six instances), unlike between the halves of every pair unit
GEO_PATTERNS = (("K-", "K+", "K-"), ("K+", "K-", "K+"), ("in", "K-", "K-"), ("out", "K+", "out"),
                ("K+", "K-", "K-"), ("K-", "out", "K+"))


def oracle_fix_calls(o, fx, e, counts=None, geo=True):
    """the fixes of epoch e as the oracle's single calls, XY -> Z -> GEO"""
    B = o.batch
    counts = np.zeros((B, 3), np.uint32) if counts is None else counts
    if fx["flags"][e] & XY:
        counts[:, 0] += o.update("xy", fx["xy"][fx["xy_index"][e]], fx["xy_cov"])
    if fx["flags"][e] & Z:
        counts[:, 1] += o.update("z", np.asarray(fx["z"][fx["z_index"][e]]).reshape(B, 1), fx["z_cov"].reshape(1, 1))
    if geo and fx["flags"][e] & GEO:
        counts[:, 2] += o.update("geographic", fx["geo"][fx["geo_index"][e]], fx["geo_cov"], extra=fx["gps_in_body"])
    return counts


def geo_scene(batch, dof, patterns=GEO_PATTERNS, delta=DELTA):
    """A C3 log of 12 epochs and its fixes; every GEO row is built from the
    oracle's state at the point the row is applied.  -> dict(log, fixes,
    names, d2 [B][3], accept [B][3], counts [B], states)."""
    from test_gpu_fixes import make_fixes
    log = synth.make_pose_log(batch, GEO_EPOCHS, "C3", dof=dof)
    fx = make_fixes(log, list(GEO_PLAN), xy_sd=0.3, z_sd=0.2)
    fx["gps_in_body"] = GEO_LEVER.copy()
    fx["geo_cov"] = GEO_COV.copy()
    tg = targets(delta)
    o = PS.start(O.OraclePoseBatch(batch, dof), log)
    d2 = np.zeros((batch, 3))
    want = np.zeros((batch, 3), np.uint8)
    got = np.zeros((batch, 3), np.uint8)
    states = []
    r = 0
    for e in range(GEO_EPOCHS):
        oracle_epoch_calls(o, log, e)
        if not fx["flags"][e]:
            continue
        oracle_fix_calls(o, fx, e, geo=False)
        x, P = o.get_state()
        states.append((x, P))
        row = fx["geo_index"][e]
        assert row == r
        for i in range(batch):
            d2[i, r], want[i, r] = tg[patterns[i][r]]
            fx["geo"][row, i] = build(shell(log, i, dof, x[i], P[i]), "geographic", fx["geo_cov"], d2[i, r],
                                      theta(i, r), fx["gps_in_body"])
        got[:, r] = o.update("geographic", fx["geo"][row], fx["geo_cov"], extra=fx["gps_in_body"])
        r += 1
    states.append(o.get_state())
    return dict(log=log, fixes=fx, names=[tuple(p) for p in patterns[:batch]], d2=d2, accept=want,
                oracle_accept=got, counts=want.sum(axis=1).astype(np.uint32), states=states)


def oracle_run_fixes(log, fx, dof):
    """The oracle over the log, run_log on each segment between fix epochs and
    the fixes as single calls -> (x, P, accept counts [B][4], fix counts [B][3])"""
    B, E = log["batch"], log["epochs"]
    o = PS.start(O.OraclePoseBatch(B, dof), log)
    acc = np.zeros((B, 4), np.uint32)
    facc = np.zeros((B, 3), np.uint32)
    cuts = sorted({0, E} | {int(e) + 1 for e in np.flatnonzero(fx["flags"])})
    for a, b in zip(cuts[:-1], cuts[1:]):
        acc += o.run_log(log, a, b - a)
        if fx["flags"][b - 1]:
            oracle_fix_calls(o, fx, b - 1, facc)
    return o.get_state() + (acc, facc)
