"""Seeded PoseUKF scenes on a configuration and a sensor set-up in which no two
numbers are alike, shared by tests/test_pose_config_scenes.py (CPU: oracle
against the numpy twin, the conditions the scenes are built for, and that
every feature moves the oracle's result) and tests/test_gpu_pose_config.py (the
HIP kernels against the oracle).

synth.default_pose_config() is degenerate where the kernels do index
arithmetic: one gyro random walk for three axes (Q's orientation block is
sigma^2 I, which neither the mounting nor the attitude turns), one max_jerk,
one constant per instability vector, taus equal in groups.  make_pose_log's
sensor set-up has diagonal covariances, no pressure lever arm, four ADCP cells,
a level truth (v_z = 0) and a northern latitude a few metres from the origin.
Here
 * distinct_config(): every such number differs from its neighbours by at
   least 1.5x; alterations(): that config with one feature reverted, permuted
   or swapped;
 * full_log(): pose_model_scenes.model_log (general model, mounted IMU,
   reverse-ordered efforts rows) with full SPD acc / dvl / adcp / efforts
   covariances, a pressure lever arm and 4, 1 or 8 ADCP cells whose samples are
   placed at the filter's expectation (d2 = ADCP_D2, inside the gate);
 * dive_log(): the same started through init_from_state with v_z = +-0.4 m/s
   and DVL samples that agree with it;
 * far(): pos0.x shifted per instance across the 64 km branch of the predict's
   latitude; lat_variants(): other latitudes; coarse(): dt = 0.01;
 * fixes_for(): XY, Z and GPS fixes with full covariances and a lever arm.

The measurements that are placed (ADCP cells, the dive's DVL rows, the fixes)
are built from the oracle's state on the SO3 side the filters under test run
on (the two sides are two filters: a cell at d2 = 1 on one is outside the
gate on the other): one log per (batch, dof, first, side).

Plain numpy, the oracle and the twin; instance i's columns depend on (seed,
first + i) alone.  The builders are cached: do not write into their arrays."""
import functools

import numpy as np

import pose_gate_scenes as GS
import pose_model_scenes as MS
from uwvk import abi

SEED = 67
DT = 1e-3
COARSE_DT = 0.01
COARSE_EPOCHS = 60

# ---- the configuration -----------------------------------------------------------
GYRO_RANDOMWALK = (1e-4, 6e-4, 1.5e-3)          # 1 : 6 : 15
MAX_JERK = (0.3, 0.5, 0.9)
# eight taus, any two a factor 1.5 apart or more; every one >= 100 * COARSE_DT
TAUS = dict(acc=20.0, gyro=4200.0, inertia=2600.0, lin=1000.0, quad=400.0, wv=250.0, adcp=1600.0, rho=650.0)
# nine values of ratio 1.5 in each instability vector, in an order that is not monotone
_ORDER = np.array([4, 0, 7, 2, 8, 1, 5, 3, 6])
INERTIA_INSTABILITY = tuple(3.0 * 1.5 ** _ORDER)
LIN_INSTABILITY = tuple(1.2 * 1.5 ** _ORDER[::-1])
QUAD_INSTABILITY = tuple(2.0 * 1.5 ** np.roll(_ORDER, 4))
LATITUDE, LONGITUDE = -0.6, 0.31
WV_LIMITS, ADCP_LIMITS, WV_SCALE = 0.15, 0.03, 0.4
WATER_DENSITY, DENSITY_LIMITS, ATMOSPHERE = 1027.5, 3.0, 100900.0


def distinct_config():
    """model_config() (bias offsets, per-axis bias instabilities) with every
    number the default leaves equal made unlike, off its default, and a
    southern latitude"""
    c = MS.model_config()
    abi.fill(c.rotation_rate.randomwalk, GYRO_RANDOMWALK)
    abi.fill(c.max_jerk, MAX_JERK)
    c.acceleration.bias_tau, c.rotation_rate.bias_tau = TAUS["acc"], TAUS["gyro"]
    m = c.model_noise_parameters
    abi.fill(m.inertia_instability, INERTIA_INSTABILITY)
    abi.fill(m.lin_damping_instability, LIN_INSTABILITY)
    abi.fill(m.quad_damping_instability, QUAD_INSTABILITY)
    m.inertia_tau, m.lin_damping_tau, m.quad_damping_tau = TAUS["inertia"], TAUS["lin"], TAUS["quad"]
    w = c.water_velocity
    w.tau, w.adcp_bias_tau = TAUS["wv"], TAUS["adcp"]
    w.limits, w.adcp_bias_limits, w.scale = WV_LIMITS, ADCP_LIMITS, WV_SCALE
    h = c.hydrostatics
    h.water_density, h.water_density_limits, h.water_density_tau = WATER_DENSITY, DENSITY_LIMITS, TAUS["rho"]
    h.atmospheric_pressure = ATMOSPHERE
    c.location.latitude, c.location.longitude = LATITUDE, LONGITUDE
    return c


def config_numbers(c=None):
    """{group: values} of the numbers distinct_config() sets apart"""
    c = c or distinct_config()
    m, w = c.model_noise_parameters, c.water_velocity
    return dict(gyro_randomwalk=list(c.rotation_rate.randomwalk), max_jerk=list(c.max_jerk),
                gyro_bias_instability=list(c.rotation_rate.bias_instability),
                acc_bias_instability=list(c.acceleration.bias_instability),
                inertia_instability=list(m.inertia_instability), lin_instability=list(m.lin_damping_instability),
                quad_instability=list(m.quad_damping_instability),
                taus=[c.acceleration.bias_tau, c.rotation_rate.bias_tau, m.inertia_tau, m.lin_damping_tau,
                      m.quad_damping_tau, w.tau, w.adcp_bias_tau, c.hydrostatics.water_density_tau])


def with_latitude(lat):
    c = distinct_config()
    c.location.latitude = lat
    return c


def alterations():
    """[(name, config, seen at 26 DOF)]: distinct_config() with one feature
    reverted, permuted or swapped.  The parameter taus and instabilities belong
    to the 27 parameter DOFs the 26-DOF layout does not have."""
    out = []

    def add(name, seen26=True):
        c = distinct_config()
        out.append((name, c, seen26))
        return c

    c = add("gyro_randomwalk_isotropic")
    abi.fill(c.rotation_rate.randomwalk, [GYRO_RANDOMWALK[1]] * 3)
    c = add("gyro_randomwalk_permuted")
    abi.fill(c.rotation_rate.randomwalk, np.roll(GYRO_RANDOMWALK, 1))
    c = add("max_jerk_permuted")
    abi.fill(c.max_jerk, np.roll(MAX_JERK, 1))
    c = add("bias_taus_swapped")
    c.acceleration.bias_tau, c.rotation_rate.bias_tau = TAUS["gyro"], TAUS["acc"]
    c = add("inertia_quad_tau_swapped", False)
    c.model_noise_parameters.inertia_tau, c.model_noise_parameters.quad_damping_tau = TAUS["quad"], TAUS["inertia"]
    c = add("wv_adcp_tau_swapped")
    c.water_velocity.tau, c.water_velocity.adcp_bias_tau = TAUS["adcp"], TAUS["wv"]
    c = add("inertia_instability_permuted", False)
    abi.fill(c.model_noise_parameters.inertia_instability, np.roll(INERTIA_INSTABILITY, 1))
    c = add("lin_instability_permuted", False)
    abi.fill(c.model_noise_parameters.lin_damping_instability, np.roll(LIN_INSTABILITY, 1))
    c = add("quad_instability_permuted", False)
    abi.fill(c.model_noise_parameters.quad_damping_instability, np.roll(QUAD_INSTABILITY, 1))
    c = add("latitude_north")
    c.location.latitude = -LATITUDE
    return out


# ---- start -----------------------------------------------------------------------
def start(f, log, cfg=None, mount_q=True):
    """init_from_config with general_uwv(), the config (distinct_config()) and
    the mounting, and the process noise for the log's dt on a batch object
    (engine or oracle wrapper).  mount_q=False: the mounting rotation left out
    of Q alone (an alteration)."""
    ib, q = MS.mounting()
    cfg = cfg or distinct_config()
    f.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, MS.general_uwv(), imu_in_body=ib)
    f.set_process_noise_from_config(cfg, log["dt"], q if mount_q else None)
    return f


def twin_from_log(log, i, dof, cfg=None):
    """instance i of the log as a numpy_twin.PoseTwin, started like start()"""
    import numpy_twin as T
    ib, q = MS.mounting()
    cd = T.cfg_dict(cfg or distinct_config())
    t = T.PoseTwin.from_config(dof, log["pos0"][i], log["pos_cov"][i], log["rot0"][i], log["rot_cov"][i], cd,
                               T.UWV.from_abi(MS.general_uwv()), imu_in_body=ib)
    t.set_noise_from_config(cd, log["dt"], q_imu_in_body=q)
    return t


def param_dict(p):
    """an abi.PoseParameter as the dict numpy_twin.PoseTwin takes"""
    return dict(imu_in_body=np.array(p.imu_in_body[:]), gyro_bias_offset=np.array(p.gyro_bias_offset[:]),
                gyro_bias_tau=p.gyro_bias_tau, acc_bias_offset=np.array(p.acc_bias_offset[:]),
                acc_bias_tau=p.acc_bias_tau, inertia_tau=p.inertia_tau, lin_damping_tau=p.lin_damping_tau,
                quad_damping_tau=p.quad_damping_tau, water_velocity_tau=p.water_velocity_tau,
                water_velocity_scale=p.water_velocity_scale, adcp_bias_tau=p.adcp_bias_tau,
                atmospheric_pressure=p.atmospheric_pressure, water_density_tau=p.water_density_tau)


def state_handles(cfg=None):
    """(loc, uwv, param) for init_from_state: synth.pose_parameter(config) plus the mounting"""
    cfg = cfg or distinct_config()
    return MS.location(cfg), MS.general_uwv(), MS.general_param(cfg)


def start_from_state(f, x, P, dt=DT, cfg=None):
    cfg = cfg or distinct_config()
    f.init_from_state(x, P, *state_handles(cfg))
    f.set_process_noise_from_config(cfg, dt, MS.mounting()[1])
    return f


def twin_from_state(x, P, i, dof, dt=DT, cfg=None):
    import numpy_twin as T
    cfg = cfg or distinct_config()
    t = T.PoseTwin(dof, x[i], P[i], (cfg.location.latitude, cfg.location.longitude),
                   T.UWV.from_abi(MS.general_uwv()), param_dict(MS.general_param(cfg)))
    t.set_noise_from_config(T.cfg_dict(cfg), dt, q_imu_in_body=MS.mounting()[1])
    return t


def shell(log, i, dof, x, P):
    """instance i as a twin holding (x, P): the measurement model pose_gate_scenes.build places samples with"""
    t = twin_from_log(log, i, dof)
    t.mu, t.P = np.array(x, float), np.array(P, float)
    return t


class on_side:
    """the oracle and the twin on one SO3 side while a scene is built"""

    def __init__(self, right):
        self.right = bool(right)

    def __enter__(self):
        import numpy_twin as T
        import oracle_ctypes as O
        self.T, self.prev = T, T.SO3_RIGHT
        T.SO3_RIGHT = self.right
        self.o = O.so3_side(self.right)
        self.o.__enter__()

    def __exit__(self, *exc):
        self.T.SO3_RIGHT = self.prev
        return self.o.__exit__(*exc)


# ---- the sensor set-up -------------------------------------------------------------
def full_cov(sd, rho):
    """diag(sd) C diag(sd) with C_ij = rho[(i + j) % len(rho)] off the diagonal"""
    sd = np.asarray(sd, float)
    n = len(sd)
    C = np.eye(n)
    for i in range(n):
        for j in range(n):
            if i != j:
                C[i, j] = rho[(i + j) % len(rho)]
    S = sd[:, None] * C * sd[None, :]
    S = 0.5 * (S + S.T)  # exactly symmetric
    np.linalg.cholesky(S)
    return S


_SA = 1e-3 / np.sqrt(DT)  # make_pose_log's accelerometer standard deviation
ACC_COV = full_cov(_SA * np.array([1.0, 1.6, 2.5]), (0.3, 0.5, 0.2))
DVL_COV = full_cov(0.01 * np.array([1.0, 2.4, 1.5]), (0.6, 0.25, 0.4))
ADCP_COV = GS.cov2(0.05, 0.08, 0.45)
# five times make_pose_log's standard deviations: at (5, 5, 5, 1, 1, 1) the velocity-only update of epoch 45
# multiplies a rounding-level difference between two correct filters by 190 (3e-12 -> 5e-10 sigma, measured
# between the pair and the one-instance kernel, which run the same code from epoch 3 on), here by 10
EFFORTS_COV = full_cov([25.0, 40.0, 60.0, 5.0, 8.0, 12.5], (0.2, 0.35, 0.5, 0.6, 0.3, 0.45))
PRESSURE_LEVER = np.array([0.4, -0.25, 0.6])   # pressure_sensor_in_imu, m
XY_COV = GS.cov2(0.05, 0.10, 0.5)
Z_COV = np.array([0.05 ** 2])
GEO_COV = GS.cov2(1.0, 1.7, 0.45)
GEO_LEVER = np.array([1.0, -0.6, 0.3])
FULL_COVS = dict(acc_cov=ACC_COV, dvl_cov=DVL_COV, adcp_cov=ADCP_COV, efforts_cov=EFFORTS_COV)
CELL_WEIGHTS = {4: np.array([2.0 / 3.0, 0.0, 1.0, 1.0 / 3.0]), 1: np.array([0.4]),
                8: np.array([0.9, 0.1, 0.55, 0.3, 1.0, 0.0, 0.7, 0.45])}
FOUR_CELL_WEIGHTS = np.array(GS.CELL_WEIGHTS)    # make_pose_log's
ADCP_D2 = 1.0                                     # of every placed cell; the gate is at 5.991
ADCP_EPOCH = MS.ADCP_EVERY - 1
DVL_EPOCHS = (MS.EARLY_DVL_EPOCH, 199)
DIVE_VZ = 0.4
# Through the ADCP epoch and no further: on the left side the oracle's own | |q| - 1 | (ukfom does not
# renormalise) reaches 1.0e-14 over 200 epochs of the dive, the bound test_gpu_pose_edges.errors holds a
# kernel's quaternion to; 6.2e-15 at 150
DIVE_EPOCHS = MS.ADCP_EVERY
DIVE_VEL_SD = 0.05   # the dive's velocity prior, m/s (the constructor's 1 m/s would let the first samples undo it)


def diagonal_of(log, key):
    """the log with one covariance replaced by its diagonal"""
    out = dict(log)
    out[key] = np.diag(np.diag(log[key]))
    return out


def dive_vz(i):
    return DIVE_VZ * (1.0 + 0.05 * (i % 3)) * (1.0 if i % 2 == 0 else -1.0)


def _epoch_by_calls(o, log, e, dof, cells, dive):
    """epoch e on the oracle by single calls in run_log's order, the rows that
    are placed (the dive's DVL sample, the ADCP cells) built from the state they meet"""
    import numpy_twin as T
    B = log["batch"]
    fl = log["flags"][e]
    assert not fl & abi.EV_EFFORTS
    o.set_rotation_rate(log["gyro"][e])
    o.predict(log["dt"])
    o.update("acceleration", log["acc"][e], log["acc_cov"])
    if fl & abi.EV_DVL:
        row = log["dvl_index"][e]
        if dive:
            x, _ = o.get_state()
            inst = log["first"] + np.arange(B)
            off = 0.01 * np.stack([(inst % 3) - 1.0, (inst % 2) - 0.5, (inst % 5) - 2.0], 1)
            log["dvl"][row] = T.qrot(T.qconj(x[:, 3:7]), x[:, 7:10]) + off
        o.update("velocity", log["dvl"][row], log["dvl_cov"])
    if fl & abi.EV_PRESSURE:
        o.update("pressure", log["pressure"][log["pressure_index"][e]][:, None], np.array([[log["pressure_cov"]]]),
                 extra=log["pressure_sensor_in_imu"])
    if fl & abi.EV_ADCP:
        row = log["adcp_index"][e]
        for c in range(cells):
            x, P = o.get_state()
            cw = log["adcp_cell_weighting"][c]
            for i in range(B):
                log["adcp"][row, c, i] = GS.build(shell(log, i, dof, x[i], P[i]), "water_velocity", log["adcp_cov"],
                                                  ADCP_D2, GS.theta(log["first"] + i, c), cw)
            o.update("water_velocity", log["adcp"][row, c], log["adcp_cov"], extra=cw)


@functools.lru_cache(maxsize=None)
def _full_log(batch, epochs, dof, first, cells, kind, right):
    import oracle_ctypes as O
    dive = kind == "dive"
    log = MS.model_log(batch, epochs, dof, first)
    if kind == "velocity_only":
        log["flags"][(log["flags"] & abi.EV_EFFORTS) != 0] |= abi.EV_EFFORTS_VELOCITY_ONLY
    log["first"], log["right"] = first, right
    for k, v in FULL_COVS.items():
        log[k] = v.copy()
    log["pressure_sensor_in_imu"] = PRESSURE_LEVER.copy()
    log["adcp_cells"] = cells
    log["adcp_cell_weighting"] = CELL_WEIGHTS[cells].copy()
    log["adcp"] = np.zeros((len(log["adcp"]), cells, batch, 2))
    log["dvl"] = log["dvl"].copy()
    placed = [e for e in range(epochs) if log["flags"][e] & abi.EV_ADCP or (dive and log["flags"][e] & abi.EV_DVL)]
    with on_side(right):
        o = O.OraclePoseBatch(batch, dof)
        if dive:
            x, P = start(o, log).get_state()
            P[:, 6:9, 6:9] = DIVE_VEL_SD ** 2 * np.eye(3)  # (the constructor's block is diagonal: no cross terms)
            for i in range(batch):
                x[i, 9] = dive_vz(first + i)
            log["x0"], log["P0"] = x, P
            start_from_state(o, x, P, log["dt"])
        else:
            start(o, log)
        at = 0
        for e in placed:
            o.run_log(log, at, e - at)
            _epoch_by_calls(o, log, e, dof, cells, dive)
            at = e + 1
    return log


def full_log(batch, epochs=MS.LOG_EPOCHS, dof=53, first=0, cells=4, right=True, velocity_only=False):
    """model_log with the full sensor set-up, its ADCP cells placed for filters
    on the given SO3 side; start it with start().  velocity_only: every efforts
    epoch in the velocity-only form, which leaves the parameter block decoupled:
    the PD and pair kernels then run the whole log at 53 DOF (after the first
    full update of model_log they hand over to the general kernel)."""
    return dict(_full_log(batch, epochs, dof, first, cells, "velocity_only" if velocity_only else "full", bool(right)))


def dive_log(batch, epochs=None, dof=53, first=0, right=True):
    """full_log whose x0 / P0 (the constructor's state with v_z = dive_vz(i))
    start it through start_from_state(f, log["x0"], log["P0"]); its DVL rows
    are the body velocity of the oracle's mean plus a fixed offset"""
    return dict(_full_log(batch, epochs or DIVE_EPOCHS, dof, first, 4, "dive", bool(right)))


def expected_counts(log):
    """run_log's accept counts [DVL, pressure, ADCP cells, efforts] when everything is accepted"""
    f = log["flags"]
    n = [int(((f & bit) != 0).sum()) for bit in (abi.EV_DVL, abi.EV_PRESSURE, abi.EV_ADCP, abi.EV_EFFORTS)]
    return [n[0], n[1], n[2] * log["adcp_cells"], n[3]]


def level_start(log):
    """the dive's start with v_z = 0 (the dive's own samples kept)"""
    x = log["x0"].copy()
    x[:, 9] = 0.0
    return x, log["P0"]


def start_scene(f, log, cfg=None):
    """start() or, for a dive, start_from_state()"""
    if "x0" in log:
        return start_from_state(f, log["x0"], log["P0"], log["dt"], cfg)
    return start(f, log, cfg)


def twins_of(log, dof, cfg=None):
    B = log["batch"]
    if "x0" in log:
        return [twin_from_state(log["x0"], log["P0"], i, dof, log["dt"], cfg) for i in range(B)]
    return [twin_from_log(log, i, dof, cfg) for i in range(B)]


def cut(log, epochs):
    """the first `epochs` epochs of the log (its sample rows kept)"""
    out = dict(log)
    out["epochs"] = epochs
    for k in ("flags", "gyro", "acc", "dvl_index", "pressure_index", "adcp_index", "efforts_index"):
        out[k] = np.ascontiguousarray(log[k][:epochs])
    return out


def coarse(log, epochs=COARSE_EPOCHS):
    """The first 60 epochs at dt = 0.01: the same samples, ten times the step
    (start() sets the process noise for the log's dt).  The DVL epoch and two
    efforts epochs fall inside; the ADCP and pressure epochs do not."""
    out = cut(log, epochs)
    out["dt"] = COARSE_DT
    assert not (out["flags"] & abi.EV_ADCP).any()
    return out


TIGHT_ROT_SD = (1e-4, 1e-4, 5e-4)   # rad


def tight(log):
    """The log with an orientation prior of 0.1 mrad (roll, pitch) and 0.5 mrad
    (yaw), scaled per instance: the earth rate's change with latitude (6e-7
    rad/s over 50 km) then shows in units of the orientation's sigma."""
    out = dict(log)
    inst = log.get("first", 0) + np.arange(log["batch"])
    sd = np.asarray(TIGHT_ROT_SD)[None, :] * (1.0 + 0.1 * (inst % 3))[:, None]
    out["rot_cov"] = np.stack([np.diag(s * s) for s in sd])
    return out


# ---- latitude -----------------------------------------------------------------------
FAR_SHIFTS = (0.0, -70e3, 50e3, 200e3, -500e3)   # m; instance i: FAR_SHIFTS[i % 5]
BRANCH_AT = 0.01                                  # rad: |x / R_M| below it is the Taylor step
LAT_VARIANTS = (0.0, -0.6, 1.4)


def far_shift(batch, first=0):
    return np.array([FAR_SHIFTS[(first + i) % len(FAR_SHIFTS)] for i in range(batch)])


def far(log, shift=None):
    """pos0.x moved per instance by far_shift (or `shift` [B])"""
    out = dict(log)
    s = far_shift(log["batch"], log.get("first", 0)) if shift is None else np.asarray(shift, float)
    out["pos0"] = log["pos0"].copy()
    out["pos0"][:, 0] += s
    out["shift"] = s
    return out


def library_branch(x, lat=LATITUDE):
    """True where the predict's latitude comes from the library sincos"""
    import numpy_twin as T
    return np.abs(np.asarray(x) / T.radii(lat)[0]) >= BRANCH_AT


PER_ROW = ("gyro", "acc", "dvl", "pressure", "efforts")  # [rows][B][...] arrays


def own_side_partner(log, i):
    """The far log as a batch of two in which instance i keeps its slot (i % 2)
    and its partner is a copy of itself: both halves of the wave on i's side"""
    out = dict(log)
    out["batch"] = 2
    for k in PER_ROW:
        out[k] = np.ascontiguousarray(np.stack([log[k][:, i]] * 2, 1))
    for k in ("pos0", "pos_cov", "rot0", "rot_cov"):
        out[k] = np.ascontiguousarray(np.stack([log[k][i]] * 2, 0))
    out["adcp"] = np.ascontiguousarray(np.stack([log["adcp"][:, :, i]] * 2, 2))
    return out



def lat_variants():
    """[(latitude, config)]: the equator (slat0 = 0), the scene's own, near the pole"""
    return [(lat, with_latitude(lat)) for lat in LAT_VARIANTS]


# ---- fixes ---------------------------------------------------------------------------
XY, Z, GEO = GS.XY, GS.Z, GS.GEO
FIX_PLAN = ((10, XY), (60, XY | Z | GEO), (120, GEO))
GEO_D2 = 1.5


def _advance(o, log, fx, a, b, counts=None, facc=None):
    """the oracle over epochs [a, b), the fixes of epoch b - 1 as single calls"""
    c = o.run_log(log, a, b - a)
    if counts is not None:
        counts += c
    if fx["flags"][b - 1]:
        GS.oracle_fix_calls(o, fx, b - 1, facc)


def fix_cuts(log, fx):
    return sorted({0, log["epochs"]} | {int(e) + 1 for e in np.flatnonzero(fx["flags"])})


@functools.lru_cache(maxsize=None)
def _fixes(batch, epochs, dof, first, right):
    import oracle_ctypes as O
    log = _full_log(batch, epochs, dof, first, 4, "full", right)
    inst = first + np.arange(batch)
    off_xy = np.stack([0.03 * ((inst % 3) - 1), 0.02 * ((inst % 4) - 1.5)], 1)
    off_z = 0.04 * ((inst % 2) - 0.5)
    fx = dict(flags=np.zeros(epochs, np.uint32), gps_in_body=GEO_LEVER.copy(), xy_cov=XY_COV.copy(),
              z_cov=Z_COV.copy(), geo_cov=GEO_COV.copy())
    rows = dict(xy=[], z=[], geo=[])
    for k in rows:
        fx[k + "_index"] = np.full(epochs, -1, np.int32)
    with on_side(right):
        o = start(O.OraclePoseBatch(batch, dof), log)
        at = 0
        for e, kinds in FIX_PLAN:
            o.run_log(log, at, e + 1 - at)
            at = e + 1
            fx["flags"][e] = kinds
            x, _ = o.get_state()
            if kinds & XY:
                fx["xy_index"][e] = len(rows["xy"])
                rows["xy"].append(x[:, :2] + off_xy)
                o.update("xy", rows["xy"][-1], fx["xy_cov"])
            if kinds & Z:
                fx["z_index"][e] = len(rows["z"])
                rows["z"].append(x[:, 2] + off_z)
                o.update("z", rows["z"][-1][:, None], fx["z_cov"].reshape(1, 1))
            if kinds & GEO:
                x, P = o.get_state()
                r = len(rows["geo"])
                fx["geo_index"][e] = r
                rows["geo"].append(np.stack([GS.build(shell(log, i, dof, x[i], P[i]), "geographic", fx["geo_cov"],
                                                      GEO_D2, GS.theta(first + i, r), fx["gps_in_body"])
                                             for i in range(batch)]))
                o.update("geographic", rows["geo"][-1], fx["geo_cov"], extra=fx["gps_in_body"])
    for k in rows:
        fx[k] = np.array(rows[k])
    return fx


def fixes_for(log, dof):
    """The fixes dict (DevicePoseFixes) of full_log(batch, epochs, dof, first):
    XY at epochs 10 and 60, Z at 60, GPS at 60 and 120.  XY and Z rows: the
    oracle's position plus fixed per-instance offsets; GPS rows placed at d2 =
    GEO_D2 and converted with the scene's own latitude."""
    assert log["adcp_cells"] == 4 and "x0" not in log and "shift" not in log and log["dt"] == DT
    return dict(_fixes(log["batch"], log["epochs"], dof, log["first"], log["right"]))


def oracle_run_fixes(log, fx, dof):
    """the oracle advanced piecewise -> (x, P, accept counts [B][4], fix counts [B][3])"""
    import oracle_ctypes as O
    B = log["batch"]
    o = start(O.OraclePoseBatch(B, dof), log)
    acc, facc = np.zeros((B, 4), np.uint32), np.zeros((B, 3), np.uint32)
    cuts = fix_cuts(log, fx)
    for a, b in zip(cuts[:-1], cuts[1:]):
        _advance(o, log, fx, a, b, acc, facc)
    return o.get_state() + (acc, facc)


# ---- single calls with full R ----------------------------------------------------------
SINGLE_EPOCHS = 3
SINGLE_KINDS = ("acceleration", "velocity", "water_velocity", "xy", "geographic", "delayed_xy", "efforts",
                "efforts_vel")


def single_state(f, log):
    """The state the single calls are made from: start(), three predict +
    acceleration epochs and the log's early DVL sample (the velocity prior of
    1 m/s narrowed: pose_model_scenes.tilted_state says why)."""
    start(f, log)
    for e in range(SINGLE_EPOCHS):
        f.set_rotation_rate(log["gyro"][e])
        f.predict(log["dt"])
        f.update("acceleration", log["acc"][e], log["acc_cov"])
    f.update("velocity", log["dvl"][log["dvl_index"][MS.EARLY_DVL_EPOCH]], log["dvl_cov"])
    f.set_rotation_rate(log["gyro"][SINGLE_EPOCHS])
    return f


def per_instance(R, i):
    """instance i's covariance: the shared one scaled by f in [0.7, 1.5] and its
    correlations shrunk by a in [0.1, 0.5], both seeded"""
    r = np.random.default_rng([SEED, int(i), 5])
    f, a = r.uniform(0.7, 1.5), r.uniform(0.1, 0.5)
    sd = np.sqrt(np.diag(R))
    C = R / np.outer(sd, sd)
    C = (1.0 - a) * C + a * np.eye(len(R))
    out = f * sd[:, None] * C * sd[None, :]
    out = 0.5 * (out + out.T)
    np.linalg.cholesky(out)
    return out


def _expected_efforts(t, only_vel):
    got = {}
    t._upd = lambda zz, h, Rm, zman, gate=False: got.update(h=h)
    try:
        t.update("efforts", np.zeros(6), EFFORTS_COV, only_vel=only_vel)
    finally:
        del t._upd
    blocks = t.model_blocks
    z = got["h"](t.mu[None])[0]
    t.model_blocks = blocks
    return z


@functools.lru_cache(maxsize=None)
def _single_calls(batch, dof, first, shared, right):
    import oracle_ctypes as O
    log = _full_log(batch, MS.EARLY_DVL_EPOCH + 1, dof, first, 4, "full", right)
    inst = first + np.arange(batch)
    with on_side(right):
        o = single_state(O.OraclePoseBatch(batch, dof), log)
        x, P = o.get_state()

        def covs(R):
            return np.stack([R if shared else per_instance(R, first + i) for i in range(batch)])

        def placed(kind, R, d2, extra):
            return np.stack([GS.build(shell(log, i, dof, x[i], P[i]), kind, R[i], d2, GS.theta(first + i),
                                      GS.extra_of(kind, extra, i)) for i in range(batch)])

        n = lambda s, k: np.stack([np.random.default_rng([SEED, int(j), s]).standard_normal(k) for j in inst])  # noqa
        cw = np.array([CELL_WEIGHTS[8][(first + i) % 8] for i in range(batch)])
        latched = x[:, 0:2] - np.array([0.3, -0.2])
        calls = []
        R = covs(ACC_COV)
        calls.append(("acceleration", "acceleration", log["acc"][SINGLE_EPOCHS], R, None, 0))
        R = covs(DVL_COV)
        calls.append(("velocity", "velocity", log["dvl"][-1] + 0.01 * n(11, 3), R, None, 0))
        R = covs(ADCP_COV)
        calls.append(("water_velocity", "water_velocity", placed("water_velocity", R, ADCP_D2, cw), R, cw, 0))
        R = covs(XY_COV)
        calls.append(("xy", "xy", x[:, 0:2] + 0.05 * n(12, 2), R, None, 0))
        R = covs(GEO_COV)
        calls.append(("geographic", "geographic", placed("geographic", R, GEO_D2, GEO_LEVER), R, GEO_LEVER, 0))
        R = covs(XY_COV)
        calls.append(("delayed_xy", "delayed_xy", latched + 0.05 * n(13, 2), R, latched, 0))
        R = covs(EFFORTS_COV)
        for name, vo in (("efforts", 0), ("efforts_vel", 1)):
            z = np.empty((batch, 6))
            for i in range(batch):
                t = shell(log, i, dof, x[i], P[i])
                t.w = log["gyro"][SINGLE_EPOCHS][i]
                z[i] = _expected_efforts(t, bool(vo)) + 2.0 * np.sqrt(np.diag(R[i])) * n(14 + vo, 6)[i]
            calls.append((name, "efforts", z, R, None, vo))
    return log, [(nm, k, mu, (R[0] if shared else R), ex, vo) for nm, k, mu, R, ex, vo in calls]


def single_calls(batch, dof, first=0, shared=True, right=True):
    """(log, [(name, kind, mu, cov, extra, only_vel)]): one call of each kind,
    each meant for single_state(f, log); cov the shared full covariance or
    per_instance()'s [B][m][m].  The gated kinds are placed at d2 = ADCP_D2 /
    GEO_D2 for the covariance they are called with."""
    log, calls = _single_calls(batch, dof, first, bool(shared), bool(right))
    return dict(log), list(calls)
