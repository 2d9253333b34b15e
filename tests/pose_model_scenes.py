"""Seeded PoseUKF scenes on a general vehicle model and a mounted IMU, shared by
tests/test_pose_model_scenes.py (CPU: oracle against the numpy twin, and that
every feature of the scene moves the result) and tests/test_gpu_pose_model.py
(the HIP kernels against the oracle).

synth.default_uwv() is diagonal, neutrally buoyant, with its centres on the z
axis, and every other scene mounts the IMU at the body origin without a
rotation: a transposed table, a row-major 3x3 block, swapped centres or a
dropped lever arm are all invisible there.  Here
 * general_uwv(): dense non-symmetric 6x6 inertia and damping matrices,
   W != B, general centres of gravity and buoyancy;
 * mounting() / model_config(): imu_in_body with a lever arm and a rotation,
   non-zero bias offsets, unequal per-axis bias instabilities (the rotated
   bias blocks of Sigma and Q are then non-diagonal);
 * tilted_state(): (x, P) for init_from_state, roll and pitch of 0.1-0.4 rad,
   3-D velocity, acceleration and water velocity, every instance unlike;
 * efforts_calls(): the two BodyEfforts forms for the state one predict
   later, at a body rate of a few tenths of a rad/s, alone and in the
   sequence full -> predict -> velocity-only;
 * model_log(): 200 epochs of a compressed C4 log with five efforts epochs.

Plain numpy; instance i's columns depend on (seed, first + i) alone."""
import functools

import numpy as np

from uwvk import abi, synth

SEED = 61
LEVER = (0.3, -0.1, 0.05)             # imu_in_body translation, m
MOUNT_ROTVEC = (0.4, -0.3, 0.6)       # imu_in_body rotation vector, rad
GYRO_BIAS_OFFSET = (0.02, -0.01, 0.015)
ACC_BIAS_OFFSET = (0.05, -0.08, 0.03)
GYRO_BIAS_INSTABILITY = (1e-5, 3e-5, 2e-5)
ACC_BIAS_INSTABILITY = (1e-4, 3e-4, 2e-4)
RATE = np.array([0.2, -0.3, 0.4])     # body rate of the single calls and of model_log, rad/s
EFFORTS_COV = np.diag([25.0, 25.0, 25.0, 1.0, 1.0, 1.0])
IDX = [0, 1, 5]                       # the rows / columns the state overlays
DT = 1e-3                             # the step of the single calls
STATE_DVL_COV = np.eye(3) * 1e-4      # the two samples that narrow tilted_state's prior
STATE_ACC_COV = np.eye(3) * 1e-3

# ---- model_log's schedule (epoch indices) ------------------------------------
LOG_EPOCHS = 200
EFFORTS_EPOCHS = (2, 45, 90, 135, 180)          # full, velocity-only, full, velocity-only, full
ADCP_EVERY = 150                                 # the ADCP epoch is 149; pressure 99, 199; DVL 199
EARLY_DVL_EPOCH = 20


def _rng(i, stream):
    return np.random.default_rng([SEED, int(i), stream])


def _qmul(a, b):
    return synth._qmul(np.asarray(a, float), np.asarray(b, float))


def _qexp(v):
    v = np.asarray(v, float)
    th = np.linalg.norm(v)
    return np.concatenate([[np.cos(th / 2)], np.sin(th / 2) / th * v])


def _rotm(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


# ---- the vehicle model -----------------------------------------------------------
def coupled(D, rng):
    """diag D plus a dense coupling: entry (i, j), i != j, is s_ij + k_ij with
    s symmetric, |s_ij| <= 0.02 sqrt(D_i D_j), and k antisymmetric,
    0.03 sqrt(D_i D_j) <= |k_ij| <= 0.06 sqrt(D_i D_j).  So |A - A^T|_ij >=
    0.06 sqrt(D_i D_j) and |A_ij| >= 0.01 sqrt(D_i D_j) in every off-diagonal
    pair, and the symmetric part is positive definite by Gershgorin (five
    off-diagonals of at most 0.02 each on the unit-diagonal scaling)."""
    sc = np.sqrt(np.outer(D, D))
    S = np.triu(rng.uniform(-0.02, 0.02, (6, 6)), 1)
    K = np.triu(rng.uniform(0.03, 0.06, (6, 6)) * rng.choice([-1.0, 1.0], (6, 6)), 1)
    return np.diag(D) + sc * (S + S.T + K - K.T)


def general_arrays():
    M0, Dl0, Dq0 = synth.uwv_arrays(synth.default_uwv())
    rng = np.random.default_rng([SEED, 1000])
    return (coupled(1.3 * np.diag(M0), rng), coupled(0.7 * np.diag(Dl0), rng), coupled(1.5 * np.diag(Dq0), rng))


def make_uwv(M, Dl, Dq, weight=2100.0, buoyancy=1950.0, cog=(0.02, -0.01, 0.03), cob=(0.01, 0.015, 0.06)):
    u = abi.UWVParams()
    abi.fill(u.inertia_matrix, np.asarray(M).ravel())
    abi.fill(u.damping_matrices[0], np.asarray(Dl).ravel())
    abi.fill(u.damping_matrices[1], np.asarray(Dq).ravel())
    u.weight, u.buoyancy = weight, buoyancy
    abi.fill(u.distance_body2centerofgravity, cog)
    abi.fill(u.distance_body2centerofbuoyancy, cob)
    return u


def general_uwv():
    return make_uwv(*general_arrays())


def altered_uwv(name):
    """general_uwv() with one feature taken away (tests/test_pose_model_scenes.py)"""
    M, Dl, Dq = general_arrays()
    d = lambda A: np.diag(np.diag(A))  # noqa: E731
    kw = {}
    if name == "Mt":
        M = M.T
    elif name == "Dlt":
        Dl = Dl.T
    elif name == "Dqt":
        Dq = Dq.T
    elif name == "diagonal":
        M, Dl, Dq = d(M), d(Dl), d(Dq)
    elif name == "cog0":
        kw["cog"] = (0.0, 0.0, 0.0)
    elif name == "cob0":
        kw["cob"] = (0.0, 0.0, 0.0)
    elif name == "W=B":
        kw["weight"] = kw["buoyancy"] = 1950.0
    else:
        raise KeyError(name)
    return make_uwv(M, Dl, Dq, **kw)


# ---- the mounting and the configuration ------------------------------------------
def mounting(lever=LEVER, rotvec=MOUNT_ROTVEC):
    """(imu_in_body [7]: translation + unit quaternion (w, x, y, z), that quaternion)"""
    q = _qexp(rotvec) if np.any(rotvec) else np.array([1.0, 0.0, 0.0, 0.0])
    return np.concatenate([np.asarray(lever, float), q]), q


def model_config():
    """default_pose_config() with bias offsets and unequal per-axis bias instabilities"""
    c = synth.default_pose_config()
    abi.fill(c.rotation_rate.bias_offset, GYRO_BIAS_OFFSET)
    abi.fill(c.acceleration.bias_offset, ACC_BIAS_OFFSET)
    abi.fill(c.rotation_rate.bias_instability, GYRO_BIAS_INSTABILITY)
    abi.fill(c.acceleration.bias_instability, ACC_BIAS_INSTABILITY)
    return c


def general_param(cfg=None, lever=LEVER, rotvec=MOUNT_ROTVEC):
    """PoseParameter as the first constructor derives it from cfg and mounting()
    (PoseUKF.cpp:358-371): the lever arm, the bias offsets turned into the body frame"""
    cfg = cfg or model_config()
    p = synth.pose_parameter(cfg)
    R = _rotm(mounting(lever, rotvec)[1])
    abi.fill(p.imu_in_body, lever)
    abi.fill(p.gyro_bias_offset, R @ np.array(cfg.rotation_rate.bias_offset[:]))
    abi.fill(p.acc_bias_offset, R @ np.array(cfg.acceleration.bias_offset[:]))
    return p


def location(cfg=None):
    cfg = cfg or model_config()
    return abi.Location(cfg.location.latitude, cfg.location.longitude, cfg.location.altitude)


# ---- per-instance truth ----------------------------------------------------------
def attitude(i, level=False):
    """unit quaternion of instance i: yaw in +-1 rad, then pitch, then roll, each
    of magnitude 0.1-0.4 rad with its own sign (level: yaw alone)"""
    r = _rng(i, 0)
    yaw = r.uniform(-1.0, 1.0)
    tilt = r.uniform(0.1, 0.4, 2) * r.choice([-1.0, 1.0], 2)
    q = _qexp([0.0, 0.0, yaw])
    if not level:
        q = _qmul(_qmul(q, _qexp([0.0, tilt[1], 0.0])), _qexp([tilt[0], 0.0, 0.0]))
    return q


def kinematics(i):
    """(velocity, acceleration [nav], water velocity [2], gyro) of instance i"""
    r = _rng(i, 1)
    v = np.array([0.8, -0.3, 0.2]) + 0.1 * r.standard_normal(3)
    a = np.array([0.05, -0.02, 0.03]) + 0.01 * r.standard_normal(3)
    wv = np.array([0.08, -0.04]) + 0.02 * r.standard_normal(2)
    w = RATE + 0.05 * r.standard_normal(3)
    return v, a, wv, w


def rot0(batch, first=0, level=False):
    return np.stack([attitude(first + i, level) for i in range(batch)])


def rates(batch, first=0):
    return np.stack([kinematics(first + i)[3] for i in range(batch)])


def tilted_state(batch, dof=53, first=0, uwv=None, lever=LEVER, rotvec=MOUNT_ROTVEC, level=False):
    """(x, P) for init_from_state: the oracle's init_from_config on the model
    (general_uwv() unless given), model_config() and the mounting, started at
    attitude(i); then the mean's velocity, acceleration and water velocity set
    to kinematics(i), and one DVL and one accelerometer update with samples that
    agree with that mean.  Sigma keeps the constructor's rotated bias blocks."""
    if uwv is None and lever == LEVER and rotvec == MOUNT_ROTVEC and not level:
        x, P = _tilted_state(batch, dof, first)
        return x.copy(), P.copy()
    return _make_tilted_state(batch, dof, first, uwv, lever, rotvec, level)


@functools.lru_cache(maxsize=None)
def _tilted_state(batch, dof, first):
    return _make_tilted_state(batch, dof, first, None, LEVER, MOUNT_ROTVEC, False)


def _make_tilted_state(batch, dof, first, uwv, lever, rotvec, level):
    import oracle_ctypes as O
    with O.so3_side(True):  # one state whatever side the filters under test run on
        return _tilted_on_oracle(O.OraclePoseBatch(batch, dof), batch, dof, first, uwv, lever, rotvec, level)


def _tilted_on_oracle(o, batch, dof, first, uwv, lever, rotvec, level):
    base = synth.make_pose_log(batch, 1, "C3", dof=dof, first_instance=first)
    o.init_from_config(base["pos0"], base["pos_cov"], rot0(batch, first, level), base["rot_cov"], model_config(),
                       uwv or general_uwv(), imu_in_body=mounting(lever, rotvec)[0])
    x, P = o.get_state()
    L = abi.layout(dof)
    zv, za = np.empty((batch, 3)), np.empty((batch, 3))
    for i in range(batch):
        v, a, wv, _ = kinematics(first + i)
        x[i, 7:10], x[i, 10:13] = v, a
        x[i, L["s_wv"]:L["s_wv"] + 2] = wv
        Rt = _rotm(x[i, 3:7]).T
        zv[i] = Rt @ v
        za[i] = Rt @ (a + np.array([0.0, 0.0, x[i, L["s_grav"]]])) + x[i, L["s_ba"]:L["s_ba"] + 3]
    # the constructor's velocity and acceleration priors (1 m/s, 3.2 m/s^2) narrowed by one DVL and one
    # accelerometer sample that agree with the mean: Sigma gets its off-diagonals, the mean stays
    o.init_from_state(x, P, *state_handles(uwv, lever, rotvec))
    o.update("velocity", zv, STATE_DVL_COV)
    o.update("acceleration", za, STATE_ACC_COV)
    return o.get_state()


def state_handles(uwv=None, lever=LEVER, rotvec=MOUNT_ROTVEC):
    """(loc, uwv, param) for init_from_state"""
    return location(), uwv or general_uwv(), general_param(None, lever, rotvec)


def start_state(f, batch, dof, first=0, **alter):
    """init_from_state on tilted_state, the process noise, the scene's rate: a
    batch object (engine or oracle wrapper) ready for predict -> efforts call"""
    x, P = tilted_state(batch, dof, first, **alter)
    alter.pop("level", None)
    f.init_from_state(x, P, *state_handles(**alter))
    f.set_process_noise_from_config(model_config(), DT, mounting(rotvec=alter.get("rotvec", MOUNT_ROTVEC))[1])
    f.set_rotation_rate(rates(batch, first))
    return f


def _expected_efforts(model, i):
    """the general model's efforts at instance i's truth (numpy_twin's UWV), for
    measurements near the filter's expectation"""
    q = attitude(i)
    v, a, wv, w = kinematics(i)
    Rt = _rotm(q).T
    vb = Rt @ (v - np.array([wv[0], wv[1], 0.0])) - np.cross(w, LEVER)
    ab = Rt @ a - np.cross(w, np.cross(w, LEVER))
    return model.efforts(np.concatenate([ab, np.zeros(3)]), np.concatenate([vb, w]), q)


def efforts_calls(batch, first=0):
    """see _efforts_calls; computed once per (batch, first): do not write into the arrays"""
    return _efforts_calls(batch, first)


@functools.lru_cache(maxsize=None)
def _efforts_calls(batch, first):
    """{name: (measurement [B, 6], R, only_vel)} for "full" and "vel", each meant
    for the state right after ONE predict from start_state (body rate
    rates()), and "sequence": [full, vel] with one predict between them (the
    second reads the blocks the first left in the shared model).  Measurements:
    the model's efforts at the instance's truth plus a seeded offset of twice
    the measurement's standard deviation."""
    import numpy_twin as T
    sd = np.sqrt(np.diag(EFFORTS_COV))
    model = T.UWV.from_abi(general_uwv())
    exp = np.stack([_expected_efforts(model, first + i) for i in range(batch)])
    z = {k: exp + 2.0 * sd * np.stack([_rng(first + i, 2 + n).standard_normal(6) for i in range(batch)])
         for n, k in enumerate(("full", "vel", "seq_full", "seq_vel"))}
    return dict(full=(z["full"], EFFORTS_COV, 0), vel=(z["vel"], EFFORTS_COV, 1),
                sequence=[(z["seq_full"], EFFORTS_COV, 0), (z["seq_vel"], EFFORTS_COV, 1)])


# ---- the log ---------------------------------------------------------------------
def model_log(batch, epochs=LOG_EPOCHS, dof=53, first=0, level=False):
    """synth.make_pose_log(.., "C4", ..) over `epochs` with the ADCP epoch pulled
    in (ADCP_EVERY), the scene's body rate added to the gyro, attitude(i) as
    rot0 and the scene's own efforts events: EFFORTS_EPOCHS, alternating full /
    velocity-only from full, measurements the default model's efforts at the
    truth (as make_pose_log's) plus a seeded offset of the configured standard
    deviations.  Start it with start_log()."""
    log = synth.make_pose_log(batch, epochs, "C4", dof=dof, first_instance=first, adcp_every=ADCP_EVERY)
    assert not (log["flags"] & abi.EV_EFFORTS).any()  # the drop-outs start at 30 s
    at = np.array([e for e in EFFORTS_EPOCHS if e < epochs])
    log["flags"] = log["flags"].copy()
    log["flags"][at] |= abi.EV_EFFORTS
    log["flags"][at[1::2]] |= abi.EV_EFFORTS_VELOCITY_ONLY
    index = np.full(epochs, -1, np.int32)
    index[at] = np.arange(len(at))[::-1]  # the rows stored in reverse event order: the index is not the identity
    log["efforts_index"] = index
    tr = log["truth"]
    k = at + 1
    M, Dl, Dq = synth.uwv_arrays(synth.default_uwv())
    wv3 = np.array([tr.wv[0], tr.wv[1], 0.0])
    vel6 = np.concatenate([synth._rotz_T(tr.psi[k], tr.v_nav[k] - wv3), np.zeros((len(k), 2)), tr.r[k][:, None]], -1)
    acc6 = np.concatenate([synth._rotz_T(tr.psi[k], tr.a_nav[k]), np.zeros((len(k), 3))], -1)
    tau = synth.calc_efforts_np(M, Dl, Dq, acc6, vel6)
    std = np.sqrt(np.diag(log["efforts_cov"]))
    noise = np.stack([_rng(first + i, 10).standard_normal((len(k), 6)) for i in range(batch)], 1)  # [n][B][6]
    rows = tau[:, None, :] + std * noise
    log["efforts"] = np.ascontiguousarray(rows[::-1])
    log["gyro"] = log["gyro"] + RATE
    # an early DVL epoch (the 5 Hz schedule first fires at epoch 199): the velocity prior of 1 m/s is
    # narrowed before the first velocity-only efforts update, which alone would cut its variance 1e4-fold
    if EARLY_DVL_EPOCH < epochs:
        assert not log["flags"][EARLY_DVL_EPOCH] & abi.EV_DVL and log["dvl_index"].max() == len(log["dvl"]) - 1
        log["flags"][EARLY_DVL_EPOCH] |= abi.EV_DVL
        log["dvl_index"] = log["dvl_index"].copy()
        log["dvl_index"][EARLY_DVL_EPOCH] = len(log["dvl"])  # the early sample is the LAST row
        inst = first + np.arange(batch)
        early = tr.dvl[EARLY_DVL_EPOCH + 1] + 0.01 * np.stack([(inst % 3) - 1.0, (inst % 2) - 0.5,
                                                               (inst % 5) - 2.0], 1)
        log["dvl"] = np.ascontiguousarray(np.concatenate([log["dvl"], early[None]], 0))
    log["rot0"] = rot0(batch, first, level)
    return log


def start_log(f, log, uwv=None, lever=LEVER, rotvec=MOUNT_ROTVEC):
    """init_from_config with the model, model_config() and the mounting, and the process noise"""
    ib, q = mounting(lever, rotvec)
    cfg = model_config()
    f.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv or general_uwv(),
                       imu_in_body=ib)
    f.set_process_noise_from_config(cfg, log["dt"], q)
    return f


def twin_from_log(log, i, dof, uwv=None, lever=LEVER, rotvec=MOUNT_ROTVEC):
    """instance i of the log as a numpy_twin.PoseTwin, started like start_log()"""
    import numpy_twin as T
    ib, q = mounting(lever, rotvec)
    cfg = T.cfg_dict(model_config())
    t = T.PoseTwin.from_config(dof, log["pos0"][i], log["pos_cov"][i], log["rot0"][i], log["rot_cov"][i], cfg,
                               T.UWV.from_abi(uwv or general_uwv()), imu_in_body=ib)
    t.set_noise_from_config(cfg, log["dt"], q_imu_in_body=q)
    return t


def twin_from_state(x, P, i, dof, uwv=None, lever=LEVER, rotvec=MOUNT_ROTVEC):
    """instance i of (x, P) as a numpy_twin.PoseTwin, started like start_state()"""
    import numpy_twin as T
    cfg = model_config()
    p = general_param(cfg, lever, rotvec)
    param = dict(imu_in_body=np.array(p.imu_in_body[:]), gyro_bias_offset=np.array(p.gyro_bias_offset[:]),
                 gyro_bias_tau=p.gyro_bias_tau, acc_bias_offset=np.array(p.acc_bias_offset[:]),
                 acc_bias_tau=p.acc_bias_tau, inertia_tau=p.inertia_tau, lin_damping_tau=p.lin_damping_tau,
                 quad_damping_tau=p.quad_damping_tau, water_velocity_tau=p.water_velocity_tau,
                 water_velocity_scale=p.water_velocity_scale, adcp_bias_tau=p.adcp_bias_tau,
                 atmospheric_pressure=p.atmospheric_pressure, water_density_tau=p.water_density_tau)
    t = T.PoseTwin(dof, x[i], P[i], (cfg.location.latitude, cfg.location.longitude),
                   T.UWV.from_abi(uwv or general_uwv()), param)
    t.set_noise_from_config(T.cfg_dict(cfg), DT, q_imu_in_body=mounting(lever, rotvec)[1])
    return t
