"""Seeded VelocityUKF scenes shared by tests/test_vel_scenes.py (CPU: oracle
against the numpy twin, and the conditions each scene is built for) and
tests/test_gpu_vel_edges.py (the HIP kernels against the oracle).  Every
builder returns the dict layout of synth.make_vel_log, so upload_log and
OracleVelBatch.run_log take it, plus two keys of its own: "Q" (the 4x4 process
noise, None = the filter's default) and "model" (the name of its motion model,
see uwv()).  Plain numpy; instance i's columns depend on (seed, i) alone, so
the same instance can be generated in a batch of any size."""
import numpy as np

from uwvk import abi, synth


def offaxis_uwv():
    """Coupled inertia / damping, W != B and general centres: every restoring
    force term is live (the model of test_velocity_ukf_model_change_between_runs)."""
    u = synth.default_uwv()
    M, Dl, Dq = synth.uwv_arrays(u)
    C = np.zeros((6, 6))
    C[0, 4] = C[4, 0] = 8.0
    C[1, 3] = C[3, 1] = -6.0
    C[2, 5] = C[5, 2] = 3.0
    abi.fill(u.inertia_matrix, (M * 1.3 + C).ravel())
    abi.fill(u.damping_matrices[0], (Dl * 0.7 + 0.5 * C).ravel())
    abi.fill(u.damping_matrices[1], (Dq * 1.5 + 0.25 * np.abs(C)).ravel())
    u.weight, u.buoyancy = 2100.0, 1950.0
    abi.fill(u.distance_body2centerofgravity, [0.02, -0.01, 0.03])
    abi.fill(u.distance_body2centerofbuoyancy, [0.01, 0.015, 0.06])
    return u


def uwv(log):
    return offaxis_uwv() if log.get("model") == "offaxis" else synth.default_uwv()


def _rng(seed, i, stream):
    return np.random.default_rng([seed, int(i), stream])


def _per_instance(seed, first, batch, stream, shape, scale=1.0):
    """[batch, *shape] normals, row i drawn from (seed, first + i, stream) alone"""
    return scale * np.stack([_rng(seed, first + i, stream).standard_normal(shape) for i in range(batch)])


def _assemble(batch, epochs, dt, dvl_at, p_at, seed, first, gyro_mean, gyro_sd, eff_sd, x0, P0, dvl_cov, p_cov, Q,
              model, shuffle):
    """Inputs and samples around x0: gyro / efforts [E][B][.], one DVL and one
    pressure row per event.  shuffle: the sample rows are stored in reverse
    event order behind an unused first row, so *_index is not the identity."""
    flags = np.zeros(epochs, np.uint32)
    flags[dvl_at] |= abi.EV_DVL
    flags[p_at] |= abi.EV_PRESSURE
    gyro = np.asarray(gyro_mean, float) + _per_instance(seed, first, batch, 0, (epochs, 3), gyro_sd)
    efforts = _per_instance(seed, first, batch, 1, (epochs, 6), eff_sd)

    def samples(at, stream, centre, sd, width):
        n = len(at)
        z = centre[:, None, :] + _per_instance(seed, first, batch, stream, (n, width), sd)  # [B][n][w], event order
        index = np.full(epochs, -1, np.int32)
        if shuffle:
            rows = np.concatenate([np.full((batch, 1, width), 99.0), z[:, ::-1]], 1)
            index[at] = n - np.arange(n)
        else:
            rows = z
            index[at] = np.arange(n)
        return index, np.ascontiguousarray(rows.transpose(1, 0, 2))

    dvl_index, dvl = samples(dvl_at, 2, x0[:, :3], 0.05, 3)
    p_index, pressure = samples(p_at, 3, x0[:, 3:], 0.05, 1)
    return dict(batch=batch, epochs=epochs, dt=dt, flags=flags,
                gyro=np.ascontiguousarray(gyro.transpose(1, 0, 2)),
                efforts=np.ascontiguousarray(efforts.transpose(1, 0, 2)),
                dvl_index=dvl_index, dvl=dvl, dvl_cov=np.array(dvl_cov, float),
                pressure_index=p_index, pressure=np.ascontiguousarray(pressure[:, :, 0]), pressure_cov=float(p_cov),
                x0=x0, P0=P0, Q=Q, model=model)


def _x0(seed, first, batch, speed):
    n = _per_instance(seed, first, batch, 4, (4,))
    return np.concatenate([np.array([speed, 0.2, -0.1]) + 0.1 * n[:, :3], -10.0 + 0.1 * n[:, 3:]], 1)


def _spd(seed, first, batch, stream, scale, floor):
    A = _per_instance(seed, first, batch, stream, (4, 4), scale)
    return A @ np.swapaxes(A, 1, 2) + floor * np.eye(4)


def dense_events(batch, epochs=12, seed=41, first=0):
    """DVL at every 3rd epoch (e % 3 == 2), pressure at every 2nd (e % 2 == 0),
    both at every 6th; with the default 12 epochs the first epoch has a
    pressure sample, the last a DVL sample and epochs 1, 3, 7, 9 have none.
    The sample rows are shuffled (see _assemble).  Default model and Q."""
    e = np.arange(epochs)
    x0 = _x0(seed, first, batch, 1.0)
    P0 = np.broadcast_to(np.diag([0.01, 0.01, 0.01, 0.01]), (batch, 4, 4)).copy()
    return _assemble(batch, epochs, 0.02, e[e % 3 == 2], e[e % 2 == 0], seed, first, [0.0, 0.0, 0.3], 0.02, 5.0,
                     x0, P0, np.eye(3) * 1e-3, 1e-3, None, "default", True)


TILTED_DVL_COV = np.array([[4.0e-3, 1.2e-3, -0.8e-3], [1.2e-3, 3.0e-3, 0.9e-3], [-0.8e-3, 0.9e-3, 5.0e-3]])


def tilted_q():
    A = np.array([[2e-2, 1e-3, -3e-3, 2e-3], [4e-3, 1e-2, 2e-3, -1e-3], [-2e-3, 3e-3, 1e-2, 4e-3],
                  [1e-3, -2e-3, 3e-3, 5e-3]])
    return A @ A.T


def tilted(batch, epochs=60, seed=43, first=0):
    """Roll, pitch and yaw rates of the same order (0.6, -0.5, 0.7 rad/s) at
    dt = 0.02: the model quaternion leaves every axis within 50 epochs.  Off-axis
    model, a full SPD P0 that differs per instance, full dvl_cov and Q.  DVL at
    every 5th epoch, pressure at every 4th."""
    e = np.arange(epochs)
    x0 = _x0(seed, first, batch, 1.0)
    P0 = _spd(seed, first, batch, 5, 0.06, 1e-3)
    return _assemble(batch, epochs, 0.02, e[e % 5 == 4], e[e % 4 == 1], seed, first, [0.6, -0.5, 0.7], 0.05, 5.0,
                     x0, P0, TILTED_DVL_COV, 2e-3, tilted_q(), "offaxis", False)


SPREAD_SIGMA = np.array([1e-3, 1e-2, 1e-1, 1.0])  # velocity sigma (m/s) of instance i: SPREAD_SIGMA[i % 4]


def mixed_spread(batch, epochs=20, seed=47, first=0):
    """Within every 4 consecutive instances (one wave of the 16-lane-row
    kernel) the velocity sigma runs from 1e-3 to 1 m/s at 1.5 m/s: the
    quadratic damping bends the sigma points of the wide instances, whose
    iterative mean takes a second pass, and not those of the narrow ones.
    DVL at every 7th epoch (the spread survives until then), pressure at every 5th."""
    e = np.arange(epochs)
    x0 = _x0(seed, first, batch, 1.5)
    sg = SPREAD_SIGMA[(first + np.arange(batch)) % 4]
    A = _per_instance(seed, first, batch, 5, (4, 4), 0.2) + np.eye(4)
    P0 = A @ np.swapaxes(A, 1, 2)
    d = np.sqrt(np.diagonal(P0, axis1=1, axis2=2))
    s = np.concatenate([np.repeat(sg[:, None], 3, 1), np.full((batch, 1), 0.1)], 1) / d
    P0 = P0 * s[:, :, None] * s[:, None, :]
    return _assemble(batch, epochs, 0.02, e[e % 7 == 6], e[e % 5 == 4], seed, first, [0.1, -0.1, 0.3], 0.02, 5.0,
                     x0, P0, np.eye(3) * 1e-3, 1e-3, None, "default", False)


SCENES = dict(dense=dense_events, tilted=tilted, mixed=mixed_spread)


def take(log, idx):
    """the log of the instances `idx` alone (their own columns of every array)"""
    idx = np.atleast_1d(idx)
    out = dict(log)
    out["batch"] = len(idx)
    for k in ("gyro", "efforts", "dvl"):
        out[k] = np.ascontiguousarray(log[k][:, idx])
    out["pressure"] = np.ascontiguousarray(log["pressure"][:, idx])
    out["x0"], out["P0"] = log["x0"][idx].copy(), log["P0"][idx].copy()
    return out


def add_events(log, epochs):
    """a copy of `log` with a DVL and a pressure event at each of `epochs`
    (samples: the log's last rows, shifted a little), on top of what it has"""
    out = dict(log)
    for k in ("flags", "dvl_index", "pressure_index", "dvl", "pressure"):
        out[k] = log[k].copy()
    for n, e in enumerate(epochs):
        for flag, index, rows in ((abi.EV_DVL, "dvl_index", "dvl"), (abi.EV_PRESSURE, "pressure_index", "pressure")):
            if not out["flags"][e] & flag:
                out["flags"][e] |= flag
                out[index][e] = len(out[rows])
                out[rows] = np.concatenate([out[rows], out[rows][-1:] + 0.003 * (n + 1)])
    return out


def start(f, log, P0=None):
    """init / model / noise / first gyro on a batch object (engine or oracle wrapper)"""
    f.init(log["x0"], log["P0"] if P0 is None else P0)
    if log.get("Q") is not None:
        f.set_process_noise(log["Q"])
    f.set_gyro(log["gyro"][0])
    f.setup_motion_model(uwv(log))
    return f
