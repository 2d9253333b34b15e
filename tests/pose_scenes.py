"""Seeded PoseUKF edge scenes shared by tests/test_pose_scenes.py (CPU: oracle
against the numpy twin, and the condition each scene is built for) and
tests/test_gpu_pose_edges.py (the HIP kernels against the oracle).

Wide-prior scenes: synth.make_pose_log(B, E, "C3") with the orientation prior
replaced per instance and one DVL epoch put inside the window, so that the
sigma points' orientation steps mu [+] +-L_j leave the Taylor branches of
so3_exp_psp (|v| < 0.25) and so3_log_psp (rotation < ~0.1 rad,
csrc/uwvk_psp_dev.hpp).  The acceleration update collapses roll and pitch
within three epochs, so the window is short and the DVL epoch early.

Indefinite-Sigma scenes: a healthy (x, P) with its off-diagonals, and P with
one pivot of its unpivoted LDL^T made negative or zero at a chosen index, the
27 parameter rows still exactly decoupled.

Plain numpy; instance i's columns depend on (seed, first + i) alone."""
import numpy as np

from uwvk import abi, synth

EPOCHS = 6
DVL_EPOCH = 1  # orientation still wide: yaw untouched, roll / pitch at ~0.22 of (0.3, 0.3)

# orientation prior standard deviations (roll, pitch, yaw), rad; None: make_pose_log's own
SCENE_SD = dict(wide=(0.3, 0.3, 0.5), straddle=(0.2, 0.3, 0.04), narrow=None, big_step=None, far_step=None)
BIG_GYRO = np.array([1.5, -2.0, 2.0])  # rad/s; |w dt| = 0.32 at BIG_DT: the process model's exp off its series
BIG_DT = 0.1
# so3_exp_psp's series is good far beyond its threshold (the first dropped term
# is u^6 / 13!, u = |v|^2 / 4: 1e-17 at 0.5 rad), so a wrong threshold shows
# only past ~2.3 rad, where that term reaches 1e-9: |w dt| = 2.56
FAR_GYRO = 8.0 * BIG_GYRO
STEP_GYRO = dict(big_step=BIG_GYRO, far_step=FAR_GYRO)

# the thresholds of so3_exp_psp / so3_log_psp as rotation angles
EXP_SERIES_BELOW = 0.25
LOG_SERIES_BELOW = 2.0 * np.arctan(0.05)  # n2 < 0.0025 w^2: 0.09992 rad


def dvl_epoch(scene):
    return 0 if scene in STEP_GYRO else DVL_EPOCH


def make(scene, batch, dof=53, first=0, epochs=None):
    """The log of `scene`: make_pose_log's dict (upload_log / OraclePoseBatch.run_log
    take it).  wide / straddle: rot_cov = diag(sd_i^2) with sd_i the scene's
    std-devs scaled by 1 + 0.02 ((first + i) % 3 - 1); the odd instances of
    wide start from -q0.  big_step: the narrow prior and ONE epoch of dt = 0.1
    with the gyro BIG_GYRO plus the log's own noise, its DVL sample in that
    epoch (further epochs of such steps against the 1 kHz log's measurements
    are ill-conditioned: oracle and twin part by 7e-11 in the second).
    far_step: the same with the gyro FAR_GYRO."""
    if epochs is None:
        epochs = 1 if scene in STEP_GYRO else EPOCHS
    at = dvl_epoch(scene)
    log = synth.make_pose_log(batch, epochs, "C3", dof=dof, first_instance=first)
    assert not (log["flags"] & abi.EV_DVL).any()  # the 5 Hz schedule first fires at epoch 199
    inst = first + np.arange(batch)
    log["flags"] = log["flags"].copy()
    log["flags"][at] |= abi.EV_DVL
    log["dvl_index"] = log["dvl_index"].copy()
    log["dvl_index"][at] = 0
    dvl = np.broadcast_to(log["truth"].dvl[at + 1], (1, batch, 3)).copy()
    dvl[0] += 0.01 * np.stack([(inst % 3) - 1.0, (inst % 2) - 0.5, (inst % 5) - 2.0], 1)
    log["dvl"] = dvl
    sd = SCENE_SD[scene]
    if sd is not None:
        s = np.asarray(sd)[None, :] * (1.0 + 0.02 * ((inst % 3) - 1.0))[:, None]
        log["rot_cov"] = np.zeros((batch, 3, 3))
        for k in range(3):
            log["rot_cov"][:, k, k] = s[:, k] ** 2
    if scene == "wide":
        log["rot0"] = np.where((inst % 2 == 1)[:, None], -log["rot0"], log["rot0"])
    if scene in STEP_GYRO:
        log["dt"] = BIG_DT
        log["gyro"] = log["gyro"] - log["truth"].gyro[1:epochs + 1][:, None, :] + STEP_GYRO[scene]
    log["scene"] = scene
    return log


PER_INSTANCE_EPOCH_MAJOR = ("gyro", "acc", "dvl")
PER_INSTANCE = ("pos0", "pos_cov", "rot0", "rot_cov")


def mix(parts):
    """The batch made of [(log, instance), ...] in that order; the logs share
    their flags, dt and shared covariances (scenes of one `epochs`, not big_step)."""
    base = parts[0][0]
    out = dict(base)
    out["batch"] = len(parts)
    for lg, _ in parts:
        assert lg["dt"] == base["dt"] and np.array_equal(lg["flags"], base["flags"])
    for k in PER_INSTANCE_EPOCH_MAJOR:
        out[k] = np.ascontiguousarray(np.stack([lg[k][:, i] for lg, i in parts], 1))
    for k in PER_INSTANCE:
        out[k] = np.ascontiguousarray(np.stack([lg[k][i] for lg, i in parts], 0))
    return out


def start(f, log):
    """init_from_config and the process noise on a batch object (engine or oracle wrapper)"""
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    f.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    f.set_process_noise_from_config(cfg, log["dt"])
    return f


def ori_column_norms(P):
    """|L[3:6, j]| of L = chol(P), j = 0 .. dof-1: the orientation step of sigma point pair j"""
    L = np.linalg.cholesky(P)
    return np.linalg.norm(L[3:6, :], axis=0)


def single_calls(log, x):
    """The single update calls of the wide-prior tests, [(name, kind, mu, cov,
    extra, only_vel)], each meant for the state right after the first predict
    (x: its mean, [B][store]); seeded, the same for every filter.  far_step
    leaves the two BodyEfforts forms out: at a body rate of 25 rad/s the
    model's rate terms make the update ill-conditioned (oracle and twin part by
    1.9e-10 sigma there, 1.5e-12 over the rest of the scene)."""
    B = len(x)
    rng = np.random.default_rng(23)
    n = lambda *s: rng.standard_normal(s)  # noqa: E731
    calls = [
        ("acceleration", "acceleration", log["acc"][0], log["acc_cov"], None, 0),
        ("velocity", "velocity", log["dvl"][0] + 0.01 * n(B, 3), np.eye(3) * 1e-4, None, 0),
        ("pressure", "pressure", (101325.0 - x[:, 2] * 9.81 * 1025 + 50 * n(B))[:, None], np.array([[1e4]]),
         np.array([0.1, -0.2, 0.3]), 0),
        ("water_velocity", "water_velocity", np.array([1.0, 0.0]) + 0.1 * n(B, 2), np.eye(2) * 0.05 ** 2,
         np.linspace(0.0, 1.0, B), 0),
        ("xy", "xy", x[:, 0:2] + n(B, 2), np.eye(2) * 0.5, None, 0),
        ("z", "z", x[:, 2:3] + 0.1 * n(B, 1), np.array([[0.01]]), None, 0),
        ("efforts_vel", "efforts", 20 * n(B, 6), np.diag([25.0, 25, 25, 1, 1, 1]), None, 1),
        ("efforts", "efforts", 20 * n(B, 6), np.diag([25.0, 25, 25, 1, 1, 1]), None, 0),
        ("geographic", "geographic", _lat_lon(x[:, 0] + 0.3 * n(B), x[:, 1] + 0.3 * n(B)), np.eye(2) * 4.0,
         np.array([0.5, 0.0, -0.2]), 0),
        ("delayed_xy", "delayed_xy", x[:, 0:2] + 0.2 * n(B, 2), np.eye(2) * 0.5, x[:, 0:2] - 0.3, 0),
    ]
    return [c for c in calls if not (log.get("scene") == "far_step" and c[1] == "efforts")]


def _lat_lon(north, east):
    from numpy_twin import nav_to_world
    lat, lon = nav_to_world((synth.LAT0, synth.LON0), north, east)
    return np.stack([lat, lon], 1)


def twin(log, i, dof):
    """instance i of the log as a numpy_twin.PoseTwin, started like start()"""
    import numpy_twin as T
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    t = T.PoseTwin.from_config(dof, log["pos0"][i], log["pos_cov"][i], log["rot0"][i], log["rot_cov"][i],
                               T.cfg_dict(cfg), T.UWV.from_abi(uwv))
    t.set_noise_from_config(T.cfg_dict(cfg), log["dt"])
    return t


# ---- indefinite Sigma -------------------------------------------------------
PIVOTS = {53: (0, 5, 14, 15, 18, 19, 52), 26: (0, 5, 14, 15, 18, 19, 25)}
EFF_PANEL_PIVOTS = (15, 16, 31, 32, 47, 48)  # the edges of eff_chol's 16-column panels (dof 53)
ZERO_PARAM_DOF = 30  # a linear-damping parameter (dof 53)
HEALTHY_EPOCHS = 3


def healthy_state(batch, dof=53, first=0):
    """(log, x, P): the narrow scene's instances on the oracle after three
    predict + acceleration epochs and the DVL update of DVL_EPOCH's sample: P
    with its off-diagonals, the parameter rows exactly decoupled."""
    import oracle_ctypes as O
    log = make("narrow", batch, dof, first)
    o = start(O.OraclePoseBatch(batch, dof), log)
    for e in range(HEALTHY_EPOCHS):
        o.set_rotation_rate(log["gyro"][e])
        o.predict(log["dt"])
        o.update("acceleration", log["acc"][e], log["acc_cov"])
    o.update("velocity", log["dvl"][0], log["dvl_cov"])
    x, P = o.get_state()
    return log, x, P


def negative_pivot(P, p):
    """L diag(D) L^T, symmetrised, with L = chol(P), D = 1 and D[p] = -1: the
    first non-positive pivot of its unpivoted LDL^T is pivot p, negative"""
    L = np.linalg.cholesky(P)
    D = np.ones(len(P))
    D[p] = -1.0
    Pb = (L * D) @ L.T
    return 0.5 * (Pb + Pb.T)


def zero_pivot(P, d):
    """P with row and column d zeroed (d = 0), or a decoupled parameter's
    variance zeroed: pivot d is exactly 0.0"""
    Pb = P.copy()
    Pb[d, :] = 0.0
    Pb[:, d] = 0.0
    return Pb


def indefinite_scenes(dof):
    """{name: (builder P -> P_bad, pivot index, sign)}, sign -1 or 0"""
    out = {"neg%d" % p: ((lambda P, p=p: negative_pivot(P, p)), p, -1) for p in PIVOTS[dof]}
    out["zero0"] = ((lambda P: zero_pivot(P, 0)), 0, 0)
    if dof == 53:
        out["zeroparam"] = ((lambda P: zero_pivot(P, ZERO_PARAM_DOF)), ZERO_PARAM_DOF, 0)
        for p in EFF_PANEL_PIVOTS:
            out.setdefault("neg%d" % p, ((lambda P, p=p: negative_pivot(P, p)), p, -1))
    return out


# the z update's variance, as a multiple of P[2, 2], of the run-time not-positive-definite case
Z_VARIANCE_FACTORS = (-0.5, -1.5)


def z_variance_breaks_sigma(factor):
    """S = (1 + factor) P[2, 2]; Sigma - C K^T has P[2, 2] (1 - 1 / (1 + factor)) at pivot 2: negative iff -1 < factor < 0"""
    return -1.0 < factor < 0.0


def param_block_decoupled(P):
    """the host's eligibility test of the PD / pair kernels: rows 19..45 zero off the diagonal"""
    blk = np.array(P[19:46, :])
    blk[np.arange(27), 19 + np.arange(27)] = 0.0
    return not blk.any()


def state_handles(dof):
    """(loc, uwv, param) for init_from_state"""
    cfg = synth.default_pose_config()
    loc = abi.Location(cfg.location.latitude, cfg.location.longitude, cfg.location.altitude)
    return loc, synth.default_uwv(), synth.pose_parameter(cfg)


# ---- the PSP steps on an indefinite Sigma, restated on the CPU -----------------
# A PSP step factors the leading k tangent DOFs and carries the others linearly
# (DESIGN.md 4.3), which is exact because the step's model is affine in them.
# With Sigma = L diag(d) L^T that equals a UKF whose point pair j sits at
# mu [+] +-sqrt|d_j| L_j and counts with the weight sign(d_j): an affine
# direction then contributes d_j (J L_j)(J L_j)^T whatever d_j's sign, and drops
# out of the means.  One term is not signed: the kernel counts the 2 (n - k)
# linearly carried points, each at the centre's image c plus or minus its
# linear part, once each in the spread about the mean, wc = 1 + 2 (n - k) times
# (c - mean)(c - mean)^T (psp_update, psp_predict), whatever their pivots'
# signs: _centre_terms (and the same term of the iterated means) puts those back.  While the first non-positive pivot lies
# at or beyond the step's k this is the value the kernel's formulas define.
def ldl(P):
    """unit lower L and pivots d of the unpivoted LDL^T (a zero pivot needs a zero column below it)"""
    A = np.array(P, float)
    n = len(A)
    L, d = np.eye(n), np.zeros(n)
    for k in range(n):
        d[k] = A[k, k]
        if d[k] != 0.0:
            L[k + 1:, k] = A[k + 1:, k] / d[k]
            A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k]) * d[k]
        else:
            assert not A[k + 1:, k].any()
    return L, d


def _signed_points(lay, mu, P):
    L, d = ldl(P)
    n = lay.dof
    D = np.zeros((2 * n + 1, n))
    D[1::2] = (L * np.sqrt(np.abs(d))).T
    D[2::2] = -D[1::2]
    w = np.ones(2 * n + 1)
    w[1::2] = w[2::2] = np.sign(d)
    return lay.boxplus(np.broadcast_to(mu, (2 * n + 1,) + mu.shape), D), w


def _signed_mean(minus, plus, X, w):
    ref = X[0].copy()
    for _ in range(100):
        dev = minus(X, ref)
        d = ((w[:, None] * dev).sum(axis=0) + 2.0 * (1.0 - w[1::2]).sum() * dev[0]) / len(X)  # (as _centre_terms)
        ref = plus(ref, d)
        if np.linalg.norm(d) <= 1e-6:
            return ref
    raise AssertionError("the signed mean did not converge")


def _centre_terms(w, c):
    """sum over the point pairs of (1 - w_j) c c^T: with 0.5 (D^T w D) the
    pair's share of the centre term becomes c c^T whatever its weight"""
    return (1.0 - w[1::2]).sum() * np.outer(c, c)


def signed_ukf_predict(lay, mu, P, g, Qp):
    X, w = _signed_points(lay, mu, P)
    X = g(X)
    m = _signed_mean(lay.boxminus, lay.boxplus, X, w)
    D = lay.boxminus(X, m)
    return m, 0.5 * (D.T * w) @ D + _centre_terms(w, D[0]) + Qp


def signed_ukf_update(lay, mu, P, z, h, R, zmanifold, gate):
    """numpy_twin.ukf_update for vector measurements without a gate"""
    assert zmanifold in (True, False) and not gate
    X, w = _signed_points(lay, mu, P)
    Z = h(X)
    zm = _signed_mean(lambda a, b: a - b, lambda a, b: a + b, Z, w)
    dZ, dX = Z - zm, lay.boxminus(X, mu)
    S = 0.5 * (dZ.T * w) @ dZ + _centre_terms(w, dZ[0]) + R
    Cm = 0.5 * (dX.T * w) @ dZ
    K = Cm @ np.linalg.inv(S)
    P = P - Cm @ K.T
    delta = K @ (z - zm)
    X, w = _signed_points(lay, mu, P)
    mu = lay.boxplus(mu, delta)
    X = lay.boxplus(X, np.broadcast_to(delta, (X.shape[0], delta.shape[0])))
    D = lay.boxminus(X, mu)
    return mu, 0.5 * (D.T * w) @ D, True


class signed_twin:
    """Context manager: numpy_twin's PoseTwin steps run the signed-weight UKF."""

    def __enter__(self):
        import numpy_twin as T
        self.T, self.prev = T, (T.ukf_predict, T.ukf_update)
        T.ukf_predict, T.ukf_update = signed_ukf_predict, signed_ukf_update
        return self

    def __exit__(self, *exc):
        self.T.ukf_predict, self.T.ukf_update = self.prev
        return False


def first_bad_pivot(P):
    """index of the first non-positive pivot of P's unpivoted LDL^T, len(P) if there is none"""
    from helpers import pivots
    d = pivots(P)
    return len(d) - 1 if not d[-1] > 0 else len(P)


def signed_window(log, x, P, i, dof, look=None):
    """Instance i from (x, P) through epochs 0 .. NOTPD_WINDOW-1 of its log on
    the twin with the signed-weight UKF -> (mu, P); look(step, P) before every step."""
    t = twin(log, i, dof)
    t.mu, t.P = np.array(x, float), np.array(P, float)
    look = look or (lambda step, P: None)
    with signed_twin():
        for e in range(NOTPD_WINDOW):
            look("predict", t.P)
            t.w = log["gyro"][e][i]
            t.predict(log["dt"])
            look("acceleration", t.P)
            t.update("acceleration", log["acc"][e][i], log["acc_cov"])
            if log["flags"][e] & abi.EV_DVL:
                look("velocity", t.P)
                t.update("velocity", log["dvl"][log["dvl_index"][e]][i], log["dvl_cov"])
    return t.mu, t.P


PSP_K = dict(predict=15, acceleration=6, velocity=6, water_velocity=6, pressure=19, efforts_vel=9,
             xy=0, z=0, geographic=0, delayed_xy=0)  # the leading tangent DOFs each PSP step factors
NOTPD_WINDOW = 4  # epochs 0..3 of the healthy state's own log: four predicts and accelerations, the DVL epoch
