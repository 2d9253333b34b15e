"""numpy twin of the CPU oracle — an independent restatement for cross-checking.

TEST INFRASTRUCTURE ONLY (tests/ import it; the product never does).
PARITY STATUS: unpinned against the reference binary.  The
reference's UKF arithmetic lives in ukfom/MTK (absent here).  This twin is
written from the frozen spec in vectorised numpy form — LAPACK
Cholesky, matrix products over all sigma points at once — so that it shares no
code path with oracle/uwvk_oracle.c.  Agreement of the two restatements is the
strongest available guard against a restatement bug.

Sources restated: PoseUKF.cpp:12-84 (process), :107-219 (measurements),
:288-372 (init), :393-465 (noise / predict), :476-611 (update wiring, gates),
:685-699; VelocityUKF.cpp:6-130; PoseState.hpp:29-45.

Second part (the small filters, checked against oracle/uwvk_small_oracle.c):
BottomUKF.cpp:5-67, IndirectPoseUKF.cpp:7-142, PoseUKF.cpp:221-244 and
:613-654, DESIGN.md §3 items 1-4 and 11.  Written from those sources, not from
the C file, and in a different form on purpose: S2 through the rotation matrix
R_x = I + [v]x + [v]x^2 / (1 + x_z), v = e3 x x (the C and HIP code use two
basis vectors), the visual model through composed rotation matrices (they use
step-wise quaternion sandwiches).
"""
import numpy as np

EARTHW = 7.292115e-5
A_WGS, F_WGS = 6378137.0, 1.0 / 298.257223563
D2P95 = 5.991
IDX = [0, 1, 5]


# ---------------------------------------------------------------- SO3 / quats
def qmul(a, b):
    a, b = np.asarray(a), np.asarray(b)
    w1, v1 = a[..., :1], a[..., 1:]
    w2, v2 = b[..., :1], b[..., 1:]
    w = w1 * w2 - np.sum(v1 * v2, -1, keepdims=True)
    v = w1 * v2 + w2 * v1 + np.cross(v1, v2)
    return np.concatenate([w, v], -1)


def qconj(q):
    return np.concatenate([q[..., :1], -q[..., 1:]], -1)


def qrot(q, v):
    """Rotate v by unit quaternion q (Eigen _transformVector form)."""
    u = q[..., 1:]
    uv = 2.0 * np.cross(u, v)
    return v + q[..., :1] * uv + np.cross(u, uv)


def qmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def so3_exp(v):
    v = np.asarray(v, dtype=float)
    th = np.linalg.norm(v, axis=-1, keepdims=True)
    safe = np.where(th > 0, th, 1.0)
    s = np.where(th > 0, np.sin(0.5 * th) / safe, 0.0)
    c = np.where(th > 0, np.cos(0.5 * th), 1.0)
    return np.concatenate([c, s * v], -1)


def so3_log(q):
    q = np.where(q[..., :1] < 0, -q, q)
    nv = np.linalg.norm(q[..., 1:], axis=-1, keepdims=True)
    safe = np.where(nv > 0, nv, 1.0)
    k = np.where(nv > 0, 2.0 * np.arctan2(nv, q[..., :1]) / safe, 0.0)
    return k * q[..., 1:]


# ---------------------------------------------------------------- layout
# SO3 [+] side, process-wide like the C oracle's switch:
# True = body frame q exp(d) (default since r05, MTK's SO3::boxplus), False =
# nav frame exp(d) q.  Set it before constructing a twin.
SO3_RIGHT = True


def so3_plus(q, d, right):
    """q [+] d for an already scaled rotation vector d."""
    return qmul(q, so3_exp(d)) if right else qmul(so3_exp(d), q)


def so3_minus(a, b, right):
    """a [-] b: log(b^-1 a) (right) or log(a b^-1) (left)."""
    return so3_log(qmul(qconj(b), a)) if right else so3_log(qmul(a, qconj(b)))


class Layout:
    def __init__(self, dof, right=None):
        self.dof = dof
        self.right = SO3_RIGHT if right is None else right
        self.full = dof == 53
        self.store = dof + 1
        # tangent -> storage for vect DOFs
        self.vec_d = np.array([d for d in range(dof) if not 3 <= d < 6])
        self.vec_s = np.where(self.vec_d < 3, self.vec_d, self.vec_d + 1)
        o = 20 if not self.full else 47
        self.s = dict(pos=0, quat=3, vel=7, acc=10, bg=13, ba=16, grav=19, wv=o, wvb=o + 2, badcp=o + 4,
                      rho=o + 6)
        if self.full:
            self.s.update(inertia=20, lin=29, quad=38)
        od = 19 if not self.full else 46
        self.d = dict(pos=0, ori=3, vel=6, acc=9, bg=12, ba=15, grav=18, wv=od, wvb=od + 2, badcp=od + 4,
                      rho=od + 6)
        if self.full:
            self.d.update(inertia=19, lin=28, quad=37)

    def boxplus(self, X, D):
        """X [..., store] (+) D [..., dof]: vect + D; SO3 q exp(D) (right) or exp(D) q (left)."""
        Y = np.array(X, dtype=float, copy=True)
        Y[..., self.vec_s] = X[..., self.vec_s] + D[..., self.vec_d]
        Y[..., 3:7] = so3_plus(X[..., 3:7], D[..., 3:6], self.right)
        return Y

    def boxminus(self, X, M):
        D = np.zeros(X.shape[:-1] + (self.dof,))
        D[..., self.vec_d] = X[..., self.vec_s] - M[..., self.vec_s]
        D[..., 3:6] = so3_minus(X[..., 3:7], M[..., 3:7], self.right)
        return D


class VecLayout:
    def __init__(self, n):
        self.dof = n

    def boxplus(self, X, D):
        return X + D

    def boxminus(self, X, M):
        return X - M


# ---------------------------------------------------------------- S2
def skew(v):
    z = np.zeros_like(v[..., 0])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def s2_rot(x):
    """R_x, the minimal rotation taking e3 to x: I + [v]x + [v]x^2 / (1 + x_z), v = e3 x x."""
    x = np.asarray(x, dtype=float)
    K = skew(np.cross(np.array([0.0, 0.0, 1.0]), x))
    return np.eye(3) + K + K @ K / (1.0 + x[..., 2])[..., None, None]


def s2_from(v):
    """MTK::S2(v): the normalised vector."""
    v = np.asarray(v, dtype=float)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def s2_plus(x, d):
    """x [+] d = R_x (sinc|d| d, cos|d|)."""
    d = np.asarray(d, dtype=float)
    t = np.linalg.norm(d, axis=-1, keepdims=True)
    sc = np.where(t > 0, np.sin(t) / np.where(t > 0, t, 1.0), 1.0)
    e = np.concatenate([sc * d, np.cos(t)], -1)
    return (s2_rot(x) @ e[..., None])[..., 0]


def s2_minus(y, x):
    """y [-] x = log(R_x^T y), log(w) = atan2(|w12|, w3) w12 / |w12|."""
    w = (np.swapaxes(s2_rot(x), -1, -2) @ np.asarray(y, dtype=float)[..., None])[..., 0]
    nn = np.linalg.norm(w[..., :2], axis=-1, keepdims=True)
    k = np.where(nn > 0, np.arctan2(nn, w[..., 2:]) / np.where(nn > 0, nn, 1.0), 0.0)
    return k * w[..., :2]


class S2Layout:
    """A single S2 value (the measurement manifold of the normal and bearing updates)."""
    dof = 2

    def boxplus(self, X, D):
        return s2_plus(X, D)

    def boxminus(self, X, M):
        return s2_minus(X, M)


class Compound:
    """Compound manifold over segments ("v", dim) | ("so3",) | ("s2",), stored in
    order: vect dim, quaternion (w, x, y, z), unit 3-vector.  `right` is the side
    of every SO3 segment (MTK has one SO3::boxplus)."""

    def __init__(self, segs, right=None):
        self.right = SO3_RIGHT if right is None else right
        self.segs = []
        di = si = 0
        for seg in segs:
            kind = seg[0]
            dd, ss = (seg[1], seg[1]) if kind == "v" else ((3, 4) if kind == "so3" else (2, 3))
            self.segs.append((kind, slice(di, di + dd), slice(si, si + ss)))
            di, si = di + dd, si + ss
        self.dof, self.store = di, si

    def boxplus(self, X, D):
        X, D = np.asarray(X, dtype=float), np.asarray(D, dtype=float)
        Y = np.empty(np.broadcast_shapes(X.shape[:-1], D.shape[:-1]) + (self.store,))
        for kind, d, s in self.segs:
            if kind == "v":
                Y[..., s] = X[..., s] + D[..., d]
            elif kind == "so3":
                Y[..., s] = so3_plus(X[..., s], D[..., d], self.right)
            else:
                Y[..., s] = s2_plus(X[..., s], D[..., d])
        return Y

    def boxminus(self, X, M):
        X, M = np.asarray(X, dtype=float), np.asarray(M, dtype=float)
        D = np.empty(np.broadcast_shapes(X.shape[:-1], M.shape[:-1]) + (self.dof,))
        for kind, d, s in self.segs:
            if kind == "v":
                D[..., d] = X[..., s] - M[..., s]
            elif kind == "so3":
                D[..., d] = so3_minus(X[..., s], M[..., s], self.right)
            else:
                D[..., d] = s2_minus(X[..., s], M[..., s])
        return D


# ---------------------------------------------------------------- UKF core
def sigma_points(lay, mu, P):
    L = np.linalg.cholesky(P)
    n = lay.dof
    D = np.zeros((2 * n + 1, n))
    D[1::2] = L.T
    D[2::2] = -L.T
    return lay.boxplus(np.broadcast_to(mu, (2 * n + 1,) + mu.shape), D)


def manifold_mean(lay, X):
    ref = X[0].copy()
    for _ in range(10000):
        d = lay.boxminus(X, ref).mean(axis=0)
        ref = lay.boxplus(ref, d)
        if np.linalg.norm(d) <= 1e-6:
            break
    return ref


def vect_mean(Z):
    ref = Z[0].copy()
    for _ in range(10000):
        d = (Z - ref).mean(axis=0)
        ref = ref + d
        if np.linalg.norm(d) <= 1e-6:
            break
    return ref


def ukf_predict(lay, mu, P, g, Qp):
    X = sigma_points(lay, mu, P)
    X = g(X)
    m = manifold_mean(lay, X)
    D = lay.boxminus(X, m)
    return m, 0.5 * D.T @ D + Qp


def ukf_update(lay, mu, P, z, h, R, zmanifold, gate):
    """zmanifold: False (Eigen vector: plain average), True (vect manifold:
    iterative mean) or a layout with boxplus / boxminus (a manifold-valued
    measurement: iterative mean, deviations and innovation by [-])."""
    X = sigma_points(lay, mu, P)
    Z = h(X)
    if zmanifold is True or zmanifold is False:
        zm = vect_mean(Z) if zmanifold else Z.mean(axis=0)
        dZ = Z - zm
        nu = z - zm
    else:
        zm = manifold_mean(zmanifold, Z)
        dZ = zmanifold.boxminus(Z, zm)
        nu = zmanifold.boxminus(z, zm)
    dX = lay.boxminus(X, mu)
    S = 0.5 * dZ.T @ dZ + R
    C = 0.5 * dX.T @ dZ
    Si = np.linalg.inv(S)
    K = C @ Si
    d2 = nu @ Si @ nu
    if gate and d2 > D2P95:
        return mu, P, False
    P = P - C @ K.T
    delta = K @ nu
    # apply_delta: re-spread, shift by delta, covariance about mu [+] delta
    X = sigma_points(lay, mu, P)
    mu = lay.boxplus(mu, delta)
    X = lay.boxplus(X, np.broadcast_to(delta, (X.shape[0], delta.shape[0])))
    D = lay.boxminus(X, mu)
    return mu, 0.5 * D.T @ D, True


# ---------------------------------------------------------------- geography
def radii(lat0):
    e2 = F_WGS * (2 - F_WGS)
    den = 1 - e2 * np.sin(lat0) ** 2
    return A_WGS * (1 - e2) / den ** 1.5, A_WGS / np.sqrt(den)


def nav_to_world(loc, x, y):
    rm, rn = radii(loc[0])
    return loc[0] + x / rm, loc[1] - y / (rn * np.cos(loc[0]))


def world_to_nav(loc, lat, lon):
    rm, rn = radii(loc[0])
    return (lat - loc[0]) * rm, -(lon - loc[1]) * rn * np.cos(loc[0])


def wgs84_gravity(lat, alt):
    s2 = np.sin(lat) ** 2
    return 9.7803253359 * (1 + 0.00193185265241 * s2) / np.sqrt(1 - 0.00669437999013 * s2) - 3.086e-6 * alt


# ---------------------------------------------------------------- dynamics
class UWV:
    def __init__(self, M, Dl, Dq, weight=0.0, buoyancy=0.0, cog=(0, 0, 0), cob=(0, 0, 0)):
        self.M, self.Dl, self.Dq = np.array(M, float), np.array(Dl, float), np.array(Dq, float)
        self.W, self.B = weight, buoyancy
        self.cog, self.cob = np.array(cog, float), np.array(cob, float)

    @classmethod
    def from_abi(cls, u):
        return cls(np.array(u.inertia_matrix[:]).reshape(6, 6), np.array(u.damping_matrices[0][:]).reshape(6, 6),
                   np.array(u.damping_matrices[1][:]).reshape(6, 6), u.weight, u.buoyancy,
                   u.distance_body2centerofgravity[:], u.distance_body2centerofbuoyancy[:])

    def forces(self, M, Dl, Dq, nu, q):
        v, w = nu[..., :3], nu[..., 3:]
        a = nu @ M[:3].T
        b = nu @ M[3:].T
        cor = np.concatenate([np.cross(w, a), np.cross(v, a) + np.cross(w, b)], -1)
        damp = nu @ Dl.T + (np.abs(nu) * nu) @ Dq.T
        qc = qconj(q)
        fg = qrot(qc, np.array([0.0, 0.0, -self.W]))
        fb = qrot(qc, np.array([0.0, 0.0, self.B]))
        g = -np.concatenate([fg + fb, np.cross(self.cog, fg) + np.cross(self.cob, fb)], -1)
        return cor, damp, g

    def efforts(self, acc6, nu, q, M=None, Dl=None, Dq=None):
        M = self.M if M is None else M
        Dl = self.Dl if Dl is None else Dl
        Dq = self.Dq if Dq is None else Dq
        cor, damp, g = self.forces(M, Dl, Dq, nu, q)
        return acc6 @ M.T + cor + damp + g

    def rk4(self, s, tau, dt):
        Minv = np.linalg.inv(self.M)

        def f(s):
            q = s[..., 3:7]
            nu = s[..., 7:13]
            pd = qrot(q, s[..., 7:10])
            wq = np.concatenate([np.zeros(nu.shape[:-1] + (1,)), nu[..., 3:]], -1)
            qd = 0.5 * qmul(q, wq)
            cor, damp, g = self.forces(self.M, self.Dl, self.Dq, nu, q)
            nud = (tau - cor - damp - g) @ Minv.T
            return np.concatenate([pd, qd, nud], -1)

        k1 = f(s)
        k2 = f(s + 0.5 * dt * k1)
        k3 = f(s + 0.5 * dt * k2)
        k4 = f(s + dt * k3)
        o = s + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
        o[..., 3:7] /= np.linalg.norm(o[..., 3:7], axis=-1, keepdims=True)
        return o


# ---------------------------------------------------------------- PoseUKF
class PoseTwin:
    """Single PoseUKF instance (numpy)."""

    def __init__(self, dof, x, P, loc, uwv, param):
        self.lay = Layout(dof)
        self.mu, self.P = np.array(x, float), np.array(P, float)
        self.loc = np.array(loc, float)
        self.uwv = uwv
        self.p = param  # dict of PoseUKFParameter fields
        s = self.lay.s
        if self.lay.full:
            self.off_i = self.mu[s["inertia"]:s["inertia"] + 9].copy()
            self.off_l = self.mu[s["lin"]:s["lin"] + 9].copy()
            self.off_q = self.mu[s["quad"]:s["quad"] + 9].copy()
        self.off_rho = self.mu[s["rho"]]
        self.w = np.zeros(3)
        self.Q = np.zeros((dof, dof))
        self.model_blocks = None  # shared DynamicModel's (surge,sway,yaw) blocks, None = base

    @classmethod
    def from_config(cls, dof, pos, pos_cov, rot, rot_cov, cfg, uwv, imu_in_body=None):
        """PoseUKF.cpp:288-372.  imu_in_body: None (identity) or the 7-vector
        translation + unit quaternion (w, x, y, z) of the Affine3d: the
        translation goes into the parameter (:358), the rotation turns the bias
        offsets (:298-299, :360-362) and the bias blocks of Sigma (:328-329)."""
        lay = Layout(dof)
        s, d = lay.s, lay.d
        x = np.zeros(lay.store)
        x[0:3], x[3:7] = pos, rot
        bg0, ba0 = np.array(cfg["gyro_bias_offset"], float), np.array(cfg["acc_bias_offset"], float)
        Pbg = np.diag(np.square(cfg["gyro_bias_instability"]))
        Pba = np.diag(np.square(cfg["acc_bias_instability"]))
        lever = np.zeros(3)
        if imu_in_body is not None:
            ib = np.asarray(imu_in_body, float)
            lever, Rb = ib[:3].copy(), qmat(ib[3:7])
            bg0, ba0 = Rb @ bg0, Rb @ ba0
            Pbg, Pba = Rb @ Pbg @ Rb.T, Rb @ Pba @ Rb.T
        x[s["bg"]:s["bg"] + 3] = bg0
        x[s["ba"]:s["ba"] + 3] = ba0
        x[s["grav"]] = wgs84_gravity(cfg["lat"], cfg["alt"])
        if lay.full:
            x[s["inertia"]:s["inertia"] + 9] = uwv.M[np.ix_(IDX, IDX)].ravel(order="F")
            x[s["lin"]:s["lin"] + 9] = uwv.Dl[np.ix_(IDX, IDX)].ravel(order="F")
            x[s["quad"]:s["quad"] + 9] = uwv.Dq[np.ix_(IDX, IDX)].ravel(order="F")
        x[s["rho"]] = cfg["rho"]
        P = np.zeros((dof, dof))
        P[0:3, 0:3], P[3:6, 3:6] = pos_cov, rot_cov
        P[6:9, 6:9], P[9:12, 9:12] = np.eye(3), 10 * np.eye(3)
        P[12:15, 12:15] = Pbg
        P[15:18, 15:18] = Pba
        P[18, 18] = 0.05 ** 2
        if lay.full:
            for k in ("inertia", "lin", "quad"):
                P[d[k]:d[k] + 9, d[k]:d[k] + 9] = np.diag(np.square(cfg[k + "_instability"]))
        for k in ("wv", "wvb"):
            P[d[k]:d[k] + 2, d[k]:d[k] + 2] = cfg["wv_limits"] ** 2 * np.eye(2)
        P[d["badcp"]:d["badcp"] + 2, d["badcp"]:d["badcp"] + 2] = cfg["adcp_limits"] ** 2 * np.eye(2)
        P[d["rho"], d["rho"]] = cfg["rho_limits"] ** 2
        param = dict(imu_in_body=lever, gyro_bias_offset=bg0,
                     gyro_bias_tau=cfg["gyro_tau"], acc_bias_offset=ba0,
                     acc_bias_tau=cfg["acc_tau"], inertia_tau=cfg["inertia_tau"], lin_damping_tau=cfg["lin_tau"],
                     quad_damping_tau=cfg["quad_tau"], water_velocity_tau=cfg["wv_tau"],
                     water_velocity_scale=cfg["wv_scale"], adcp_bias_tau=cfg["adcp_tau"],
                     atmospheric_pressure=cfg["patm"], water_density_tau=cfg["rho_tau"])
        f = cls(dof, x, P, (cfg["lat"], cfg["lon"]), uwv, param)
        return f

    def set_noise_from_config(self, cfg, dt, q_imu_in_body=None):
        """PoseUKF.cpp:393-439.  q_imu_in_body: None (identity) or the unit
        quaternion (w, x, y, z) whose matrix turns the orientation, gyro-bias
        and acc-bias blocks (:396, :409-413)."""
        lay, d = self.lay, self.lay.d
        Q = np.zeros((lay.dof, lay.dof))
        j = np.asarray(cfg["max_jerk"], float)
        Q[0:3, 0:3] = np.diag(1.5 * dt ** 4 * (j / 24.0) ** 2)
        Q[6:9, 6:9] = np.diag(1.5 * dt ** 2 * (j / 8.0) ** 2)
        Q[9:12, 9:12] = np.diag((j / 4.0) ** 2)
        Q[3:6, 3:6] = np.diag(np.square(cfg["gyro_randomwalk"]))
        Q[12:15, 12:15] = np.diag(2.0 / (cfg["gyro_tau"] * dt) * np.square(cfg["gyro_bias_instability"]))
        Q[15:18, 15:18] = np.diag(2.0 / (cfg["acc_tau"] * dt) * np.square(cfg["acc_bias_instability"]))
        Q[18, 18] = 1e-12
        if lay.full:
            for k, tk in (("inertia", "inertia_tau"), ("lin", "lin_tau"), ("quad", "quad_tau")):
                Q[d[k]:d[k] + 9, d[k]:d[k] + 9] = np.diag(2.0 / (cfg[tk] * dt) * np.square(cfg[k + "_instability"]))
        for k in ("wv", "wvb"):
            Q[d[k]:d[k] + 2, d[k]:d[k] + 2] = 2.0 / (cfg["wv_tau"] * dt) * cfg["wv_limits"] ** 2 * np.eye(2)
        Q[d["badcp"]:d["badcp"] + 2, d["badcp"]:d["badcp"] + 2] = (2.0 / (cfg["adcp_tau"] * dt) *
                                                                   cfg["adcp_limits"] ** 2 * np.eye(2))
        Q[d["rho"], d["rho"]] = 2.0 / (cfg["rho_tau"] * dt) * cfg["rho_limits"] ** 2
        if q_imu_in_body is not None:
            Rb = qmat(np.asarray(q_imu_in_body, float))
            Q[3:6, 3:6] = Rb @ np.diag(np.square(cfg["gyro_randomwalk"])) @ Rb.T
            Q[12:15, 12:15] = Rb @ ((2.0 / (cfg["gyro_tau"] * dt)) *
                                    np.diag(np.square(cfg["gyro_bias_instability"]))) @ Rb.T
            Q[15:18, 15:18] = Rb @ ((2.0 / (cfg["acc_tau"] * dt)) *
                                    np.diag(np.square(cfg["acc_bias_instability"]))) @ Rb.T
        self.Q = Q

    # -- process model, PoseUKF.cpp:12-84 (vectorised over sigma points)
    def _g(self, X, dt):
        s, p = self.lay.s, self.p
        Y = X.copy()
        Y[:, 0:3] = X[:, 0:3] + dt * X[:, 7:10]
        lat, _ = nav_to_world(self.loc, X[:, 0], X[:, 1])
        er = EARTHW * np.stack([np.cos(lat), np.zeros_like(lat), np.sin(lat)], -1)
        wn = qrot(X[:, 3:7], self.w - X[:, s["bg"]:s["bg"] + 3]) - er
        Y[:, 3:7] = so3_plus(X[:, 3:7], wn * dt, self.lay.right)  # orientation.boxplus, :32
        Y[:, 7:10] = X[:, 7:10] + dt * X[:, 10:13]

        def decay(sl, tau, off):
            Y[:, sl] = X[:, sl] + dt * ((-1.0 / tau) * (X[:, sl] - off))

        decay(slice(s["bg"], s["bg"] + 3), p["gyro_bias_tau"], p["gyro_bias_offset"])
        decay(slice(s["ba"], s["ba"] + 3), p["acc_bias_tau"], p["acc_bias_offset"])
        if self.lay.full:
            decay(slice(s["inertia"], s["inertia"] + 9), p["inertia_tau"], self.off_i)
            decay(slice(s["lin"], s["lin"] + 9), p["lin_damping_tau"], self.off_l)
            decay(slice(s["quad"], s["quad"] + 9), p["quad_damping_tau"], self.off_q)
        decay(slice(s["wv"], s["wv"] + 4), p["water_velocity_tau"], 0.0)
        decay(slice(s["badcp"], s["badcp"] + 2), p["adcp_bias_tau"], 0.0)
        decay(slice(s["rho"], s["rho"] + 1), p["water_density_tau"], self.off_rho)
        return Y

    def predict(self, dt):
        """predictionStepImpl, PoseUKF.cpp:446-465."""
        d = self.lay.d
        Qp = self.Q.copy()
        R = qmat(self.mu[3:7])
        Qp[3:6, 3:6] = R @ self.Q[3:6, 3:6] @ R.T
        vs = self.mu[7:10] * np.array([1, 1, 10.0])
        add = self.p["water_velocity_scale"] * (vs @ vs) * dt
        for k in ("wv", "wvb"):
            Qp[d[k]:d[k] + 2, d[k]:d[k] + 2] += add * np.eye(2)
        self.mu, self.P = ukf_predict(self.lay, self.mu, self.P, lambda X: self._g(X, dt), dt ** 2 * Qp)

    def _upd(self, z, h, R, zman, gate=False):
        self.mu, self.P, acc = ukf_update(self.lay, self.mu, self.P, np.asarray(z, float), h,
                                          np.asarray(R, float), zman, gate)
        return acc

    def rotation_rate_body(self):
        """getRotationRate, PoseUKF.cpp:693-699."""
        lat, _ = nav_to_world(self.loc, self.mu[0], self.mu[1])
        er = EARTHW * np.array([np.cos(lat), 0.0, np.sin(lat)])
        return self.w - self.mu[self.lay.s["bg"]:self.lay.s["bg"] + 3] - qrot(qconj(self.mu[3:7]), er)

    def update(self, kind, z, R, extra=None, only_vel=False):
        s = self.lay.s
        if kind == "acceleration":
            return self._upd(z, lambda X: qrot(qconj(X[:, 3:7]), X[:, 10:13] + np.outer(X[:, s["grav"]], [0, 0, 1]))
                             + X[:, s["ba"]:s["ba"] + 3], R, True)
        if kind == "velocity":
            return self._upd(z, lambda X: qrot(qconj(X[:, 3:7]), X[:, 7:10]), R, True)
        if kind == "pressure":
            sp = np.zeros(3) if extra is None else np.asarray(extra, float)
            return self._upd(z, lambda X: (self.p["atmospheric_pressure"] - (X[:, 2] + qrot(X[:, 3:7], sp)[:, 2]) *
                                           X[:, s["grav"]] * X[:, s["rho"]])[:, None], R, False)
        if kind == "water_velocity":
            cw = float(extra)

            def h(X):
                qi = qconj(X[:, 3:7])
                v = X[:, 7:10]
                wvb = np.concatenate([X[:, s["wvb"]:s["wvb"] + 2], np.zeros((len(X), 1))], 1)
                wv = np.concatenate([X[:, s["wv"]:s["wv"] + 2], np.zeros((len(X), 1))], 1)
                return (cw * qrot(qi, v - wvb) + (1 - cw) * qrot(qi, v - wv))[:, :2] + X[:, s["badcp"]:s["badcp"] + 2]
            return self._upd(z, h, R, True, gate=True)
        if kind == "xy":
            return self._upd(z, lambda X: X[:, 0:2], R, False)
        if kind == "z":
            return self._upd(z, lambda X: X[:, 2:3], R, False)
        if kind == "geographic":
            gps = np.zeros(3) if extra is None else np.asarray(extra, float)
            x, y = world_to_nav(self.loc, z[0], z[1])
            zz = np.array([x, y]) - qrot(self.mu[3:7], gps)[:2]
            return self._upd(zz, lambda X: X[:, 0:2], R, False, gate=True)
        if kind == "delayed_xy":
            zz = np.asarray(z, float) + (self.mu[0:2] - np.asarray(extra, float))
            return self._upd(zz, lambda X: X[:, 0:2], R, False)
        if kind == "efforts":
            return self._efforts(z, R, only_vel)
        raise KeyError(kind)

    def _blocks(self, blk):
        M, Dl, Dq = self.uwv.M.copy(), self.uwv.Dl.copy(), self.uwv.Dq.copy()
        if blk is not None:
            for mat, k in ((M, 0), (Dl, 1), (Dq, 2)):
                mat[np.ix_(IDX, IDX)] = blk[9 * k:9 * k + 9].reshape(3, 3, order="F")
        return M, Dl, Dq

    def _efforts(self, z, R, only_vel):
        """PoseUKF.cpp:153-219, 581-602."""
        s = self.lay.s
        wb = self.rotation_rate_body()
        imu = self.p["imu_in_body"]
        if only_vel:
            q = self.mu[3:7]
            w3 = np.array([self.mu[s["wv"]], self.mu[s["wv"] + 1], 0.0])
            ab = qrot(qconj(q), self.mu[10:13]) - np.cross(wb, np.cross(wb, imu))
            M, Dl, Dq = self._blocks(self.model_blocks)

            def h(X):
                vb = qrot(qconj(q), X[:, 7:10]) - np.cross(wb, imu) - qrot(qconj(q), w3)
                nu = np.concatenate([vb, np.broadcast_to(wb, vb.shape)], 1)
                acc6 = np.concatenate([np.broadcast_to(ab, vb.shape), np.zeros_like(vb)], 1)
                return np.stack([self.uwv.efforts(acc6[i], nu[i], q, M, Dl, Dq) for i in range(len(X))])
            return self._upd(z, h, R, False)

        def h(X):
            out = []
            for x in X:
                blk = None
                if self.lay.full:
                    blk = np.concatenate([x[s["inertia"]:s["inertia"] + 9], x[s["lin"]:s["lin"] + 9],
                                          x[s["quad"]:s["quad"] + 9]])
                M, Dl, Dq = self._blocks(blk)
                qi = qconj(x[3:7])
                wv = np.array([x[s["wv"]], x[s["wv"] + 1], 0.0])
                vb = qrot(qi, x[7:10]) - np.cross(wb, imu) - qrot(qi, wv)
                ab = qrot(qi, x[10:13]) - np.cross(wb, np.cross(wb, imu))
                out.append(self.uwv.efforts(np.concatenate([ab, np.zeros(3)]), np.concatenate([vb, wb]), x[3:7],
                                            M, Dl, Dq))
                if self.lay.full:
                    self.model_blocks = blk  # the shared model keeps the last point's blocks (:173)
            return np.stack(out)
        return self._upd(z, h, R, False)


# ---------------------------------------------------------------- VelocityUKF
class VelTwin:
    def __init__(self, x, P, uwv):
        self.lay = VecLayout(4)
        self.mu, self.P = np.array(x, float), np.array(P, float)
        self.Q = np.diag([1e-4, 1e-4, 1e-4, 0.0])
        self.uwv = uwv
        self.gyro = np.zeros(3)
        self.tau = np.zeros(6)
        self.model = np.concatenate([np.zeros(3), [1.0, 0, 0, 0], self.mu[:3], self.gyro])

    def set_gyro(self, w):
        self.gyro = np.asarray(w, float)
        self.model[10:13] = self.gyro

    def set_efforts(self, tau):
        self.tau = np.asarray(tau, float)

    def set_process_noise(self, Q):
        self.Q = np.array(Q, float)

    def process(self, X, dt):
        """processMotionModel (VelocityUKF.cpp:6-33) on the rows of X"""
        q = self.model[3:7]
        s = np.concatenate([np.zeros((len(X), 3)), np.broadcast_to(q, (len(X), 4)), X[:, :3],
                            np.broadcast_to(self.gyro, (len(X), 3))], 1)
        n = self.uwv.rk4(s, self.tau, dt)
        v = X[:, :3] + (n[:, 7:10] - X[:, :3])
        z = X[:, 3] + dt * qrot(q, v)[:, 2]
        return np.concatenate([v, z[:, None]], 1)

    def predict(self, dt):
        self.mu, self.P = ukf_predict(self.lay, self.mu, self.P, lambda X: self.process(X, dt), dt * self.Q)
        self.model = self.uwv.rk4(self.model, self.tau, dt)

    def update_dvl(self, z, R):
        self.mu, self.P, _ = ukf_update(self.lay, self.mu, self.P, np.asarray(z, float), lambda X: X[:, :3],
                                        np.asarray(R, float), True, False)

    def update_pressure(self, z, R):
        self.mu, self.P, _ = ukf_update(self.lay, self.mu, self.P, np.atleast_1d(np.asarray(z, float)),
                                        lambda X: X[:, 3:4], np.atleast_2d(R), True, False)


# ---------------------------------------------------------------- BottomUKF
class BottomTwin:
    """Single BottomUKF (BottomUKF.cpp): state {distance, normal (S2)}, stored (d, nx, ny, nz)."""

    def __init__(self, x, P):
        self.lay = Compound([("v", 1), ("s2",)])
        x = np.array(x, float)
        self.mu = np.concatenate([x[:1], s2_from(x[1:])])
        self.P = np.array(P, float)
        self.Q = np.eye(3)  # Covariance::Identity(), :45
        self.velocity = np.zeros(3)

    def predict(self, dt):
        """predictionStepImpl :48-54, processModel :5-16."""
        Qp = np.linalg.norm(self.velocity[:2]) ** 2.0 * dt ** 2.0 * self.Q
        vinv = -1.0 * self.velocity[2]

        def g(X):
            Y = X.copy()
            Y[:, 0] = X[:, 0] + vinv * dt
            return Y
        self.mu, self.P = ukf_predict(self.lay, self.mu, self.P, g, Qp)

    def update_range(self, z, cov, direction, origin):
        """integrateMeasurement(RangeMeasurement, ...) :56-61, measurementDistance :18-30."""
        u, o = np.asarray(direction, float), np.asarray(origin, float)

        def h(X):
            n = X[:, 1:4]
            bottom = np.stack([np.zeros(len(X)), np.zeros(len(X)), -X[:, 0]], -1)
            v = n @ u
            w = np.sum((bottom - o) * n, -1)
            return np.where(v != 0.0, w / np.where(v != 0.0, v, 1.0), 0.0)[:, None]
        self.mu, self.P, _ = ukf_update(self.lay, self.mu, self.P, np.atleast_1d(np.asarray(z, float)), h,
                                        np.atleast_2d(np.asarray(cov, float)), True, False)

    def update_normal(self, z, cov):
        """integrateMeasurement(NormalType, cov) :63-67: an S2-valued measurement."""
        self.mu, self.P, _ = ukf_update(self.lay, self.mu, self.P, s2_from(z), lambda X: X[:, 1:4],
                                        np.asarray(cov, float), S2Layout(), False)


# ---------------------------------------------------------------- visual landmark
def qmats(Q):
    """Rotation matrices [N, 3, 3] of quaternions [N, 4]."""
    return np.moveaxis(qmat(np.asarray(Q).T), -1, 0)


def visual_updates(lay, amu, asig, sm, body_pose, features, feature_cov, feature_pos, cam, cam_in):
    """The feature loop of IndirectPoseUKF.cpp:109-131 / PoseUKF.cpp:628-649 on the
    augmented state (marker position at storage offset sm, its quaternion after):
    one S2-valued update per feature, accept_any_mahalanobis_distance.
    body_pose(X) -> (R [N, 3, 3], t [N, 3]) of the body / IMU in nav per sigma point."""
    fx2, fy2, fxy = cam[0] ** 2.0, cam[1] ** 2.0, cam[0] * cam[1]
    Rc, tc = qmat(cam_in[3:7]), np.asarray(cam_in[:3], float)
    for mu_px, cv, f in zip(np.asarray(features, float), np.asarray(feature_cov, float),
                            np.asarray(feature_pos, float)):
        z = s2_from(np.array([(mu_px[0] - cam[2]) / cam[0], (mu_px[1] - cam[3]) / cam[1], 1.0]))
        R = np.array([[cv[0, 0] / fx2, cv[0, 1] / fxy], [cv[1, 0] / fxy, cv[1, 1] / fy2]])

        def h(X):
            Rb, tb = body_pose(X)
            Rcn = Rb @ Rc                       # camera in nav: body_in_nav * cam_in_body
            tcn = tb + Rb @ tc
            fn = qmats(X[:, sm + 3:sm + 7]) @ f + X[:, sm:sm + 3]
            fc = (np.swapaxes(Rcn, -1, -2) @ (fn - tcn)[..., None])[..., 0]  # its inverse
            return s2_from(fc)
        amu, asig, _ = ukf_update(lay, amu, asig, z, h, R, S2Layout(), False)
    return amu, asig


def _augment(mu, P, marker_pose, cov_marker):
    n = P.shape[0]
    amu = np.concatenate([mu, np.asarray(marker_pose, float)])
    asig = np.zeros((n + 6, n + 6))
    asig[:n, :n] = P
    asig[n:, n:] = cov_marker
    return amu, asig


def _pose_update_visual(self, features, feature_cov, feature_pos, marker_pose, cov_marker, cam, cam_in_imu):
    """PoseUKF::integrateMeasurement(vector<VisualFeatureMeasurement>, ...), PoseUKF.cpp:613-654,
    on PoseStateWithMarker (:225-228, n = dof + 6) with measurementVisualLandmark (:233-243)."""
    n, s = self.lay.dof, self.lay.store
    lay = Compound([("v", 3), ("so3",), ("v", n - 6), ("v", 3), ("so3",)], self.lay.right)
    amu, asig = _augment(self.mu, self.P, marker_pose, cov_marker)
    amu, asig = visual_updates(lay, amu, asig, s, lambda X: (qmats(X[:, 3:7]), X[:, 0:3]), features, feature_cov,
                               feature_pos, cam, cam_in_imu)
    self.mu, self.P = amu[:s], asig[:n, :n]


PoseTwin.update_visual = _pose_update_visual


# ---------------------------------------------------------------- IndirectPoseUKF
class IndirectPoseTwin:
    """Single IndirectPoseUKF (IndirectPoseUKF.cpp): state {position_error,
    orientation_error (SO3)}, stored t(3) q(4); poses are t(3) q(4)."""

    def __init__(self, pos_std, ori_std, tau, init_pos_err=None, init_pos_std=None):
        self.lay = Compound([("v", 3), ("so3",)])
        self.mu = np.concatenate([np.zeros(3) if init_pos_err is None else np.asarray(init_pos_err, float),
                                  [1.0, 0.0, 0.0, 0.0]])
        ips = np.ones(3) if init_pos_std is None else np.asarray(init_pos_std, float)
        self.P = np.diag(np.concatenate([np.abs(ips) ** 2, np.abs(ori_std) ** 2]))
        self.Q = np.diag(np.concatenate([np.abs(pos_std) ** 2, np.abs(ori_std) ** 2]))
        self.tau = tau
        self.ref = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])

    def predict(self, dt):
        """predictionStepImpl :80-92, processModel :7-20."""
        rot = qmat(self.mu[3:7])
        Qp = self.Q.copy()
        Qp[3:, 3:] = rot @ ((2.0 / (self.tau * dt)) * self.Q[3:, 3:]) @ rot.T
        Qp = dt ** 2.0 * Qp

        def g(X):
            Y = X.copy()
            d = (-1.0 / self.tau) * so3_log(X[:, 3:7])
            Y[:, 3:7] = so3_plus(X[:, 3:7], d * dt, self.lay.right)
            return Y
        self.mu, self.P = ukf_predict(self.lay, self.mu, self.P, g, Qp)

    def update_visual(self, features, feature_cov, feature_pos, marker_pose, cov_marker, cam, cam_in_body):
        """integrateMeasurement(marker_features, ...) :94-135 on FilterStateWithMarker (:26-30)."""
        lay = Compound([("v", 3), ("so3",), ("v", 3), ("so3",)], self.lay.right)
        amu, asig = _augment(self.mu, self.P, marker_pose, cov_marker)
        Rr, tr = qmat(self.ref[3:7]), self.ref[:3]

        def body(X):  # body_in_nav * pose_error, :42-45
            return Rr @ qmats(X[:, 3:7]), tr + X[:, 0:3] @ Rr.T
        amu, asig = visual_updates(lay, amu, asig, 7, body, features, feature_cov, feature_pos, cam, cam_in_body)
        self.mu, self.P = amu[:7], asig[:6, :6]

    def corrected_pose(self):
        """getCorrectedPose :137-142: pose_ref * pose_error."""
        return np.concatenate([self.ref[:3] + qmat(self.ref[3:7]) @ self.mu[:3], qmul(self.ref[3:7], self.mu[3:7])])


def cfg_dict(c):
    """Flatten an abi.PoseConfig into the dict PoseTwin.from_config expects."""
    m = c.model_noise_parameters
    return dict(gyro_bias_offset=list(c.rotation_rate.bias_offset), acc_bias_offset=list(c.acceleration.bias_offset),
                gyro_bias_instability=list(c.rotation_rate.bias_instability),
                acc_bias_instability=list(c.acceleration.bias_instability),
                gyro_randomwalk=list(c.rotation_rate.randomwalk), gyro_tau=c.rotation_rate.bias_tau,
                acc_tau=c.acceleration.bias_tau, lat=c.location.latitude, lon=c.location.longitude,
                alt=c.location.altitude, rho=c.hydrostatics.water_density,
                rho_limits=c.hydrostatics.water_density_limits, rho_tau=c.hydrostatics.water_density_tau,
                patm=c.hydrostatics.atmospheric_pressure, inertia_instability=list(m.inertia_instability),
                lin_instability=list(m.lin_damping_instability), quad_instability=list(m.quad_damping_instability),
                inertia_tau=m.inertia_tau, lin_tau=m.lin_damping_tau, quad_tau=m.quad_damping_tau,
                wv_limits=c.water_velocity.limits, wv_tau=c.water_velocity.tau, wv_scale=c.water_velocity.scale,
                adcp_limits=c.water_velocity.adcp_bias_limits, adcp_tau=c.water_velocity.adcp_bias_tau,
                max_jerk=list(c.max_jerk))
