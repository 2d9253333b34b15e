"""GPU parity for the PoseUKF surface around the hot loop, through the C ABI,
against the CPU oracle on the same seeded inputs.

Covers:
* resetFilterWithExternalPose      /root/reference/src/PoseUKF.cpp:685-691
* getRotationRate                  PoseUKF.cpp:693-699
* PoseUKF(state, cov, location, model, param)   PoseUKF.cpp:374-391
* setProcessNoiseCovariance with a general Q (the [EXT] base call that
  setProcessNoiseFromConfig ends in, PoseUKF.cpp:438; applied in
  predictionStepImpl :446-474), incl. q_imu_in_body (:410-412)
* the measurementEfforts -> constrainVelocity shared-model side effect:
  measurementEfforts leaves the filter's DynamicModel holding the last sigma
  point's parameters (:173), the velocity-only update then runs on them (:592)
* a C1-length single-filter run (60,000 epochs, 300 DVL updates)
* C4 at full batch (65,536 instances, 2,000 epochs, compressed drop-out cycle)
  checked on instances spread over the XCD map.

Tolerances as tests/test_gpu_parity.py: 1e-9 (in oracle std-devs and
sqrt(P_ii P_jj)) per single call, 1e-7 over multi-epoch logs; the C1-length
run is held to TOL_C1 (stated below, drift measured on MI355X).
"""
import numpy as np
import pytest

from helpers import cov_err, init_both, pose_setup, state_err

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-9
TOL_LOG = 1e-7
# 60,000-epoch single filter: the engine/oracle rounding differences (summation
# order, FMA contraction, the PSP/time-scale reformulations) random-walk through
# the recursion; r02 measured the drift on MI355X
TOL_C1 = 1e-6


@pytest.fixture(scope="module")
def eng():
    from uwvk import engine
    if not engine.device_available(0):
        pytest.fail("no gfx950 device / libuwvk.so not loadable: the HIP path is mandatory")
    return engine


@pytest.fixture(scope="module")
def orc():
    import oracle_ctypes
    return oracle_ctypes


def _mk(eng, B, dof=53, path="psp"):
    g = eng.PoseUKFBatch(B, dof)
    if path == "dense":
        g.set_dense_sigma(True)
    return g


def _check(o, g, dof, tol):
    (xo, Po), (xg, Pg) = o.get_state(), g.get_state()
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(Pg))
    se, ce = state_err(xg, xo, Po, dof).max(), cov_err(Pg, Po).max()
    assert se < tol, "state error %g" % se
    assert ce < tol, "covariance error %g" % ce
    return se, ce


def _run_both(o, g, log, first, count):
    co = o.run_log(log, first, count)
    acc = None
    if g is not None:
        from uwvk import engine
        acc = engine.DeviceBuffer(np.zeros((g.batch, 4), np.uint32))
        g.run_log(g.upload_log(log), first, count, accept_counts=acc)
        np.testing.assert_array_equal(co, acc.read(np.uint32, (g.batch, 4)))
    return co


def _param():
    from uwvk import abi
    p = abi.PoseParameter()
    abi.fill(p.imu_in_body, [0.3, -0.1, 0.05])
    abi.fill(p.gyro_bias_offset, [1e-5, -2e-5, 5e-6])
    p.gyro_bias_tau = 600.0
    abi.fill(p.acc_bias_offset, [1e-3, 0.0, -2e-3])
    p.acc_bias_tau = 600.0
    p.inertia_tau = p.lin_damping_tau = p.quad_damping_tau = 3600.0
    p.water_velocity_tau, p.water_velocity_limits, p.water_velocity_scale = 900.0, 0.1, 1e-3
    p.adcp_bias_tau, p.atmospheric_pressure, p.water_density_tau = 900.0, 101325.0, 3600.0
    return p


# ---- resetFilterWithExternalPose / getRotationRate -------------------------------

@pytest.mark.parametrize("path", ["psp", "dense"])
@pytest.mark.parametrize("dof", [53, 26])
def test_reset_with_external_pose(eng, orc, dof, path):
    """PoseUKF.cpp:685-691: position and orientation replaced, every other
    component and the whole covariance kept; then the filter runs on."""
    B = 4
    cfg, uwv, log = pose_setup(B, dof, "C4", 800)
    o, g = orc.OraclePoseBatch(B, dof), _mk(eng, B, dof, path)
    init_both(o, g, cfg, uwv, log)
    _run_both(o, g, log, 0, 400)
    x0, P0 = g.get_state()
    rng = np.random.default_rng(11)
    pose = np.empty((B, 7))
    pose[:, :3] = x0[:, :3] + rng.standard_normal((B, 3)) * [2.0, 2.0, 0.5]
    q = x0[:, 3:7] + 0.05 * rng.standard_normal((B, 4))
    q *= np.sign(q[:, :1])  # either sign: the engine must accept both hemispheres
    q[1] = -q[1]
    pose[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    for f in (o, g):
        f.reset_with_external_pose(pose)
    x1, P1 = g.get_state()
    np.testing.assert_array_equal(P1, P0)  # sigma kept bit for bit
    np.testing.assert_array_equal(x1[:, 7:], x0[:, 7:])
    np.testing.assert_array_equal(x1[:, :3], pose[:, :3])
    _check(o, g, dof, TOL_STEP)
    _run_both(o, g, log, 400, 400)
    assert not g.get_status().any()
    _check(o, g, dof, TOL_LOG)


@pytest.mark.parametrize("dof", [53, 26])
def test_get_rotation_rate(eng, orc, dof):
    """PoseUKF.cpp:693-699: stored rate - gyro bias - q^-1 * earth rate at the
    latitude of the current position (GeographicProjection::navToWorld)."""
    B = 5
    cfg, uwv, log = pose_setup(B, dof, "C4", 600)
    o, g = orc.OraclePoseBatch(B, dof), _mk(eng, B, dof)
    init_both(o, g, cfg, uwv, log)
    # move the estimate well away from the origin so the latitude term matters
    x, P = o.get_state()
    x[:, 0] += np.linspace(-5e4, 5e4, B)
    x[:, 13:16] = np.array([1e-4, -2e-4, 3e-4])  # gyro bias (store slots 13-15, both layouts)
    loc = __import__("uwvk").abi.Location(0.925, 0.154, 0.0)
    for f in (o, g):
        f.init_from_state(x, P, loc, uwv, _param())
    _run_both(o, g, log, 0, 300)
    _check(o, g, dof, TOL_LOG)
    w = log["gyro"][299] + 1e-3
    for f in (o, g):
        f.set_rotation_rate(w)
    ro, rg = o.get_rotation_rate(), g.get_rotation_rate()
    # host restatement from each side's own state (diagnostic for a mismatch)
    from uwvk import synth
    from helpers import qrot_inv
    for name, f in (("oracle", o), ("engine", g)):
        xs = f.get_state()[0]
        lat = 0.925 + xs[:, 0] / 6.3727e6
        er = synth.EARTHW * np.stack([np.cos(lat), 0 * lat, np.sin(lat)], 1)
        hr = w - xs[:, 13:16] - qrot_inv(xs[:, 3:7], er)
        print(name, "vs host form:", np.abs(hr - (ro if name == "oracle" else rg)).max())
    np.testing.assert_allclose(rg, ro, rtol=0, atol=1e-12 * np.abs(ro).max())
    # before any rate is stored the reference returns - bias - q^-1 w_earth (rotation_rate = 0)
    g2, o2 = _mk(eng, B, dof), orc.OraclePoseBatch(B, dof)
    init_both(o2, g2, cfg, uwv, log)
    np.testing.assert_allclose(g2.get_rotation_rate(), o2.get_rotation_rate(), rtol=0, atol=1e-16)


# ---- second constructor ------------------------------------------------------------

@pytest.mark.parametrize("path", ["psp", "dense"])
@pytest.mark.parametrize("dof", [53, 26])
def test_init_from_state(eng, orc, dof, path):
    """PoseUKF(state, cov, location, model, param) (PoseUKF.cpp:374-391): the
    model-parameter offsets come from the given state, rotation_rate = 0, the
    projection from `location`; then a C4 log (ADCP, pressure, efforts)."""
    from uwvk import abi
    B = 3
    cfg, uwv, log = pose_setup(B, dof, "C4", 300)
    o = orc.OraclePoseBatch(B, dof)
    o.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    o.set_process_noise_from_config(cfg, 1e-3)
    o.run_log(log)
    x, P = o.get_state()
    rng = np.random.default_rng(5)
    lay = abi.layout(dof)
    if dof == 53:
        x[:, 20:47] *= 1.0 + 0.05 * rng.standard_normal((B, 27))  # model parameters (become the offsets)
    x[:, lay["s_wv"]:lay["s_wv"] + 2] += 0.05
    x[:, lay["s_rho"]] += 3.0
    P = P + np.eye(dof)[None] * 1e-6
    loc = abi.Location(0.9251, 0.1538, 12.0)
    _, _, log2 = pose_setup(B, dof, "C4", 800, seed=77)
    o2, g = orc.OraclePoseBatch(B, dof), _mk(eng, B, dof, path)
    for f in (o2, g):
        f.init_from_state(x, P, loc, uwv, _param())
        f.set_process_noise_from_config(cfg, 1e-3)
    _check(o2, g, dof, 1e-15)
    np.testing.assert_allclose(g.get_rotation_rate(), o2.get_rotation_rate(), rtol=0, atol=1e-16)
    _run_both(o2, g, log2, 0, 800)
    assert not g.get_status().any()
    _check(o2, g, dof, TOL_LOG)


# ---- general process noise ---------------------------------------------------------

def _corr(n, rng, strength):
    """Random SPD matrix with unit diagonal."""
    G = rng.standard_normal((n, n))
    C = G @ G.T
    d = np.sqrt(np.diag(C))
    C = C / np.outer(d, d)
    return (1 - strength) * np.eye(n) + strength * C


def _q_variants(cfg, dof, rng):
    """Three Q shapes outside setProcessNoiseFromConfig's, around its diagonal
    (the config Q from the independent numpy twin, oracle/numpy_twin.py)."""
    import numpy_twin as T
    from uwvk import synth
    tw = T.PoseTwin.from_config(dof, np.zeros(3), np.eye(3), np.array([1.0, 0, 0, 0]), np.eye(3) * 1e-4,
                                T.cfg_dict(cfg), T.UWV.from_abi(synth.default_uwv()))
    tw.set_noise_from_config(T.cfg_dict(cfg), 1e-3)
    base = tw.Q.copy()
    sd = np.sqrt(np.diag(base))
    dense = np.outer(sd, sd) * _corr(dof, rng, 0.4)  # couples every row, band >> 128 entries
    rows9 = base.copy()  # couplings into the rewritten rows (< 9) only: velocity x acceleration, pos x bias
    for i, j, c in ((6, 9, 0.3), (7, 10, -0.2), (8, 11, 0.25), (0, 15, 0.1)):
        rows9[i, j] = rows9[j, i] = c * sd[i] * sd[j]
    wide = base.copy()  # rows >= 9 only, bandwidth 6 (not the lane-resident shape), band fits or not by dof
    for i in range(9, dof):
        for j in range(max(9, i - 6), i):
            wide[i, j] = wide[j, i] = 0.1 * sd[i] * sd[j]
    return {"dense": dense, "rows9": rows9, "wide": wide}


@pytest.mark.parametrize("path", ["psp", "dense"])
@pytest.mark.parametrize("dof", [53, 26])
@pytest.mark.parametrize("variant", ["dense", "rows9", "wide"])
def test_general_process_noise(eng, orc, dof, path, variant):
    """setProcessNoiseCovariance with a Q outside setProcessNoiseFromConfig's
    shape: single predict steps, then a C4 log in one run_log call."""
    B = 3
    cfg, uwv, log = pose_setup(B, dof, "C4", 600)
    Q = _q_variants(cfg, dof, np.random.default_rng(3))[variant]
    np.linalg.cholesky(Q)  # positive definite (eigvalsh cannot resolve Q's 1e-16 .. 2 diagonal)
    o, g = orc.OraclePoseBatch(B, dof), _mk(eng, B, dof, path)
    init_both(o, g, cfg, uwv, log)
    for f in (o, g):
        f.set_process_noise(Q)
    assert g.epoch_qshape() == 2  # run_log takes the general-Q instantiation of the epoch kernel
    for e in range(3):
        for f in (o, g):
            f.set_rotation_rate(log["gyro"][e])
            f.predict(1e-3)
        _check(o, g, dof, TOL_STEP)
    _run_both(o, g, log, 3, 597)
    assert not g.get_status().any()
    _check(o, g, dof, TOL_LOG)


@pytest.mark.parametrize("path", ["psp", "dense"])
def test_process_noise_imu_in_body_single_predict(eng, orc, path):
    """setProcessNoiseFromConfig with a non-identity q_imu_in_body (PoseUKF.cpp:
    410-412 rotate the bias blocks), then ONE predictionStep right away (the
    advisor's r01 finding: the first predict must see the new Q shape).
    The default config's blocks are isotropic, so the rotation is the identity
    on them; tests/test_gpu_pose_config.py runs a config on which it has teeth."""
    B = 4
    cfg, uwv, log = pose_setup(B, 53, "C3", 10)
    qb = np.array([np.cos(0.3), np.sin(0.3) * 0.6, 0.0, np.sin(0.3) * 0.8])
    o, g = orc.OraclePoseBatch(B, 53), _mk(eng, B, 53, path)
    for f in (o, g):
        f.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
        f.set_process_noise_from_config(cfg, 1e-3, q_imu_in_body=qb)
        f.set_rotation_rate(log["gyro"][0])
        f.predict(1e-3)
    _check(o, g, 53, TOL_STEP)
    assert g.epoch_qshape() == 1  # the config's Q (rotated bias blocks): the simple-Q instantiation


# ---- measurementEfforts -> constrainVelocity side effect ---------------------------

@pytest.mark.parametrize("path", ["psp", "dense"])
@pytest.mark.parametrize("dof", [53, 26])
def test_efforts_then_velocity_only_single_calls(eng, orc, dof, path):
    """Full efforts update, predict, then a velocity-only efforts update on the
    same filters: the second runs on the model the first left behind
    (PoseUKF.cpp:173 -> :592).  That model is the prior mean's parameters (the
    last sigma point differs from mu only in the water density), so it departs
    from the configured one from the second full update on: the velocity-only
    update at e = 4 is the one that depends on it
    (tests/test_oracle_kat.py::test_efforts_side_effect_reaches_velocity_only_update)."""
    B = 4
    cfg, uwv, log = pose_setup(B, dof, "C4", 10)
    o, g = orc.OraclePoseBatch(B, dof), _mk(eng, B, dof, path)
    init_both(o, g, cfg, uwv, log)
    rng = np.random.default_rng(9)
    R = np.diag([25.0, 25, 25, 1, 1, 1])
    for e, only_vel in enumerate((0, 1, 1, 0, 1)):
        for f in (o, g):
            f.set_rotation_rate(log["gyro"][e])
            f.predict(1e-3)
        tau = 20 * rng.standard_normal((B, 6))
        ao = o.update("efforts", tau, R, only_vel=only_vel)
        ag = g.update("efforts", tau, R, only_vel=only_vel)
        np.testing.assert_array_equal(ao, ag)
        _check(o, g, dof, TOL_STEP)


@pytest.mark.parametrize("path", ["psp", "dense"])
def test_efforts_mixed_run_log(eng, orc, path):
    """run_log with BodyEfforts epochs alternating full / velocity-only
    (EV_EFFORTS_VELOCITY_ONLY): every velocity-only update follows a full one
    on the same filter and must see its model."""
    from uwvk import abi
    B = 4
    cfg, uwv, _ = pose_setup(B, 53, "C4", 10)
    from uwvk import synth
    log = synth.make_pose_log(B, 1600, "C4", dropout_on=0.2, dropout_off=0.2)
    eff = np.nonzero(log["flags"] & abi.EV_EFFORTS)[0]
    assert len(eff) >= 6
    log["flags"][eff[1::2]] |= abi.EV_EFFORTS_VELOCITY_ONLY
    o, g = orc.OraclePoseBatch(B, 53), _mk(eng, B, 53, path)
    init_both(o, g, cfg, uwv, log)
    _run_both(o, g, log, 0, 1600)
    assert not g.get_status().any()
    _check(o, g, 53, TOL_LOG)


# ---- long horizon ------------------------------------------------------------------

def test_c1_length_single_filter(eng, orc):
    """one filter, 60,000 epochs of 1 kHz IMU + 5 Hz DVL
    (300 DVL updates), one run_log call; the drift against the oracle must stay
    below TOL_C1."""
    from uwvk import abi
    cfg, uwv, log = pose_setup(1, 53, "C1", 60000)
    assert int(((log["flags"] & abi.EV_DVL) != 0).sum()) == 300
    o, g = orc.OraclePoseBatch(1, 53), _mk(eng, 1, 53)
    init_both(o, g, cfg, uwv, log)
    _run_both(o, g, log, 0, 60000)
    assert not g.get_status().any()
    se, ce = _check(o, g, 53, TOL_C1)
    print("C1 60k epochs: state err %.3e sd, cov err %.3e" % (se, ce))


# ---- C4 at full batch --------------------------------------------------------------

def _xcd_samples(B, n=16):
    """Instances spread over the XCD map: block i goes to XCD i % 8, so take
    pairs at both ends of each XCD's round-robin range and the ragged tail."""
    s = set()
    for x in range(8):
        s.add(x)
        s.add(B // 2 + 8 * 97 + x)
    s.update((B - 1, B - 9, 12345, 40001))
    return sorted(s)[:n + 4]


@pytest.mark.timeout(900)
def test_c4_full_batch_sampled(eng, orc):
    """C4 at batch 65,536 over 2,000 epochs with the drop-out cycle compressed
    100x (0.3 s / 0.1 s: 8 DVL, 2 ADCP, 20 pressure and 7 BodyEfforts epochs):
    the PSP launches split at the efforts epochs and the efforts update on
    k_psp_efforts (PSP, k = 48, since r05), as in the C4 bench.  Sampled instances against the oracle
    (their logs are generated alone: the Philox streams are keyed by the
    global instance id), no status bits, and a second run bitwise equal."""
    from uwvk import abi, synth
    B, E = 65536, 2000
    cyc = dict(dropout_on=0.3, dropout_off=0.1)
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    log = synth.make_pose_log(B, E, "C4", **cyc)
    assert int(((log["flags"] & abi.EV_EFFORTS) != 0).sum()) == 7
    g = _mk(eng, B, 53)
    g.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    g.set_process_noise_from_config(cfg, 1e-3)
    dlog = g.upload_log(log)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    g.run_log(dlog, accept_counts=acc)
    counts = acc.read(np.uint32, (B, 4))
    assert not g.get_status().any()
    xg, Pg = g.get_state()
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(Pg))
    # determinism: a second handle on the same inputs, bit for bit
    g2 = _mk(eng, B, 53)
    g2.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    g2.set_process_noise_from_config(cfg, 1e-3)
    g2.run_log(dlog)
    x2, P2 = g2.get_state()
    np.testing.assert_array_equal(x2, xg)
    np.testing.assert_array_equal(P2, Pg)
    del g2, x2, P2
    samples = _xcd_samples(B)
    one = synth.make_pose_log(1, E, "C4", first_instance=samples[0], **cyc)
    np.testing.assert_array_equal(one["acc"][:, 0], log["acc"][:, samples[0]])
    del log, dlog
    for i in samples:
        li = synth.make_pose_log(1, E, "C4", first_instance=i, **cyc)
        o = orc.OraclePoseBatch(1, 53)
        o.init_from_config(li["pos0"], li["pos_cov"], li["rot0"], li["rot_cov"], cfg, uwv)
        o.set_process_noise_from_config(cfg, 1e-3)
        co = o.run_log(li)
        np.testing.assert_array_equal(co[0], counts[i])
        xo, Po = o.get_state()
        se = state_err(xg[i:i + 1], xo, Po, 53).max()
        ce = cov_err(Pg[i:i + 1], Po).max()
        assert se < TOL_LOG and ce < TOL_LOG, "instance %d: state %g cov %g" % (i, se, ce)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("persist", [None, 0])
def test_headline_shape_sampled(eng, orc, persist):
    """The exact shape of the driver's bench line: C3 at
    batch 65,536, the Monte-Carlo start through the second constructor
    (bench.initialise "mc", PoseUKF.cpp:374-391), the DVL-aligned log
    (bench.window_shift) with its alignment shift and 5-epoch warm-up in
    launches of the window's length, then the 20-epoch
    window in ONE run_log launch (right SO3 side, no pressure / ADCP events):
    since r06 the default is the two-instances-per-wave parameter-decoupled
    kernel k_psp_epoch_pair<1, 1, 1> on the persistent scheduler (pair units
    from the ticket counter; no tail spreading for pair launches since r06v);
    persist=0 runs the one-instance
    PD kernel k_psp_epoch_p<26, 1, 1, 1, 1> in the static tail-spread launch.
    16+ XCD-spread instances (tail instances included)
    against the oracle, each run alone on its own one-instance log (the
    Philox streams are keyed by the global instance id)."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from uwvk import synth
    B, warmup, steps = 65536, 5, 20
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    log, shift = bench.dvl_aligned_log(synth, B, warmup, steps, "C3", 53, 0, cfg=cfg)
    e0 = shift + warmup
    assert int(((log["flags"][e0:] & 2) != 0).sum()) >= 1  # the window holds its DVL epoch
    g = _mk(eng, B, 53)
    if persist is not None:
        g.set_persist(persist)
    bench.initialise(g, log, cfg, uwv, "mc")
    g.set_process_noise_from_config(cfg, log["dt"])
    assert g.param_block() == 1 and g.pair_active() == (1 if persist is None else 0)
    dlog = g.upload_log(log)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    p0 = e0 % steps  # bench.py's untimed launches: the remainder, then the window's length
    if p0:
        g.run_log(dlog, 0, p0, accept_counts=acc)
    for q in range(p0, e0, steps):
        g.run_log(dlog, q, min(steps, e0 - q), accept_counts=acc)
    g.run_log(dlog, e0, steps, accept_counts=acc)
    counts = acc.read(np.uint32, (B, 4))
    assert not g.get_status().any()
    xg, Pg = g.get_state()
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(Pg))
    del log, dlog
    samples = _xcd_samples(B)
    # the persistent plan's tail units are the last instances of the batch
    samples = sorted(set(samples) | {B - 2, B - 100, B - 3000})
    for i in samples:
        li, _ = bench.dvl_aligned_log(synth, 1, warmup, steps, "C3", 53, i, cfg=cfg)
        o = orc.OraclePoseBatch(1, 53)
        bench.initialise(o, li, cfg, uwv, "mc", first_instance=i)
        o.set_process_noise_from_config(cfg, li["dt"])
        co = o.run_log(li)
        np.testing.assert_array_equal(co[0], counts[i])
        xo, Po = o.get_state()
        se = state_err(xg[i:i + 1], xo, Po, 53).max()
        ce = cov_err(Pg[i:i + 1], Po).max()
        assert se < TOL_LOG and ce < TOL_LOG, "instance %d: state %g cov %g" % (i, se, ce)
