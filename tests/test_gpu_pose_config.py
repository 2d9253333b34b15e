"""The PoseUKF kernels on a configuration and a sensor set-up in which no two
numbers are alike (the scenes of tests/pose_config_scenes.py, each valid on the
CPU first: tests/test_pose_config_scenes.py), against the oracle.

Every other PoseUKF test runs on synth.default_pose_config() and
make_pose_log's sensor set-up, or a small variation of them: one gyro random
walk (Q's orientation block sigma^2 I: the mounting's and the attitude's turn
are the identity on it), one max_jerk, one constant per instability vector,
taus equal in groups, diagonal sensor covariances, no pressure lever arm, four
ADCP cells, v_z = 0, dt = 1e-3, one northern latitude metres from the origin.
Here none of that holds:

 1 init_from_config / init_from_state with distinct_config() and the mounting,
   the process noise from the config (still the lane-resident form:
   epoch_qshape() == 1), three predicts from tilted attitudes;
 2 every single call with a full R, shared and per instance;
 3 run_log over full_log with 4, 1 and 8 ADCP cells, over the dive and over the
   log with velocity-only efforts epochs (the PD and pair kernels at 53 DOF run
   all of that one; a full efforts update hands over to the general kernel), on
   every path; pair against the one-instance kernel; in two calls bitwise;
 4 dt = 0.01;
 5 pos0.x up to 500 km from the origin, the halves of every pair wave on
   different sides of the predict's latitude branch, and three other
   latitudes; each instance bitwise what it is beside a partner of its own side;
 6 run_log_fixes with full xy / geo covariances and a GPS lever arm;
 7 run_log_track's records.

Paths and tolerances: tests/test_gpu_pose_edges.py (dense, psp, pd, pair; 1e-9
for a single call, 1e-7 for a log, means in the oracle's sigma and covariances
relative to sqrt(P_ii P_jj)), 1e-15 for the init; accept flags and counts
bitwise.

Measured on an MI355X (max over instances, layouts and sides; mean in sigma /
covariance; 169 tests in 12 s):
 1 init from config and from state 0 / 6.6e-17, rotation rate within 1e-16;
   the three predicts dense 2.4e-14 / 1.8e-13, psp 2.2e-14 / 8.1e-13;
 2 single calls: shared R dense 9.9e-11 / 7.3e-11, psp 1.0e-10 / 7.2e-11; per
   instance dense 7.9e-11 / 7.3e-11, psp 8.1e-11 / 7.2e-11;
 3 full_log with 4, 1 and 8 cells: dense 9.8e-10 / 4.3e-11, psp, pd and pair
   2.2e-9 / 4.8e-11; dive 1.0e-9 / 5.3e-11; velocity-only dense 8.0e-10 /
   2.7e-11, psp, pd and pair 1.8e-9 / 3.0e-11; | |q| - 1 | <= 7.8e-15; pair
   against the one-instance kernel at 53 DOF 1.3e-10 / 2.8e-12 (velocity-only:
   means bitwise, 1.9e-14), bitwise at 26 DOF; cut after the ADCP epoch 2.2e-9;
 4 coarse 2.0e-9 / 3.8e-11;
 5 far dense 3.4e-10 / 1.6e-10, psp, pd and pair 2.2e-9 / 5.1e-10; the three
   latitudes 1.1e-10 / 7.5e-11;
 6 fixes against the oracle 2.6e-9 / 4.8e-11 (bitwise the cut run on all five paths);
 7 the track's records 2.2e-9 / 4.6e-11.
Nothing was found wrong in the kernels.  One scene was: at make_pose_log's
efforts covariance the pair and the one-instance kernel ended 2.1e-9 apart
(left side, 53 DOF), although they run the same code from epoch 3 on: the
velocity-only update of epoch 45 multiplies a rounding-level difference by 190.
pose_config_scenes.EFFORTS_COV and DESIGN.md section 10 say what was changed.

Mutants of csrc/ this module and the existing GPU modules (all of tests/ but the
distributed, mission and benchmark modules: 961 tests) were run against, one
at a time, arithmetic only (169 tests here):
 (a) qo_lane turns Q's orientation block by R^T Q R: fails 138 here (every
     test of a PSP path but test_far_unlike_halves, which compares the kernel
     with itself); of the existing tests only
     test_gpu_surface.py::test_general_process_noise[dense-26-psp] fails;
 (b) qo_lane skips the turn (sh.q_ori[r * 3 + c]): fails 138 here; every
     existing test passes;
 (c) tan_ntau_sel swaps the water-velocity and ADCP-bias taus: fails 138 here;
     every existing test passes;
 (d) the update adds only R's diagonal to S: fails 130 here (the inits have no
     update); 63 existing tests fail too (59 of test_gpu_pose_gates.py, 2 of
     test_gpu_fixes.py::test_fixes_match_oracle, 2 of test_gpu_delayed.py);
 (e) the latitude's library branch uses lat0 alone: fails 10 here, the `far`
     scene on every PSP path; every existing test passes;
 (f) vs2 without the factor 10: fails 122 here (every run_log of a PSP path);
     47 existing tests fail too (test_gpu_pose_model.py 22, test_gpu_efforts.py
     8, test_gpu_surface.py 6, golden, delayed, fixes, parity, pd, track: their
     filters estimate a v_z that is not zero);
 (g) run_log leaves ea.p_sens zero: fails 87 here (every run_log with a
     pressure epoch, the literal path too); every existing test passes.
So five of the seven, (a) on all but one general-Q test, (b), (c), (e) and (g),
passed the suite before this module."""
import functools

import numpy as np
import pytest

import oracle_ctypes as O
import pose_config_scenes as CS
import pose_model_scenes as MS
from helpers import cov_err, state_err
from test_gpu_fixes import PATHS as FIX_PATHS
from test_gpu_fixes import _by_cuts, _same, _with_fixes
from test_gpu_pose_edges import (PATH_DOF, SIDES, SINGLE_PATH_DOF, TOL_LOG, TOL_PAIR, TOL_STEP, check_path, errors,
                                 handle)
from test_gpu_pose_model import TOL_INIT
from uwvk import engine

pytestmark = pytest.mark.gpu

B = 6  # three pair waves, every instance unlike
NAMES = ("state", "covariance", "accept counts", "status", "rotation rate")


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not engine.device_available(0):
        pytest.fail("no gfx950 device / libuwvk.so not loadable: the HIP path is mandatory")


def report(what, path, dof, side, e):
    print("%s %s dof %d %s: state %.3g cov %.3g |q|-1 %.3g" % ((what, path, dof, side) + tuple(e)))


# ---- 1. init and Q -------------------------------------------------------------------
PREDICTS = 3


@functools.lru_cache(maxsize=None)
def init_ref(dof, right):
    log = CS.full_log(B, 4, dof)
    ref = {}
    with O.so3_side(right):
        for how in ("config", "state"):
            o = CS.start(O.OraclePoseBatch(B, dof), log)
            x0, P0 = o.get_state()
            if how == "state":
                CS.start_from_state(o, x0, P0, log["dt"])
            out = [o.get_state() + (o.get_rotation_rate(),)]
            for e in range(PREDICTS):
                o.set_rotation_rate(log["gyro"][e])
                o.predict(log["dt"])
                out.append(o.get_state())
            ref[how] = out
    return log, ref


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("path,dof", SINGLE_PATH_DOF)
@pytest.mark.parametrize("how", ["config", "state"])
def test_init_and_process_noise(how, path, dof, side):
    """init_from_config with the mounting and distinct_config(), or
    init_from_state with synth.pose_parameter(distinct_config()) plus the
    mounting (eight unlike taus); the process noise from the config: its
    orientation block is anisotropic and turned by the mounting, and must still
    be the lane-resident form; three predicts turn it by the attitude."""
    right = side == "right"
    log, ref = init_ref(dof, right)
    g = CS.start(handle(path, dof, B, right), log)
    if how == "state":
        CS.start_from_state(g, *ref["config"][0][:2], log["dt"])
    xo, Po, rate = ref[how][0]
    e = errors(*g.get_state(), xo, Po, dof)
    report("init from %s" % how, path, dof, side, e)
    assert max(e[:2]) < TOL_INIT, e
    np.testing.assert_allclose(g.get_rotation_rate(), rate, rtol=0, atol=1e-16)
    assert g.epoch_qshape() == 1
    for n in range(PREDICTS):
        g.set_rotation_rate(log["gyro"][n])
        g.predict(log["dt"])
        e = errors(*g.get_state(), *ref[how][1 + n], dof)
        report("predict %d after init from %s" % (n, how), path, dof, side, e)
        assert max(e[:2]) < TOL_STEP, (n, e)
    assert not g.get_status().any()


# ---- 2. single calls with full R -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def calls_ref(dof, right, shared):
    log, calls = CS.single_calls(B, dof, shared=shared, right=right)
    ref = {}
    with O.so3_side(right):
        ref["state"] = CS.single_state(O.OraclePoseBatch(B, dof), log).get_state()
        for name, kind, mu, cov, extra, vo in calls:
            o = CS.single_state(O.OraclePoseBatch(B, dof), log)
            acc = o.update(kind, mu, cov, extra=extra, only_vel=vo)
            ref[name] = o.get_state() + (acc,)
    return log, calls, ref


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("path,dof", SINGLE_PATH_DOF)
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_instance"])
def test_single_calls_full_r(shared, path, dof, side):
    """acceleration, velocity, water_velocity, xy, geographic, delayed_xy and
    the two efforts forms from single_state, R the shared full covariance or
    instance i's own: accept flags bitwise (every one accepted), state and
    Sigma to 1e-9, status 0."""
    right = side == "right"
    log, calls, ref = calls_ref(dof, right, shared)
    assert [c[0] for c in calls] == list(CS.SINGLE_KINDS)
    g = handle(path, dof, B, right)
    CS.single_state(g, log)
    worst = list(errors(*g.get_state(), *ref["state"], dof))
    assert max(worst[:2]) < TOL_STEP, ("single_state", worst)
    for name, kind, mu, cov, extra, vo in calls:
        CS.single_state(g, log)
        acc = g.update(kind, mu, cov, extra=extra, only_vel=vo)
        xo, Po, acc_o = ref[name]
        np.testing.assert_array_equal(acc, acc_o, err_msg=name)
        assert acc_o.all(), name
        e = errors(*g.get_state(), xo, Po, dof)
        assert max(e[:2]) < TOL_STEP, (name, e)
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert not g.get_status().any(), name
    report("single calls, %s R" % ("shared" if shared else "per-instance"), path, dof, side, worst)


# ---- 3. - 5. run_log ---------------------------------------------------------------------
LOG_SCENES = ("full", "cells1", "cells8", "dive", "velocity_only")
LAT_SCENES = ("far",) + tuple("lat%g" % lat for lat in CS.LAT_VARIANTS)
LAT_EPOCHS = 40


def scene(name, dof, right):
    """(log, config or None)"""
    if name == "full":
        return CS.full_log(B, dof=dof, right=right), None
    if name in ("cells1", "cells8"):
        return CS.full_log(B, dof=dof, cells=int(name[5:]), right=right), None
    if name == "dive":
        return CS.dive_log(B, dof=dof, right=right), None
    if name == "velocity_only":
        return CS.full_log(B, dof=dof, right=right, velocity_only=True), None
    if name == "coarse":
        return CS.coarse(CS.full_log(B, dof=dof)), None
    if name == "far":
        return CS.far(CS.tight(CS.coarse(CS.full_log(B, dof=dof)))), None
    lat = float(name[3:])
    return CS.cut(CS.full_log(B, dof=dof), LAT_EPOCHS), CS.with_latitude(lat)


@functools.lru_cache(maxsize=None)
def log_ref(name, dof, right):
    log, cfg = scene(name, dof, right)
    with O.so3_side(right):
        o = CS.start_scene(O.OraclePoseBatch(B, dof), log, cfg)
        counts = o.run_log(log)
        ref = o.get_state() + (counts,)
    return log, cfg, ref


def run_scene(path, dof, right, log, cfg=None, cuts=()):
    g = CS.start_scene(handle(path, dof, log["batch"], right), log, cfg)
    check_path(g, path, dof)
    acc = engine.DeviceBuffer(np.zeros((log["batch"], 4), np.uint32))
    dlog = g.upload_log(log)
    edges = [0] + [c for c in cuts if c < log["epochs"]] + [log["epochs"]]
    for a, b in zip(edges[:-1], edges[1:]):
        g.run_log(dlog, a, b - a, accept_counts=acc)
    x, P = g.get_state()
    return (x, P, acc.read(np.uint32, (log["batch"], 4)), g.get_status(), g.get_rotation_rate(),
            (g.pair_active(), g.param_block()))


def against_oracle(name, path, dof, side):
    right = side == "right"
    log, cfg, (xo, Po, counts) = log_ref(name, dof, right)
    x, P, acc, status, _, kernels = run_scene(path, dof, right, log, cfg)
    np.testing.assert_array_equal(acc, counts)
    assert not status.any()
    e = errors(x, P, xo, Po, dof)
    report(name, path, dof, side, e)
    assert max(e[:2]) < TOL_LOG, e
    return log, counts, kernels


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("path,dof", PATH_DOF)
@pytest.mark.parametrize("name", LOG_SCENES)
def test_full_logs(name, path, dof, side):
    log, counts, kernels = against_oracle(name, path, dof, side)
    # every DVL, pressure and efforts update and every placed ADCP cell accepted
    np.testing.assert_array_equal(counts, [CS.expected_counts(log)] * B)
    assert min(CS.expected_counts(log)) >= 1
    if dof == 53 and path in ("pd", "pair"):
        # a full efforts update couples the parameter block (tests/test_gpu_pd.py): the PD / pair kernel ran
        # epochs 0 .. 2 only; the velocity-only log leaves it decoupled and they ran all of it
        assert kernels == ((int(path == "pair"), 1) if name == "velocity_only" else (0, 0))


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("dof", [53, 26])
@pytest.mark.parametrize("name", LOG_SCENES)
def test_pair_against_one_instance_kernel(name, dof, side):
    """The pair kernel within 1e-9 of the one-instance kernel on the same batch;
    the same log in two calls, cut after the first efforts epoch (where run_log
    ends a launch anyway), bitwise the single call.  A cut inside a launch
    (after the ADCP epoch) folds the time scale of DESIGN.md section 4.4 back
    at another epoch, which changes the rounding: that run is held to the
    oracle like the single call, its accept counts bitwise."""
    right = side == "right"
    log, cfg, (xo, Po, counts) = log_ref(name, dof, right)
    pair = run_scene("pair", dof, right, log, cfg)
    one = run_scene("pd", dof, right, log, cfg)
    np.testing.assert_array_equal(pair[2], one[2])
    es, ec = state_err(pair[0], one[0], one[1], dof).max(), cov_err(pair[1], one[1]).max()
    print("%s dof %d %s pair against the one-instance kernel: state %.3g cov %.3g" % (name, dof, side, es, ec))
    assert es < TOL_PAIR and ec < TOL_PAIR
    parts = run_scene("pair", dof, right, log, cfg, cuts=(MS.EFFORTS_EPOCHS[0] + 1,))
    for what, u, v in zip(NAMES, pair, parts):
        np.testing.assert_array_equal(u, v, err_msg=what)
    inside = run_scene("pair", dof, right, log, cfg, cuts=(CS.ADCP_EPOCH + 1,))
    np.testing.assert_array_equal(inside[2], counts)
    e = errors(inside[0], inside[1], xo, Po, dof)
    report(name + " cut after the ADCP epoch", "pair", dof, side, e)
    assert max(e[:2]) < TOL_LOG and not inside[3].any(), e


@pytest.mark.parametrize("path,dof", PATH_DOF)
def test_coarse(path, dof):
    """dt = 0.01: the process noise for that dt, A_ii = 1 - dt / tau ten times further from 1"""
    log, counts, _ = against_oracle("coarse", path, dof, "right")
    np.testing.assert_array_equal(counts, [[1, 0, 0, 2]] * B)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("path,dof", PATH_DOF)
@pytest.mark.parametrize("name", LAT_SCENES)
def test_far_and_latitudes(name, path, dof, side):
    log, _, _ = against_oracle(name, path, dof, side)
    if name == "far":
        lib = CS.library_branch(log["pos0"][:, 0])
        assert sum(lib[2 * u] != lib[2 * u + 1] for u in range(B // 2)) >= 2


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("dof", [53, 26])
def test_far_unlike_halves(dof, side):
    """On the pair path the halves of every wave of `far` take different
    branches of the predict's latitude.  Each instance is bitwise the same
    instance in its own slot of a wave whose other half lies on its side (a
    copy of itself): the unlike-halves contract of tests/test_gpu_pose_edges.py."""
    right = side == "right"
    log, cfg, _ = log_ref("far", dof, right)
    mixed = run_scene("pair", dof, right, log, cfg)
    for i in range(B):
        own = run_scene("pair", dof, right, CS.own_side_partner(log, i), cfg)
        for what, u, v in zip(NAMES, mixed, own):
            np.testing.assert_array_equal(u[i], v[i % 2], err_msg="%s of instance %d" % (what, i))


# ---- 6. fixes ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixes_ref(batch, dof, right):
    log = CS.full_log(batch, dof=dof, right=right)
    fx = CS.fixes_for(log, dof)
    with O.so3_side(right):
        ref = CS.oracle_run_fixes(log, fx, dof)
    return log, fx, ref


@pytest.mark.parametrize("B_,dof,pd,right,kernels", FIX_PATHS)
def test_fixes(B_, dof, pd, right, kernels):
    """run_log_fixes with a full xy_cov, a correlated geo_cov and a GPS lever
    arm at a southern latitude: bitwise run_log cut at the fix epochs with the
    single calls at the cuts (the contract of tests/test_gpu_fixes.py), and the
    oracle advanced piecewise; accept counts of the fixes bitwise."""
    log, fx, (xo, Po, acc_o, facc_o) = fixes_ref(B_, dof, right)

    def start():
        g = engine.PoseUKFBatch(B_, dof)
        g.set_param_block(pd)
        g.set_so3_right(right)
        return CS.start(g, log)

    ga, gb = start(), start()
    assert (ga.pair_active(), ga.param_block()) == kernels
    got = _with_fixes(engine, ga, log, fx)
    ref = _by_cuts(engine, gb, log, fx)
    _same(got, ref)
    assert not got["status"].any()
    np.testing.assert_array_equal(got["acc"], acc_o)
    np.testing.assert_array_equal(got["facc"], facc_o)
    np.testing.assert_array_equal(facc_o, [[2, 1, 2]] * B_)
    e = errors(got["x"], got["P"], xo, Po, dof)
    print("fixes B %d dof %d pd %d right %d: state %.3g cov %.3g |q|-1 %.3g" % ((B_, dof, pd, right) + e))
    assert max(e[:2]) < TOL_LOG, e


# ---- 7. the track ------------------------------------------------------------------------------
EVERY = 50


@pytest.mark.parametrize("dof", [53, 26])
def test_track_records(dof):
    """run_log_track with every = 50 on the pair path: the mean and variance
    records against the oracle's states at those epochs"""
    log, cfg, (xo, Po, counts) = log_ref("full", dof, True)
    g = CS.start_scene(handle("pair", dof, B, True), log, cfg)
    check_path(g, "pair", dof)
    acc = engine.DeviceBuffer(np.zeros((B, 4), np.uint32))
    tr = g.run_log_track(g.upload_log(log), EVERY, accept_counts=acc)
    rec = np.arange(EVERY - 1, log["epochs"], EVERY)
    np.testing.assert_array_equal(tr.epochs, rec)
    np.testing.assert_array_equal(acc.read(np.uint32, (B, 4)), counts)
    mean, var = tr.mean(), tr.variance()
    o = CS.start_scene(O.OraclePoseBatch(B, dof), log, cfg)
    worst = [0.0, 0.0]
    for r in range(len(rec)):
        o.run_log(log, r * EVERY, EVERY)
        x, P = o.get_state()
        d = np.diagonal(P, axis1=1, axis2=2)
        es, ev = state_err(mean[r], x, P, dof).max(), (np.abs(var[r] - d) / d).max()
        worst = [max(worst[0], es), max(worst[1], ev)]
        assert es < TOL_LOG and ev < TOL_LOG, (r, es, ev)
    print("track dof %d: state %.3g variance %.3g" % (dof, worst[0], worst[1]))
    x, P = g.get_state()
    np.testing.assert_array_equal(mean[-1], x)
    np.testing.assert_array_equal(var[-1], np.diagonal(P, axis1=1, axis2=2))
    assert not g.get_status().any()
