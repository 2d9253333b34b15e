"""Edge tests of the PoseUKF kernels on the scenes of tests/pose_scenes.py (each
valid on the CPU first: tests/test_pose_scenes.py).

 B1 wide orientation priors against the oracle: the library branches of
    so3_exp_psp / so3_log_psp (csrc/uwvk_psp_dev.hpp), lanes of one wave on
    different branches (straddle), the process model's own exp (big_step, and
    far_step at 2.56 rad, where the series would be wrong by more than the
    tolerance), the quaternion double cover (the odd instances of wide start
    from -q0);
 B2 a pair wave whose two halves hold unlike instances;
 B3 UWVK_ST_NOTPD: which step raises it for which pivot, that it stays in its
    instance (and in its half of a pair wave), sticky and clear.

Paths: dense (the literal kernels, set_dense_sigma), psp (one instance per
wave, the general kernel: set_pair(False), set_param_block(False)), pd
(set_pair(False): the parameter-decoupled kernel at 53 DOF), pair (the
default on an even batch).  The pd / pair choice is run_log's alone: the
single calls of all three PSP paths are k_psp_predict / k_psp_update, so they
run on dense and psp only.  Both layouts on psp and pair, both SO3 sides in B1
and B2.  Tolerances (tests/test_gpu_parity.py): means in the oracle's sigma
and covariances relative to sqrt(P_ii P_jj), 1e-9 for a single call and 1e-7
for a log.

Measured on an MI355X (max over instances, scenes, layouts and sides, sigma units):
 B1 single calls: dense 2.1e-11, psp 2.1e-11; run_log: dense 4.5e-10,
    psp / pd / pair 4.2e-10 (wide), far_step 3.6e-11; | |q| - 1 | <= 6.7e-16;
 B2 pair against the one-instance kernel: 1.5e-16 (means bitwise);
 B3 an undetected pivot (p >= 15) through run_log against the signed-weight
    restatement of the PSP steps (pose_scenes.signed_window): 1.5e-10; the
    variance factor -1.5 against the oracle: 3.7e-13.
Mutants of csrc/uwvk_psp_dev.hpp this suite was run against: so3_exp_psp's
threshold 0.0625 -> 1e9 fails 15 tests (far_step, 1.5e-8 off the unit norm;
up to big_step's 0.32 rad the series is still exact to 1e-17, only | |q| - 1 |
moves, to 1.2e-14); pchol's ok or-reduced over both halves fails 12 (the
healthy partner of instance j is flagged); so3_log_psp without its w < 0 flip
is the same function, bitwise: the series is even in the sign of q and the
fallback so3_log flips for itself, so no test can tell it apart."""
import functools

import numpy as np
import pytest

import oracle_ctypes as O
import pose_scenes as PS
from helpers import cov_err, state_err
from uwvk import engine, synth

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-9
TOL_LOG = 1e-7
TOL_PAIR = 1e-9  # pair against the one-instance kernel (tests/test_gpu_pair_units.py)
NOTPD = 0x1
B_WIDE = 8
B_NOTPD = 6

PATH_DOF = [("dense", 53), ("psp", 53), ("pd", 53), ("pair", 53), ("psp", 26), ("pair", 26)]
SINGLE_PATH_DOF = [("dense", 53), ("psp", 53), ("psp", 26)]  # the single-call kernels (see above)
SIDES = ["right", "left"]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not engine.device_available(0):
        pytest.fail("no gfx950 device / libuwvk.so not loadable: the HIP path is mandatory")


def handle(path, dof, B, right=True):
    g = engine.PoseUKFBatch(B, dof)
    g.set_so3_right(right)
    if path == "dense":
        g.set_dense_sigma(True)
    elif path == "psp":
        g.set_pair(False)
        g.set_param_block(False)
    elif path == "pd":
        g.set_pair(False)
    else:
        assert path == "pair" and B % 2 == 0
    return g


def check_path(g, path, dof):
    """the handle (with its state) is about to run the kernel the path names"""
    assert g.pair_active() == (1 if path == "pair" else 0)
    if path != "dense":  # (a dense handle leaves the decoupled kernels at its first step)
        assert g.param_block() == (1 if dof == 53 and path in ("pd", "pair") else 0)


def errors(x, P, xo, Po, dof):
    assert np.isfinite(x).all() and np.isfinite(P).all()
    np.testing.assert_array_equal(P, np.swapaxes(P, 1, 2))  # exactly symmetric
    qn = float(np.abs(np.linalg.norm(x[:, 3:7], axis=1) - 1.0).max())
    assert qn <= 1e-14, qn
    return float(state_err(x, xo, Po, dof).max()), float(cov_err(P, Po).max()), qn


# ---- B1. wide priors against the oracle ------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_ref(scene, dof, right):
    """(log, calls, ref): the oracle after the first predict, after each single
    call made from there, and after run_log over the scene; computed once."""
    log = PS.make(scene, B_WIDE, dof)
    ref = {}
    with O.so3_side(right):
        def predicted():
            o = PS.start(O.OraclePoseBatch(B_WIDE, dof), log)
            o.set_rotation_rate(log["gyro"][0])
            o.predict(log["dt"])
            return o
        ref["predict"] = predicted().get_state()
        calls = PS.single_calls(log, ref["predict"][0])
        for name, kind, mu, cov, extra, vo in calls:
            o = predicted()
            acc = o.update(kind, mu, cov, extra=extra, only_vel=vo)
            ref[name] = o.get_state() + (acc,)
        o = PS.start(O.OraclePoseBatch(B_WIDE, dof), log)
        counts = o.run_log(log)
        ref["run_log"] = o.get_state() + (counts,)
    return log, calls, ref


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("path,dof", SINGLE_PATH_DOF)
@pytest.mark.parametrize("scene", ["wide", "straddle", "big_step", "far_step"])
def test_wide_prior_single_calls(scene, path, dof, side):
    """predict, then every update kind from the predicted state (the prior at
    its widest for each), against the oracle: state, covariance, accept flags,
    status 0, P symmetric, |q| = 1."""
    right = side == "right"
    log, calls, ref = wide_ref(scene, dof, right)
    g = handle(path, dof, B_WIDE, right)

    def predicted():
        PS.start(g, log)
        g.set_rotation_rate(log["gyro"][0])
        g.predict(log["dt"])

    predicted()
    worst = list(errors(*g.get_state(), *ref["predict"], dof))
    assert max(worst[:2]) < TOL_STEP, ("predict", worst)
    for name, kind, mu, cov, extra, vo in calls:
        predicted()
        acc = g.update(kind, mu, cov, extra=extra, only_vel=vo)
        xo, Po, acc_o = ref[name]
        np.testing.assert_array_equal(acc, acc_o, err_msg=name)
        e = errors(*g.get_state(), xo, Po, dof)
        assert max(e[:2]) < TOL_STEP, (name, e)
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert not g.get_status().any(), name
    print("%s %s dof %d %s single calls: state %.3g cov %.3g |q|-1 %.3g" % ((scene, path, dof, side) + tuple(worst)))


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("path,dof", PATH_DOF)
@pytest.mark.parametrize("scene", ["wide", "straddle", "big_step", "far_step"])
def test_wide_prior_run_log(scene, path, dof, side):
    right = side == "right"
    log, _, ref = wide_ref(scene, dof, right)
    g = PS.start(handle(path, dof, B_WIDE, right), log)
    check_path(g, path, dof)
    acc = engine.DeviceBuffer(np.zeros((B_WIDE, 4), np.uint32))
    g.run_log(g.upload_log(log), accept_counts=acc)
    xo, Po, counts = ref["run_log"]
    np.testing.assert_array_equal(acc.read(np.uint32, (B_WIDE, 4)), counts)
    assert counts[:, 0].all()  # the DVL epoch ran
    assert not g.get_status().any()
    e = errors(*g.get_state(), xo, Po, dof)
    print("%s %s dof %d %s run_log: state %.3g cov %.3g |q|-1 %.3g" % ((scene, path, dof, side) + e))
    assert max(e[:2]) < TOL_LOG, e


# ---- B2. unlike halves of a pair ------------------------------------------------
NAMES = ("state", "covariance", "accept counts", "status", "rotation rate")


def run_mixed(parts, pair, dof, right):
    log = PS.mix(parts)
    g = handle("pair" if pair else "pd", dof, len(parts), right)
    PS.start(g, log)
    assert g.pair_active() == (1 if pair else 0)
    acc = engine.DeviceBuffer(np.zeros((len(parts), 4), np.uint32))
    g.run_log(g.upload_log(log), accept_counts=acc)
    x, P = g.get_state()
    return x, P, acc.read(np.uint32, (len(parts), 4)), g.get_status(), g.get_rotation_rate()


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("dof", [53, 26])
def test_pair_unlike_halves(dof, side):
    """N, N' narrow and W, W' wide instances (W' from -q0) in batches of 4 on the
    pair kernel: unit u holds slots 2u (lower half of the wave) and 2u + 1
    (upper half).  An instance that keeps its slot between two runs and
    changes only its partner comes out bitwise equal:
      [N, W, W', N'] and [N, N', W', W]: N in slot 0 (narrow, lower half; its
                     partner wide, then narrow), W' in slot 2 (wide, lower half);
      [N, W, W', N'] and [W', W, N, N']: W in slot 1 (wide, upper half), N' in
                     slot 3 (narrow, upper half).
    [W, N, N', W'] is the mirror arrangement.  Every instance of every run is
    within 1e-9 sigma of the one-instance kernel on the same batch."""
    right = side == "right"
    n, w = PS.make("narrow", 4, dof), PS.make("wide", 4, dof)
    N, N2, W, W2 = (n, 0), (n, 1), (w, 2), (w, 3)
    assert (w["rot0"][3] == -n["rot0"][3]).all() and w["rot_cov"][2, 0, 0] > 0.08
    batches = dict(a=[N, W, W2, N2], b=[N, N2, W2, W], c=[W, N, N2, W2], d=[W2, W, N, N2])
    got = {k: run_mixed(v, True, dof, right) for k, v in batches.items()}
    for k, v in batches.items():
        ref = run_mixed(v, False, dof, right)
        np.testing.assert_array_equal(got[k][2], ref[2])
        assert not got[k][3].any() and not ref[3].any()
        es, ec = state_err(got[k][0], ref[0], ref[1], dof), cov_err(got[k][1], ref[1])
        print("dof %d %s batch %s pair vs single: state %.3g cov %.3g" % (dof, side, k, es.max(), ec.max()))
        assert es.max() < TOL_PAIR and ec.max() < TOL_PAIR
        assert got[k][2][:, 0].all()
    for first, second, slots in (("a", "b", (0, 2)), ("a", "d", (1, 3))):
        for s in slots:
            assert batches[first][s] is batches[second][s] and batches[first][s ^ 1] is not batches[second][s ^ 1]
            for name, u, v in zip(NAMES, got[first], got[second]):
                np.testing.assert_array_equal(u[s], v[s], err_msg="%s slot %d of %s / %s" % (name, s, first, second))


# ---- B3. not positive definite ----------------------------------------------------
ALL = 1 << 20
# The first non-positive pivot p of Sigma raises UWVK_ST_NOTPD in an op iff
# p < EXPECT_FLAG[path][op].  From the code: the literal kernels factor all of
# Sigma at the start of every step (chol_lds, uwvk_pose_dev.hpp); a PSP step
# factors the leading k tangent DOFs only (pchol<DOF, K>: PG::KP = 15 for the
# predict, HM::K of PAcc / PVel / PWater = 6, PPressure = 19, PEffVO = 9, PXY /
# PZ = 0, uwvk_psp_dev.hpp) and psp_update_eff all of it (eff_chol); run_log's
# first step is the predict, and with p >= 15 no later step of the window meets
# a non-positive pivot below its own k (tests/test_pose_scenes.py).
_PSP = dict(PS.PSP_K, efforts=ALL, run_log=PS.PSP_K["predict"])
EXPECT_FLAG = dict(dense={op: ALL for op in _PSP}, psp=_PSP, pd=_PSP, pair=_PSP)
OPS = sorted(_PSP)


@functools.lru_cache(maxsize=None)
def healthy(dof):
    log, x, P = PS.healthy_state(B_NOTPD, dof)
    calls = {c[0]: c for c in PS.single_calls(log, x)}
    return log, x, P, calls


def init_state(g, dof, x, P, log):
    g.init_from_state(x, P, *PS.state_handles(dof))
    g.set_process_noise_from_config(synth.default_pose_config(), log["dt"])
    g.set_rotation_rate(log["gyro"][PS.HEALTHY_EPOCHS])


def snap(g, extra=None):
    x, P = g.get_state()
    return x, P, g.get_status(), g.get_rotation_rate(), np.zeros(0) if extra is None else np.asarray(extra)


def same(a, b, rows):
    for u, v in zip(a, b):
        if u.ndim and len(u) == len(a[0]):
            np.testing.assert_array_equal(u[rows], v[rows])


def apply_op(g, op, dof, dlog=None):
    """the op on the handle -> what it reports per instance (accept flags / counts)"""
    log, x, P, calls = healthy(dof)
    if op == "predict":
        g.predict(log["dt"])
        return None
    if op == "run_log":
        acc = engine.DeviceBuffer(np.zeros((B_NOTPD, 4), np.uint32))
        g.run_log(dlog, 0, PS.NOTPD_WINDOW, accept_counts=acc)
        return acc.read(np.uint32, (B_NOTPD, 4))
    _, kind, mu, cov, extra, vo = calls[op]
    return g.update(kind, mu, cov, extra=extra, only_vel=vo)  # raises on any code but UWVK_OK


def masked_clean_call(g, dof, j):
    """a z update with instance j masked out: a clean call that does not touch j"""
    log, x, P, calls = healthy(dof)
    _, kind, mu, cov, extra, vo = calls["z"]
    g.update(kind, mu, cov, mask=(np.arange(B_NOTPD) != j).astype(np.uint8))


def notpd_contract(bad, good, path, dof, op, j, name):
    """bad, good: two handles of the path, re-initialised here"""
    log, x, P, calls = healthy(dof)
    build, p, sign = PS.indefinite_scenes(dof)[name]
    flag = p < EXPECT_FLAG[path][op]
    Pj = P.copy()
    Pj[j] = build(P[j])
    others = np.arange(B_NOTPD) != j
    only_j = np.where(others, 0, NOTPD).astype(np.uint32)
    what = "%s dof %d %s j %d %s (pivot %d)" % (path, dof, op, j, name, p)
    init_state(bad, dof, x, Pj, log)
    init_state(good, dof, x, P, log)
    if op == "run_log":
        check_path(bad, path, dof)  # P_bad keeps the handle PD- and pair-eligible
    dlog = bad.upload_log(log) if op == "run_log" else None
    before = snap(bad)
    same(before, snap(good), others)
    assert not before[2].any()
    after = snap(bad, apply_op(bad, op, dof, dlog))
    ref = snap(good, apply_op(good, op, dof, dlog))
    np.testing.assert_array_equal(after[2], only_j if flag else 0 * only_j, err_msg=what)  # exactly NOTPD, or 0
    same(after, ref, others)  # bitwise beside a valid Sigma: state, covariance, status 0, rate, accepts
    assert not ref[2].any()
    accepted = np.ones(B_NOTPD, bool) if ref[4].ndim != 1 or not ref[4].size else ref[4].astype(bool)
    changed = (after[1] != before[1]).any(axis=(1, 2))
    np.testing.assert_array_equal(changed[others], accepted[others], err_msg=what)
    if not flag:  # the documented non-detection: the PSP formulas are defined, the output finite
        assert path != "dense"
        assert np.isfinite(after[0][j]).all() and np.isfinite(after[1][j]).all(), what
    else:
        # sticky: a clean call that leaves j alone does not clear it; clear reads and resets it
        masked_clean_call(bad, dof, j)
        np.testing.assert_array_equal(bad.get_status(), only_j, err_msg=what)
        np.testing.assert_array_equal(bad.get_status(clear=True), only_j)
        assert not bad.get_status().any()
    # re-initialised with the healthy state the handle is the healthy handle: nothing raised anew
    init_state(bad, dof, x, P, log)
    again = snap(bad, apply_op(bad, op, dof, dlog))
    same(again, ref, slice(None))
    assert np.isfinite(again[0]).all() and np.isfinite(again[1]).all() and not again[2].any()
    return after, p, flag


def scene_names(dof, op, path):
    names = [n for n, (_, p, _) in PS.indefinite_scenes(dof).items()
             if p in PS.PIVOTS[dof] or n.startswith("zero")]
    if op == "efforts" and path != "dense" and dof == 53:  # the edges of eff_chol's panels
        names += ["neg%d" % p for p in PS.EFF_PANEL_PIVOTS if "neg%d" % p not in names]
    return sorted(names)


@pytest.mark.parametrize("j", [2, 3])
@pytest.mark.parametrize("path,dof", SINGLE_PATH_DOF)
@pytest.mark.parametrize("op", [op for op in OPS if op != "run_log"])
def test_notpd_single_calls(op, path, dof, j):
    """One indefinite (or singular) Sigma among six instances, every pivot
    scene of pose_scenes.indefinite_scenes: the call returns UWVK_OK, instance
    j's status is exactly what EXPECT_FLAG says, the others are bitwise the
    all-healthy handle's."""
    bad, good = handle(path, dof, B_NOTPD), handle(path, dof, B_NOTPD)
    for name in scene_names(dof, op, path):
        notpd_contract(bad, good, path, dof, op, j, name)


@pytest.mark.parametrize("j", [2, 3])  # the lower and the upper half of pair unit 1
@pytest.mark.parametrize("path,dof", PATH_DOF)
def test_notpd_run_log(path, dof, j):
    """run_log over four epochs (four predicts and accelerations, the DVL
    epoch).  A pivot below 15 is raised by the first predict and the instance
    runs on as NaN beside its partner; from 15 on nothing is raised and the
    result is the one the PSP formulas define (the signed-weight restatement,
    pose_scenes.signed_window), in the healthy state's sigma."""
    log, x, P, _ = healthy(dof)
    worst = 0.0
    bad, good = handle(path, dof, B_NOTPD), handle(path, dof, B_NOTPD)
    for name in scene_names(dof, "run_log", path):
        after, p, flag = notpd_contract(bad, good, path, dof, "run_log", j, name)
        if not flag:
            build = PS.indefinite_scenes(dof)[name][0]
            mu, Pt = PS.signed_window(log, x[j], build(P[j]), j, dof)
            es = state_err(after[0][j:j + 1], mu[None], P[j:j + 1], dof).max()
            sd = np.sqrt(np.diag(P[j]))
            ec = (np.abs(after[1][j] - Pt) / np.outer(sd, sd)).max()
            worst = max(worst, es, ec)
            assert es < TOL_LOG and ec < TOL_LOG, (name, es, ec)
    print("%s dof %d j %d undetected pivots against the restatement: %.3g" % (path, dof, j, worst))


@pytest.mark.parametrize("j", [2, 3])
@pytest.mark.parametrize("path,dof", PATH_DOF)
def test_notpd_run_log_with_fixes(path, dof, j):
    """The same window with one XY, one Z and one GEO fix (uwvk_pose_run_log_fixes),
    pivot 0 in instance j: raised by the epoch kernel's first predict; the
    others bitwise the healthy run's, fix accept counts included."""
    from test_gpu_fixes import GEO, XY, Z, make_fixes
    log, x, P, _ = healthy(dof)
    fx = make_fixes(log, [(0, XY), (2, Z), (3, GEO)])
    Pj = P.copy()
    Pj[j] = PS.negative_pivot(P[j], 0)
    others = np.arange(B_NOTPD) != j
    out = []
    for Pi in (Pj, P):
        g = handle(path, dof, B_NOTPD)
        init_state(g, dof, x, Pi, log)
        check_path(g, path, dof)
        dfx = g.upload_fixes(fx, counts=True)
        acc = engine.DeviceBuffer(np.zeros((B_NOTPD, 4), np.uint32))
        g.run_log(g.upload_log(log), 0, PS.NOTPD_WINDOW, accept_counts=acc, fixes=dfx)
        out.append(snap(g) + (acc.read(np.uint32, (B_NOTPD, 4)), dfx.accept_counts(g.stream)))
    bad, good = out
    np.testing.assert_array_equal(bad[2], np.where(others, 0, NOTPD))
    assert not good[2].any() and good[6].all() and good[5][:, 0].all()  # every fix and the DVL sample applied
    same(bad, good, others)


@pytest.mark.parametrize("j", [2, 3])
@pytest.mark.parametrize("path,dof", PATH_DOF)
@pytest.mark.parametrize("factor", PS.Z_VARIANCE_FACTORS)
def test_negative_z_variance_then_predict(factor, path, dof, j):
    """Sigma turns indefinite at run time: a z update whose variance for
    instance j is factor * P[2, 2], then a predict (dense / psp: the single
    call; pd / pair: run_log over one epoch, the epoch kernel's predict).
    -0.5: Sigma - C K^T has a negative pivot at index 2.  The oracle returns
          UWVK_ENOTPD from the update already (its re-spread factors the
          reduced Sigma) and again from the predict
          (tests/test_pose_scenes.py::test_negative_z_variance); here the z
          update factors nothing of the reduced Sigma (k = 0; the literal
          kernel's exact apply_delta has no second factorisation), and the
          predict raises UWVK_ST_NOTPD: by the end of the two calls j carries
          it on every path, the others are bitwise the healthy run's.
    -1.5: S < 0 and Sigma - C K^T GROWS (stays positive definite): the oracle
          returns UWVK_OK twice, nothing is raised, and every instance, j
          included, agrees with the oracle."""
    log, x, P, calls = healthy(dof)
    others = np.arange(B_NOTPD) != j
    z = calls["z"][2]
    R = np.full((B_NOTPD, 1, 1), 0.01)
    Rj = R.copy()
    Rj[j] = factor * P[j, 2, 2]
    by_log = path in ("pd", "pair")
    out = []
    for Ri in (Rj, R):
        g = handle(path, dof, B_NOTPD)
        init_state(g, dof, x, P, log)
        g.update("z", z, Ri)
        mid = g.get_status()
        if by_log:
            check_path(g, path, dof)
            g.run_log(g.upload_log(log), PS.HEALTHY_EPOCHS, 1)
        else:
            g.predict(log["dt"])
        out.append(snap(g) + (mid,))
    bad, good = out
    assert not good[2].any() and not good[5].any()
    same(bad, good, others)
    if PS.z_variance_breaks_sigma(factor):
        np.testing.assert_array_equal(bad[2], np.where(others, 0, NOTPD))
        return
    assert not bad[2].any() and not bad[5].any()
    o = O.OraclePoseBatch(B_NOTPD, dof)
    init_state(o, dof, x, P, log)
    o.update("z", z, Rj)
    if by_log:
        o.run_log(log, PS.HEALTHY_EPOCHS, 1)
    else:
        o.predict(log["dt"])
    e = errors(bad[0], bad[1], *o.get_state(), dof)
    print("%s dof %d j %d factor %g against the oracle: state %.3g cov %.3g" % (path, dof, j, factor, e[0], e[1]))
    assert max(e[:2]) < TOL_STEP


def test_init_is_a_new_filter():
    """uwvk_pose_init_from_state makes every instance a new filter
    (include/uwvk.h): the status words are zero after it, a raised
    UWVK_ST_NOTPD included."""
    log, x, P, _ = healthy(53)
    Pj = P.copy()
    Pj[2] = PS.negative_pivot(P[2], 0)
    g = handle("psp", 53, B_NOTPD)
    init_state(g, 53, x, Pj, log)
    g.predict(log["dt"])
    assert g.get_status().tolist() == [0, 0, NOTPD, 0, 0, 0]
    init_state(g, 53, x, P, log)
    assert not g.get_status().any()
