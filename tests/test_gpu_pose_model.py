"""The PoseUKF kernels on a general vehicle model, a mounted IMU and a tilted
attitude (the scenes of tests/pose_model_scenes.py, each valid on the CPU
first: tests/test_pose_model_scenes.py), against the oracle.

Every other PoseUKF test runs on synth.default_uwv() with the IMU at the body
origin: diagonal matrices, W = B, the centres on the z axis, a level truth.
There M, M^T and diag(M) are one matrix, the 3x3 (surge, sway, yaw) blocks the
state overlays are symmetric, the restoring term nearly vanishes and the lever
arm terms are multiplied by zero.  Here none of that holds:

 1 init_from_config with a mounting (lever arm and rotation): state, Sigma and
   rotation rate against the oracle, then a predict and an acceleration update
   (the non-diagonal bias blocks of Sigma and Q through a kernel);
 2 the two BodyEfforts forms as single calls from init_from_state(tilted_state);
 3 full -> predict -> velocity-only: the second reads the blocks the first left;
 4 run_log over model_log on every path, and in two calls on the pair path;
 5 (tests/test_gpu_efforts.py) PSP against the literal kernels at a full grid;
 6 the model belongs to the init, not to the handle.

Paths and tolerances: tests/test_gpu_pose_edges.py (dense, psp, pd, pair;
1e-9 for a single call, 1e-7 for a log, means in the oracle's sigma and
covariances relative to sqrt(P_ii P_jj)); accept flags and counts bitwise.

Measured on an MI355X (max over instances, layouts and sides; mean in sigma /
covariance):
 1 init with the mounting: dense and psp 0 / 6.6e-17, rotation rate within
   1e-16; the predict and acceleration update after it 2.2e-13 / 1.7e-11;
 2 single full call: dense 1.8e-13 / 5.3e-13, psp 1.9e-13 / 8.3e-13; single
   velocity-only call: dense 1.8e-13 / 3.1e-13, psp 1.8e-13 / 3.4e-13;
 3 the velocity-only call after full and predict: dense 7.0e-13 / 5.9e-13,
   psp 7.0e-13 / 9.2e-13;
 4 model_log: dense 1.3e-8 / 3.4e-10, psp, pd and pair 1.2e-8 / 3.2e-10 (the
   left side at 53 DOF; 2.8e-9 / 6.2e-11 on the right side, 1.6e-9 at 26 DOF);
   | |q| - 1 | <= 6.7e-15; in two calls bitwise.
Nothing was found wrong: every feature / path combination agrees with the
oracle at the project's tolerances.

Mutants of csrc/ this module and tests/test_gpu_efforts.py were run against
(one at a time, 41 tests here, 18 there):
 (a) Efforts6::m reads the base table transposed (c * 6 + r): fails 30 here
     (all 18 of test_efforts_calls, all 12 of test_model_log);
 (b) blk_index row-major (3 * a + b): fails 28 (16 + 12; the single full call
     at 26 DOF has no blocks to read);
 (c) cog and cob swapped in the restoring moment: fails 30 (18 + 12);
 (d) the lever arm term dropped from HConstrain's body velocity: fails 24 (the
     12 cases of test_efforts_calls with a velocity-only call, 12 of test_model_log);
 (e) host::model_blocks row-major: fails 12 (the 6 single velocity-only calls,
     which read the blocks the init stored, the 2 sequences and the 4 model_log
     cases at 26 DOF; at 53 DOF the first full update overwrites the stored blocks).
tests/test_gpu_efforts.py passes under every one of them, its general-model
grid included: it compares the PSP kernel with the literal one, and both share
Efforts6, the measurement functors and the host init.  Only the oracle sees them."""
import functools

import numpy as np
import pytest

import oracle_ctypes as O
import pose_model_scenes as MS
from test_gpu_pose_edges import PATH_DOF, SIDES, SINGLE_PATH_DOF, TOL_LOG, TOL_STEP, check_path, errors, handle
from uwvk import engine, synth

pytestmark = pytest.mark.gpu

B = 6  # three pair waves, every instance unlike
TOL_INIT = 1e-15  # tests/test_gpu_parity.py::test_init_and_predict
FIRST_EFFORTS = MS.EFFORTS_EPOCHS[0]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not engine.device_available(0):
        pytest.fail("no gfx950 device / libuwvk.so not loadable: the HIP path is mandatory")


def report(what, path, dof, side, e):
    print("%s %s dof %d %s: state %.3g cov %.3g |q|-1 %.3g" % ((what, path, dof, side) + tuple(e)))


# ---- 1. init with a mounting ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def init_ref(dof, right):
    log = MS.model_log(B, 4, dof)
    with O.so3_side(right):
        o = MS.start_log(O.OraclePoseBatch(B, dof), log)
        ref = dict(init=o.get_state(), rate=o.get_rotation_rate())
        o.set_rotation_rate(log["gyro"][0])
        o.predict(log["dt"])
        o.update("acceleration", log["acc"][0], log["acc_cov"])
        ref["step"] = o.get_state()
    return log, ref


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("path,dof", SINGLE_PATH_DOF)
def test_init_with_mounting(path, dof, side):
    right = side == "right"
    log, ref = init_ref(dof, right)
    g = MS.start_log(handle(path, dof, B, right), log)
    e = errors(*g.get_state(), *ref["init"], dof)
    report("init with the mounting", path, dof, side, e)
    assert max(e[:2]) < TOL_INIT, e
    np.testing.assert_allclose(g.get_rotation_rate(), ref["rate"], rtol=0, atol=1e-16)
    assert np.abs(ref["rate"]).min() > 1e-3  # minus the turned gyro bias offset
    g.set_rotation_rate(log["gyro"][0])
    g.predict(log["dt"])
    np.testing.assert_array_equal(g.update("acceleration", log["acc"][0], log["acc_cov"]), np.ones(B, np.uint8))
    e = errors(*g.get_state(), *ref["step"], dof)
    report("predict + acceleration after it", path, dof, side, e)
    assert max(e[:2]) < TOL_STEP, e
    assert not g.get_status().any()


# ---- 2., 3. the efforts calls ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def calls_ref(dof, right):
    """{name: [(x, P) after the first predict, then (x, P, accept flags) after
    each call of the scene (a predict before every call but the first)]}"""
    calls = MS.efforts_calls(B)
    ref = {}
    with O.so3_side(right):
        for name in ("full", "vel", "sequence"):
            o = MS.start_state(O.OraclePoseBatch(B, dof), B, dof)
            o.predict(MS.DT)
            out = [o.get_state()]
            for n, (z, R, vo) in enumerate(calls[name] if name == "sequence" else [calls[name]]):
                if n:
                    o.predict(MS.DT)
                acc = o.update("efforts", z, R, only_vel=vo)
                out.append(o.get_state() + (acc,))
            ref[name] = out
    return calls, ref


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("path,dof", SINGLE_PATH_DOF)
@pytest.mark.parametrize("name", ["full", "vel", "sequence"])
def test_efforts_calls(name, path, dof, side):
    """init_from_state(tilted_state, general_uwv, general_param), the rate, a
    predict, then the call (sequence: full, predict, velocity-only), checked
    after the predict and after every call: state, covariance, accept flags,
    status 0, P exactly symmetric, |q| = 1."""
    right = side == "right"
    calls, ref = calls_ref(dof, right)
    g = MS.start_state(handle(path, dof, B, right), B, dof)
    g.predict(MS.DT)
    e = errors(*g.get_state(), *ref[name][0], dof)
    assert max(e[:2]) < TOL_STEP, ("predict", e)
    for n, (z, R, vo) in enumerate(calls[name] if name == "sequence" else [calls[name]]):
        if n:
            g.predict(MS.DT)
        acc = g.update("efforts", z, R, only_vel=vo)
        xo, Po, acc_o = ref[name][1 + n]
        np.testing.assert_array_equal(acc, acc_o)
        e = errors(*g.get_state(), xo, Po, dof)
        report("efforts %s call %d (only_vel %d)" % (name, n, vo), path, dof, side, e)
        assert max(e[:2]) < TOL_STEP, (name, n, e)
        assert not g.get_status().any()


# ---- 4. run_log over model_log -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def log_ref(dof, right):
    log = MS.model_log(B, dof=dof)
    with O.so3_side(right):
        o = MS.start_log(O.OraclePoseBatch(B, dof), log)
        counts = o.run_log(log)
        ref = o.get_state() + (counts,)
    return log, ref


def run_model_log(path, dof, right, cuts=()):
    log, _ = log_ref(dof, right)
    g = MS.start_log(handle(path, dof, B, right), log)
    check_path(g, path, dof)
    acc = engine.DeviceBuffer(np.zeros((B, 4), np.uint32))
    dlog = g.upload_log(log)
    edges = [0] + list(cuts) + [log["epochs"]]
    for a, b in zip(edges[:-1], edges[1:]):
        g.run_log(dlog, a, b - a, accept_counts=acc)
    return g, acc.read(np.uint32, (B, 4))


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("path,dof", PATH_DOF)
def test_model_log(path, dof, side):
    right = side == "right"
    _, (xo, Po, counts) = log_ref(dof, right)
    g, acc = run_model_log(path, dof, right)
    np.testing.assert_array_equal(acc, counts)
    assert (counts[:, 0] == 2).all() and (counts[:, 1] == 2).all() and (counts[:, 3] == 5).all()
    assert not g.get_status().any()
    if dof == 53 and path in ("pd", "pair"):
        assert g.param_block() == 0  # the full update couples the block (tests/test_gpu_pd.py)
    e = errors(*g.get_state(), xo, Po, dof)
    report("model_log", path, dof, side, e)
    assert max(e[:2]) < TOL_LOG, e


@pytest.mark.parametrize("dof", [53, 26])
def test_model_log_in_two_calls(dof):
    """The same log cut right after the first efforts epoch (the second call
    starts from the blocks the full update left, and at 53 DOF from a coupled
    parameter block): bitwise the single call, on the pair path."""
    whole, acc_w = run_model_log("pair", dof, True)
    parts, acc_p = run_model_log("pair", dof, True, cuts=(FIRST_EFFORTS + 1,))
    np.testing.assert_array_equal(acc_p, acc_w)
    for u, v in zip(whole.get_state() + (whole.get_status(), whole.get_rotation_rate()),
                    parts.get_state() + (parts.get_status(), parts.get_rotation_rate())):
        np.testing.assert_array_equal(u, v)


# ---- 6. the model belongs to the init --------------------------------------------
@pytest.mark.parametrize("path,dof", SINGLE_PATH_DOF)
def test_model_belongs_to_the_init(path, dof):
    """One handle: the general model and a full efforts update, then
    init_from_config with the default model and a velocity-only (the stored
    blocks), a predict and a full call (the base table): bitwise a fresh
    handle's.  The base table is global memory read by scalar loads through
    the constant address space: a stale copy would show here."""
    calls = MS.efforts_calls(B)
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    log = synth.make_pose_log(B, 2, "C3", dof=dof)

    def default_run(g):
        g.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
        g.set_process_noise_from_config(cfg, log["dt"])
        for e, (z, R, vo) in enumerate((calls["vel"], calls["full"])):
            g.set_rotation_rate(log["gyro"][e] + MS.RATE)
            g.predict(log["dt"])
            g.update("efforts", z, R, only_vel=vo)
        return g.get_state() + (g.get_status(), g.get_rotation_rate())

    used = MS.start_state(handle(path, dof, B), B, dof)
    used.predict(MS.DT)
    used.update("efforts", *calls["full"][:2], only_vel=0)
    general = used.get_state()
    got, fresh = default_run(used), default_run(handle(path, dof, B))
    for u, v in zip(got, fresh):
        np.testing.assert_array_equal(u, v)
    assert not fresh[2].any() and np.isfinite(fresh[0]).all() and np.isfinite(fresh[1]).all()
    assert not np.array_equal(general[0], fresh[0])
