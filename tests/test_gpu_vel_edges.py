"""Edge and equivalence tests of the VelocityUKF kernels (csrc/uwvk_vel.hip)
through the C ABI, fp64, on the scenes of tests/vel_scenes.py (each valid on
the CPU first: tests/test_vel_scenes.py):

 1. every scene against the oracle on the three layouts and at the batch sizes
    that leave the 16-lane-row kernel one live row, a partial wave, one wave,
    one wave plus a row, several waves plus a row;
 2. the layouts against each other;
 3. an instance's result does not depend on its slot or on the batch (bitwise
    against a batch of one), B - 1, the instance the dead rows copy, included;
 4. a non-finite sample in one instance's device log leaves the others alone;
 5. the not-positive-definite path and the status word (uwvk_vel_get_status);
 6. the single calls: shared and per-instance covariances, masks, NaN, errors;
 7. run_log against the loop of single calls;
 8. ranges of a log compose bitwise, count = 0 is a no-op;
 9. the 4,096-epoch launch boundary;
10. the gyro and efforts run_log leaves in the handle;
11. the automatic layout choice at its threshold.

Tolerances (tests/test_gpu_parity.py): means in the oracle's sigma and
covariances relative to sqrt(P_ii P_jj), 1e-9 for single steps and 1e-7 for
logs; the motion-model state 1e-9 absolute.  Layouts: 0 one filter per lane
(k_vel_epoch), 1 one per 16-lane row (k_vel_epoch_g<16>), 2 the diagnostic
with a shadow row that stores nothing (k_vel_epoch_g<32>)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_ctypes as O
import vel_scenes as VS
from helpers import cov_err, pivots
from uwvk import engine, synth

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-9
TOL_LOG = 1e-7
TOL_MODEL = 1e-9
NOTPD = 0x1
LAYOUTS = [0, 1, 2]
GROUPS_MAX_BATCH = 30720  # kVelGroupsMaxBatch: the largest batch the automatic choice gives to layout 1
EINVAL, ENAN, ENOMODEL, ENOTINIT = 1, 2, 4, 7


@functools.lru_cache(maxsize=None)
def scene(name, B, epochs=None):
    return VS.SCENES[name](B) if epochs is None else VS.SCENES[name](B, epochs=epochs)


@functools.lru_cache(maxsize=None)
def oracle_final(name, B):
    """(x, P, model) of the oracle after the whole log, computed once"""
    log = scene(name, B)
    o = VS.start(O.OracleVelBatch(B), log)
    o.run_log(log)
    return o.get_state(model=True)


def handle(log, layout=None, P0=None):
    g = VS.start(engine.VelocityUKFBatch(log["batch"]), log, P0)
    if layout is not None:
        g.set_lane_groups(layout)
    return g


def run(log, layout, ranges=None, P0=None):
    """a fresh handle after run_log over `ranges` (default: the whole log) -> (x, P, model, status)"""
    g = handle(log, layout, P0)
    dlog = g.upload_log(log)
    for first, count in ranges or [(0, log["epochs"])]:
        g.run_log(dlog, first, count)
    return snap(g)


def snap(g):
    return (*g.get_state(model=True), g.get_status())


def same(a, b, rows=slice(None), rows_b=None):
    """(x, P, model[, status]) bitwise equal on `rows`"""
    rows_b = rows if rows_b is None else rows_b
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u[rows], v[rows_b])


def errors(got, ref):
    (xg, Pg, mg), (xo, Po, mo) = got[:3], ref[:3]
    assert np.isfinite(xg).all() and np.isfinite(Pg).all() and np.isfinite(mg).all()
    sd = np.sqrt(np.diagonal(Po, axis1=1, axis2=2))
    return float(np.max(np.abs(xg - xo) / sd)), float(cov_err(Pg, Po).max()), float(np.max(np.abs(mg - mo)))


def close(got, ref, tol, what=""):
    es, ec, em = errors(got, ref)
    print("%s state %.3g cov %.3g model %.3g" % (what, es, ec, em))
    assert es < tol and ec < tol and em < TOL_MODEL, (what, es, ec, em)


# ---- 1. scenes against the oracle -----------------------------------------
@pytest.mark.parametrize("B", [1, 3, 4, 5, 13])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(VS.SCENES))
def test_scene_against_oracle(name, layout, B):
    got = run(scene(name, B), layout)
    assert not got[3].any(), got[3]
    close(got, oracle_final(name, B), TOL_LOG, "%s layout %d B %d" % (name, layout, B))


# ---- 2. layouts agree ------------------------------------------------------
def test_layouts_agree():
    """Layouts 1 and 2 run one instruction stream (the shadow row stores
    nothing): bitwise.  The lane-per-filter kernel sums in another order."""
    log = scene("tilted", 13)
    r0, r1, r2 = (run(log, layout) for layout in LAYOUTS)
    same(r1, r2)
    close(r0, r1, TOL_LOG, "layout 0 against 1")
    assert (r0[1] != r1[1]).any()  # the two kernels do differ in rounding: test_auto_layout relies on it


# ---- 3. slot and batch independence ---------------------------------------
@functools.lru_cache(maxsize=None)
def alone(layout, k):
    """instance k of the mixed-spread scene in a batch of one"""
    return run(VS.take(scene("mixed", 70), k), layout)


@pytest.mark.parametrize("B", [4, 5, 13, 65, 70])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_slot_and_batch_independence(layout, B):
    """On the scene whose neighbours leave the mean loop after different pass
    counts.  Instance k of the scene is the same whatever the batch (vel_scenes),
    so the batch of B is the first B columns of the 70."""
    got = run(VS.take(scene("mixed", 70), np.arange(B)), layout)
    assert not got[3].any()
    for k in sorted({0, 1, 2, B // 2, 63, 64, B - 2, B - 1} & set(range(B))):
        same(got, alone(layout, k), slice(k, k + 1), slice(0, 1))


# ---- 4. a non-finite sample in the device log -----------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["dvl_nan", "pressure_inf"])
def test_nonfinite_sample_stays_in_its_instance(kind, layout):
    """run_log does not screen its samples (include/uwvk.h): the bad one enters
    instance j, whose next factorisation raises UWVK_ST_NOTPD; nothing is
    asserted about j's state."""
    B, j = 9, 5  # the second row of the second wave of the row kernel
    clean = scene("dense", B)
    log = dict(clean)
    if kind == "dvl_nan":
        e = 5  # of 12: DVL only; six epochs follow
        log["dvl"] = clean["dvl"].copy()
        log["dvl"][clean["dvl_index"][e], j, 1] = np.nan
    else:
        e = 6  # pressure (and DVL)
        log["pressure"] = clean["pressure"].copy()
        log["pressure"][clean["pressure_index"][e], j] = np.inf
    assert clean["flags"][e] and e + 2 < clean["epochs"]
    ref, got = run(clean, layout), run(log, layout)
    others = np.arange(B) != j
    assert not ref[3].any()
    same(got, ref, others)  # status included: zero
    assert got[3][j] != 0


# ---- 5. NOTPD and the status word -----------------------------------------
def _op(name):
    def predict(g, log, dlog):
        g.predict(log["dt"])

    def dvl(g, log, dlog):
        g.update_dvl(log["dvl"][0], log["dvl_cov"])

    def pressure(g, log, dlog):
        g.update_pressure(log["pressure"][0], log["pressure_cov"])

    def run_log(g, log, dlog):
        g.run_log(dlog, 0, 7)  # predicts, a pressure and a DVL update
    return dict(predict=predict, update_dvl=dvl, update_pressure=pressure, run_log_0=run_log, run_log_1=run_log)[name]


@pytest.mark.parametrize("pivot", ["leading", "last"])
@pytest.mark.parametrize("op", ["predict", "update_dvl", "update_pressure", "run_log_0", "run_log_1"])
def test_notpd(op, pivot):
    """one finite, symmetric, indefinite Sigma among 9 instances (full P0s)"""
    B, j = 9, 5
    log = scene("tilted", B)
    P = log["P0"].copy()
    if pivot == "leading":
        P[j, 0, 0] = -0.01
        assert pivots(P[j])[0] < 0
    else:
        P[j, 3, 3] = -0.002
        d = pivots(P[j])
        assert (d[:3] > 0).all() and d[3] < 0
    layout = int(op[-1]) if op.startswith("run_log") else None
    bad, healthy = handle(log, layout, P), handle(log, layout)
    dlog = bad.upload_log(log)
    others = np.arange(B) != j
    only_j = np.where(others, 0, NOTPD).astype(np.uint32)
    before = snap(bad)
    same(before, snap(healthy), others)
    assert not before[3].any()
    for g in (bad, healthy):
        _op(op)(g, log, dlog)
    after = snap(bad)
    np.testing.assert_array_equal(after[3], only_j)  # exactly that instance
    same(after, snap(healthy), others)               # its neighbours: as beside a valid Sigma
    assert (after[1][others] != before[1][others]).any(axis=(1, 2)).all()
    assert not healthy.get_status().any()
    # sticky: instance j made valid again, a clean call, the bit is still there
    bad.init(log["x0"], log["P0"])
    _op(op)(bad, log, dlog)
    np.testing.assert_array_equal(bad.get_status(), only_j)
    np.testing.assert_array_equal(bad.get_status(clear=True), only_j)
    assert not bad.get_status().any()
    _op(op)(bad, log, dlog)  # and that call did not raise it anew
    assert not bad.get_status().any()
    assert np.isfinite(bad.get_state()[1]).all()


# ---- 6. single calls -------------------------------------------------------
def _both(fs, call):
    for f in fs:
        call(f)


@pytest.mark.parametrize("B", [1, 5, 65])
def test_single_calls(B):
    """The tilted scene's first epochs through the per-call API, against the
    oracle after every call; epoch 0 with the shared full covariances, 1 with
    per-instance covariances that all differ, 2 and 3 under masks."""
    log = scene("tilted", 65) if B == 65 else VS.take(scene("tilted", 65), np.arange(B))
    o, g = VS.start(O.OracleVelBatch(B), log), handle(log)
    rng = np.random.default_rng(5)
    A = rng.normal(0, 0.03, (B, 3, 3))
    dcov = A @ np.swapaxes(A, 1, 2) + log["dvl_cov"]
    pcov = rng.uniform(1e-3, 4e-3, (B, 1, 1))
    alternate = (np.arange(B) % 2 == 0).astype(np.uint8)  # both values in every 64-lane block
    one_off = (np.arange(B) != B // 2).astype(np.uint8) if B > 1 else alternate
    kw = [dict(shared_cov=log["dvl_cov"]), dict(cov=dcov), dict(cov=dcov, mask=alternate),
          dict(shared_cov=log["dvl_cov"], mask=one_off)]
    kp = [dict(shared_cov=log["pressure_cov"]), dict(cov=pcov), dict(shared_cov=log["pressure_cov"], mask=alternate),
          dict(cov=pcov, mask=one_off)]

    def check(what):
        close(snap(g), o.get_state(model=True), TOL_STEP, "B %d %s" % (B, what))

    check("start")
    for e in range(4):
        zd = log["dvl"][e] + 0.01 * e
        zp = log["pressure"][e] - 0.01 * e
        _both((o, g), lambda f: f.set_gyro(log["gyro"][e]))
        check("set_gyro %d" % e)
        _both((o, g), lambda f: f.set_efforts(log["efforts"][e]))
        _both((o, g), lambda f: f.predict(log["dt"]))
        check("predict %d" % e)
        for name, z, k in (("update_dvl", zd, kw[e]), ("update_pressure", zp, kp[e])):
            before = snap(g)
            _both((o, g), lambda f: getattr(f, name)(z, **k))
            after = snap(g)
            check("%s %d" % (name, e))
            live = k["mask"].astype(bool) if "mask" in k else np.ones(B, bool)
            same(after[:2], before[:2], ~live)  # masked out: (x, P) untouched
            assert (after[1][live] != before[1][live]).any(axis=(1, 2)).all()
    assert not g.get_status().any()

    # NaN: accepted in a masked-out row, UWVK_ENAN in a live one, which changes nothing
    for name, z, k in (("update_dvl", log["dvl"][4].copy(), kw[2]), ("update_pressure", log["pressure"][4].copy(), kp[2])):
        live = k["mask"].astype(bool)
        twin_g = handle(log)  # the same update without the NaN, from the same state
        x, P = g.get_state()
        twin_g.init(x, P)
        before = snap(g)
        bad = z.copy()
        bad[np.flatnonzero(live)[-1]] = np.nan
        with pytest.raises(engine.UWVKError) as err:
            getattr(g, name)(bad, **k)
        assert err.value.code == ENAN
        same(snap(g), before)
        if (~live).any():
            ok = z.copy()
            ok[np.flatnonzero(~live)[0]] = np.nan
            getattr(g, name)(ok, **k)
            getattr(twin_g, name)(z, **k)
            same(g.get_state(), twin_g.get_state())
    assert not g.get_status().any()


def test_single_call_errors():
    B = 5
    log = scene("tilted", B)
    L = engine.lib()
    st = np.zeros(B, np.uint32)
    stp = st.ctypes.data_as(C.c_void_p)
    g = engine.VelocityUKFBatch(B)
    assert L.uwvk_vel_get_status(None, stp, 0) == EINVAL
    assert L.uwvk_vel_get_status(g.h, None, 0) == EINVAL
    assert L.uwvk_vel_get_status(g.h, stp, 1) == 0 and not st.any()  # readable from creation on
    z, R = log["dvl"][0], log["dvl_cov"]

    def code(call):
        with pytest.raises(engine.UWVKError) as err:
            call()
        return err.value.code

    assert code(lambda: g.update_dvl(z, R)) == ENOTINIT
    assert code(lambda: g.update_pressure(log["pressure"][0], 1e-3)) == ENOTINIT
    assert code(lambda: g.setup_motion_model(VS.uwv(log))) == ENOTINIT
    g.init(log["x0"], log["P0"])
    assert code(lambda: g.predict(log["dt"])) == ENOMODEL
    dlog = g.upload_log(log)
    assert code(lambda: g.run_log(dlog, 0, 1)) == ENOMODEL
    assert code(lambda: g.update_dvl(z)) == EINVAL  # neither a shared nor per-instance covariances
    zp = np.ascontiguousarray(z).ctypes.data_as(C.c_void_p)
    Rp = np.ascontiguousarray(R).ctypes.data_as(C.c_void_p)
    assert L.uwvk_vel_update_dvl(g.h, None, None, Rp, None) == EINVAL
    assert L.uwvk_vel_update_dvl(None, zp, None, Rp, None) == EINVAL
    assert L.uwvk_vel_update_pressure(g.h, None, None, Rp, None) == EINVAL
    assert L.uwvk_vel_predict(None, C.c_double(0.02)) == EINVAL
    assert L.uwvk_vel_run_log(g.h, None, C.c_int64(0), C.c_int64(1)) == EINVAL
    g.setup_motion_model(VS.uwv(log))
    assert code(lambda: g.run_log(dlog, 0, log["epochs"] + 1)) == EINVAL
    assert code(lambda: g.run_log(dlog, -1, 1)) == EINVAL
    x, P = g.get_state()
    np.testing.assert_array_equal(x, log["x0"])  # none of the refused calls touched the state
    np.testing.assert_array_equal(P, log["P0"])
    assert not g.get_status().any()


# ---- 7. run_log is the single calls ---------------------------------------
def _single_calls(g, log):
    """the oracle's order per epoch (or_vel_run_log): gyro, efforts, predict, DVL, pressure"""
    for e in range(log["epochs"]):
        g.set_gyro(log["gyro"][e])
        g.set_efforts(log["efforts"][e])
        g.predict(log["dt"])
        if log["flags"][e] & 2:
            g.update_dvl(log["dvl"][log["dvl_index"][e]], log["dvl_cov"])
        if log["flags"][e] & 4:
            g.update_pressure(log["pressure"][log["pressure_index"][e]], log["pressure_cov"])
    return snap(g)


def test_run_log_is_the_single_calls():
    """k_vel_epoch and k_vel_predict / k_vel_update call the same device
    functions on the same values: bitwise.  The row kernel sums across lanes."""
    B = 5
    log = scene("dense", B)
    ref = oracle_final("dense", B)
    steps = _single_calls(handle(log), log)
    r0, r1 = run(log, 0), run(log, 1)
    close(steps, ref, TOL_LOG, "single calls")
    close(r0, ref, TOL_LOG, "layout 0")
    print("run_log layout 0 against the single calls: x %.3g P %.3g model %.3g"
          % tuple(np.abs(a - b).max() for a, b in zip(r0[:3], steps[:3])))
    same(r0, steps)
    close(r1, steps, TOL_LOG, "layout 1 against the single calls")


# ---- 8. ranges compose -----------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ranges_compose(layout):
    log = scene("dense", 5)
    E = log["epochs"]
    whole = run(log, layout)
    assert log["flags"][5] and not log["flags"][7]
    for a in (5, 7):  # the second range starts at an event epoch / at an epoch without one
        same(run(log, layout, [(0, a), (a, E - a)]), whole)
    same(run(log, layout, [(0, 1), (1, E - 2), (E - 1, 1)]), whole)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_empty_range_changes_nothing(layout):
    log = scene("dense", 5)
    a, b = handle(log, layout), handle(log, layout)
    da, db = a.upload_log(log), b.upload_log(log)
    a.run_log(da, 0, 6)
    b.run_log(db, 0, 6)
    b.run_log(db, 9, 0)   # epoch 9's gyro and efforts must not reach the handle
    b.run_log(db, 0, 0)
    same(snap(b), snap(a))
    for g in (a, b):
        g.predict(log["dt"])  # reads the handle's stored gyro and efforts
    same(snap(b), snap(a))


# ---- 9. the launch boundary ------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_log():
    log = VS.add_events(synth.make_vel_log(5, 4100), [4095, 4096])
    o = VS.start(O.OracleVelBatch(5), log)
    o.run_log(log)
    return log, o.get_state(model=True)


@pytest.mark.parametrize("layout", [0, 1])
def test_launch_boundary(layout):
    """one call over 4,100 epochs is two launches, (0, 4096) and (4096, 4),
    with an update on either side of the cut"""
    log, ref = long_log()
    assert (log["flags"][[4095, 4096]] == 6).all()
    whole = run(log, layout)
    assert not whole[3].any()
    same(run(log, layout, [(0, 4096), (4096, 4)]), whole)
    close(whole, ref, TOL_LOG, "4100 epochs layout %d" % layout)


# ---- 10. latched inputs ----------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_predict_after_run_log_uses_the_last_epochs_inputs(layout):
    B = 5
    log = scene("tilted", B)
    o, g = VS.start(O.OracleVelBatch(B), log), handle(log, layout)
    o.run_log(log)
    g.run_log(g.upload_log(log))
    for f in (o, g):
        f.predict(log["dt"])  # no set_gyro / set_efforts: epoch E - 1's
    close(snap(g), o.get_state(model=True), TOL_LOG, "bare predict layout %d" % layout)
    # and the inputs matter: epoch 0's give another state
    other = VS.start(O.OracleVelBatch(B), log)
    other.run_log(log)
    other.set_gyro(log["gyro"][0])
    other.set_efforts(log["efforts"][0])
    other.predict(log["dt"])
    (xa, Pa), (xb, _) = o.get_state(), other.get_state()
    assert np.max(np.abs(xa - xb) / np.sqrt(np.diagonal(Pa, axis1=1, axis2=2))) > 1e-4


# ---- 11. the automatic layout ----------------------------------------------
@pytest.mark.parametrize("B,layout", [(GROUPS_MAX_BATCH, 1), (GROUPS_MAX_BATCH + 1, 0)])
def test_auto_layout(B, layout):
    """-1 is the row kernel up to 30,720 instances and the lane kernel from
    30,721 on (include/uwvk.h); the two differ in rounding
    (test_layouts_agree), so bitwise equality tells which one ran.  GPU against
    GPU only; 256 different instances, repeated."""
    log = VS.take(scene("dense", 256, 6), np.arange(B) % 256)
    auto, explicit, other = run(log, -1), run(log, layout), run(log, 1 - layout)
    same(auto, explicit)
    assert (auto[1] != other[1]).any()
    assert not auto[3].any()
