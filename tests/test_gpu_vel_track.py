"""uwvk_vel_run_log_track (k_vel_epoch_track, k_vel_epoch_g_track<16 / 32>)
through the C ABI, fp64, on the scenes of tests/vel_scenes.py and the screening
cases of tests/vel_track_scenes.py (each valid on the CPU first:
tests/test_vel_track_scenes.py):

 1. a clean log is the plain run, bitwise: final state, status, stored inputs,
    every record against the plain run cut there, the applied counts;
 2. the records against the oracle stepped to the same epochs;
 3. ranges and their records compose bitwise, count = 0 is a no-op;
 4. the 4,096-epoch launch boundary, with a record on its last epoch;
 5. a non-finite DVL / pressure sample is skipped for its instance alone;
 6. a non-finite gyro / efforts component skips that instance's predict;
 7. every error leaves state, status and the record buffers alone.
(8, the C++ facade: tests/test_facade_vel_run.py.)

Tolerances and layouts as tests/test_gpu_vel_edges.py: TOL_LOG = 1e-7 (means
in the reference's sigma, covariances relative to sqrt(P_ii P_jj)), TOL_MODEL =
1e-9 absolute; layout 0 one filter per lane, 1 one per 16-lane row, 2 the
diagnostic with a shadow row."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_ctypes as O
import test_gpu_vel_edges as VE
import vel_scenes as VS
import vel_track_scenes as TS
from uwvk import abi, engine, synth
from uwvk.vel_log import play_vel_log

pytestmark = pytest.mark.gpu

TOL_LOG = 1e-7
TOL_MODEL = 1e-9
NOTPD, NAN = 0x1, 0x2
LAYOUTS = [0, 1, 2]
EINVAL, ENOMODEL = 1, 4
SENTINEL = -777.0

same, snap, handle, run, scene, close = VE.same, VE.snap, VE.handle, VE.run, VE.scene, VE.close


def counts(log, first=0, count=None):
    """[2] the DVL and pressure events of epochs [first, first + count)"""
    f = log["flags"][first:log["epochs"] if count is None else first + count]
    return np.array([(f & abi.EV_DVL != 0).sum(), (f & abi.EV_PRESSURE != 0).sum()], np.uint32)


def records(t):
    return t.mean(), t.variance(), t.model()


def check_records_against_cuts(log, layout, t):
    """every record of track t is bitwise the plain run cut after that epoch:
    run_log over [0, e] on a fresh handle, then get_state.  (One cut per
    reference, not a chain of them: a cut stores the side lane's replica of
    (mu, Sigma) and reloads it into every lane, and the row kernels' replicas
    may differ in the last bit, see test_ranges_and_records_compose.)"""
    mean, var, model = records(t)
    for r, e in enumerate(t.epochs):
        p = handle(log, layout)
        p.run_log(p.upload_log(log), 0, int(e) + 1)
        x, P, m = p.get_state(model=True)
        np.testing.assert_array_equal(mean[r], x)
        np.testing.assert_array_equal(var[r], np.diagonal(P, axis1=1, axis2=2))
        np.testing.assert_array_equal(model[r], m)
    return len(t.epochs)


# ---- 1. a clean log is the plain run ---------------------------------------
@pytest.mark.parametrize("every", [1, 5])
@pytest.mark.parametrize("B", [1, 4, 5, 13])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_clean_log_is_the_plain_run(layout, B, every):
    log = scene("dense", B)
    E = log["epochs"]
    g, p = handle(log, layout), handle(log, layout)
    t = g.run_log_track(g.upload_log(log), every, model=True, applied=True)
    p.run_log(p.upload_log(log))
    got = snap(g)
    same(got, snap(p))
    assert not got[3].any()
    np.testing.assert_array_equal(t.epochs, np.arange(every - 1, E, every))
    assert check_records_against_cuts(log, layout, t) == E // every
    # the last record of instance B - 1 (the one the row kernel's dead rows copy) is not the first
    assert (t.mean()[-1][B - 1] != t.mean()[0][B - 1]).any()
    np.testing.assert_array_equal(t.applied(), np.tile(counts(log), (B, 1)))
    for f in (g, p):
        f.predict(log["dt"])  # reads the handle's stored gyro and efforts
    same(snap(g), snap(p))


def test_no_track_is_the_plain_run_and_outputs_can_be_left_out():
    log = scene("dense", 5)
    for layout in LAYOUTS:
        g = handle(log, layout)
        t = g.run_log_track(g.upload_log(log))
        same(snap(g), run(log, layout))
        assert len(t.epochs) == 0 and t.mean() is None and t.applied() is None
    g = handle(log, 1)
    t = g.run_log_track(g.upload_log(log), 4, mean=False, variance=False, model=True)
    assert t.mean() is None and t.variance() is None and t.model().shape == (3, 5, 13)
    same(snap(g), run(log, 1))
    np.testing.assert_array_equal(t.model()[-1], snap(g)[2])  # epoch 11 is the last


# ---- 2. against the oracle -------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_records_against_the_oracle(layout):
    B, every = 5, 7
    log = scene("tilted", B)
    g = handle(log, layout)
    t = g.run_log_track(g.upload_log(log), every, model=True)
    mean, var, model = records(t)
    assert list(t.epochs) == list(range(6, 60, 7))
    o = VS.start(O.OracleVelBatch(B), log)
    at = 0
    for r, e in enumerate(t.epochs):
        o.run_log(log, at, int(e) + 1 - at)
        at = int(e) + 1
        xo, Po, mo = o.get_state(model=True)
        d = np.diagonal(Po, axis1=1, axis2=2)
        es = float(np.max(np.abs(mean[r] - xo) / np.sqrt(d)))
        ev = float(np.max(np.abs(var[r] - d) / d))
        em = float(np.max(np.abs(model[r] - mo)))
        print("layout %d record %d (epoch %d): state %.3g variance %.3g model %.3g" % (layout, r, e, es, ev, em))
        assert es < TOL_LOG and ev < TOL_LOG and em < TOL_MODEL, (r, es, ev, em)
    assert not g.get_status().any()


# ---- 3. ranges and records compose ------------------------------------------
def raw_track(g, dlog, first, count, every, cap, outputs=("mean", "variance", "model")):
    """uwvk_vel_run_log_track with record buffers of `cap` records (at least one
    is allocated) and an applied buffer, all prefilled -> (code, {name: host copy})"""
    widths = dict(mean=4, variance=4, model=13)
    bufs = {k: engine.DeviceBuffer(np.full((max(cap, 1), g.batch, widths[k]), SENTINEL)) for k in outputs}
    bufs["applied"] = engine.DeviceBuffer(np.full((g.batch, 2), 7, np.uint32))
    t = abi.VelTrack()
    t.every, t.capacity = every, cap
    for k in outputs:
        setattr(t, k, bufs[k].ptr)
    code = g.L.uwvk_vel_run_log_track(g.h, C.byref(dlog.s), C.byref(dlog.hs), C.c_int64(first), C.c_int64(count),
                                      bufs["applied"].ptr, C.byref(t))
    g.synchronize()
    out = {k: bufs[k].read(np.float64, (max(cap, 1), g.batch, widths[k])) for k in outputs}
    out["applied"] = bufs["applied"].read(np.uint32, (g.batch, 2))
    return code, out


def untouched(out):
    return all((v == (7 if k == "applied" else SENTINEL)).all() for k, v in out.items())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ranges_and_records_compose(layout):
    """Bitwise on the lane-per-filter layout by construction.  On the row
    layouts a cut is exactly what it is for the plain uwvk_vel_run_log (the two
    kernels agree bitwise run for run, prefix for prefix and chain for chain):
    the first butterfly step of row_sum16(a * b) is contracted into an FMA, so
    the replicas of Sigma in even and odd lanes can differ in the last bit, and
    a cut reloads the side lane's into all of them.  At these cuts, as at those
    of test_gpu_vel_edges.test_ranges_compose, the scene's replicas agree."""
    B, every = 5, 5
    log = scene("dense", B)
    whole = handle(log, layout)
    tw = whole.run_log_track(whole.upload_log(log), every, model=True, applied=True)
    assert list(tw.epochs) == [4, 9]
    parts = handle(log, layout)
    dlog = parts.upload_log(log)
    got, applied, epochs = [], np.zeros((B, 2), np.uint32), []
    for first, count in ((0, 3), (3, 0), (3, 4), (7, 5)):
        t = parts.run_log_track(dlog, every, first, count, model=True, applied=True)
        got.append(records(t))
        epochs += list(t.epochs)
        applied += t.applied()
        np.testing.assert_array_equal(t.applied(), np.tile(counts(log, first, count), (B, 1)))
    assert epochs == [4, 9] and [len(r[0]) for r in got] == [0, 0, 1, 1]
    same(snap(parts), snap(whole))
    for k, rec in enumerate(records(tw)):
        np.testing.assert_array_equal(np.concatenate([r[k] for r in got]), rec)
    np.testing.assert_array_equal(applied, tw.applied())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_empty_range_changes_nothing(layout):
    log = scene("dense", 5)
    a, b = handle(log, layout), handle(log, layout)
    da, db = a.upload_log(log), b.upload_log(log)
    a.run_log_track(da, 5, 0, 6)
    b.run_log_track(db, 5, 0, 6)
    before = snap(b)
    for first in (9, 0, log["epochs"]):  # epoch 9's gyro and efforts must not reach the handle
        code, out = raw_track(b, db, first, 0, 1, 1)
        assert code == 0 and untouched(out)
    same(snap(b), before)
    same(snap(b), snap(a))
    for g in (a, b):
        g.predict(log["dt"])  # reads the handle's stored gyro and efforts
    same(snap(b), snap(a))


# ---- 4. the launch boundary --------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_log():
    """test_gpu_vel_edges.long_log's recipe (without its oracle run)"""
    return VS.add_events(synth.make_vel_log(5, 4100), [4095, 4096])


@pytest.mark.parametrize("layout", [0, 1])
def test_launch_boundary(layout):
    """one call over 4,100 epochs is two launches, (0, 4096) and (4096, 4); the
    fourth record falls on epoch 4,095, the last of the first launch"""
    log, every = long_log(), 1024
    assert (log["flags"][[4095, 4096]] == 6).all()
    whole = handle(log, layout)
    tw = whole.run_log_track(whole.upload_log(log), every, model=True, applied=True)
    assert list(tw.epochs) == [1023, 2047, 3071, 4095]
    parts = handle(log, layout)
    dlog = parts.upload_log(log)
    t1 = parts.run_log_track(dlog, every, 0, 4096, model=True, applied=True)
    t2 = parts.run_log_track(dlog, every, 4096, 4, model=True, applied=True)
    assert len(t1.epochs) == 4 and len(t2.epochs) == 0
    got = snap(whole)
    assert not got[3].any()
    same(snap(parts), got)
    same(got, run(log, layout))
    for a, b in zip(records(tw), records(t1)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(tw.applied(), t1.applied() + t2.applied())
    np.testing.assert_array_equal(tw.applied(), np.tile(counts(log), (5, 1)))
    # the record on the boundary is the state the first launch stored
    cut = handle(log, layout)
    cut.run_log(cut.upload_log(log), 0, 4096)
    x, P, m = cut.get_state(model=True)
    np.testing.assert_array_equal(tw.mean()[3], x)
    np.testing.assert_array_equal(tw.variance()[3], np.diagonal(P, axis1=1, axis2=2))
    np.testing.assert_array_equal(tw.model()[3], m)


# ---- 5. / 6. screening --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clean_track(layout):
    """(snap, applied) of the screened run over the clean scene"""
    log = TS.clean()
    g = handle(log, layout)
    t = g.run_log_track(g.upload_log(log), applied=True)
    return snap(g), t.applied()


def alone(j, skip, count=None, then_predict=False):
    """instance j of the clean scene on a batch-of-one handle, the single calls
    with `skip` left out -> snap"""
    one = VS.take(TS.clean(), j)
    g = handle(one)
    play_vel_log(g, one, 0, count, skip=skip)
    if then_predict:
        g.predict(one["dt"])
    return snap(g)


def check_instance(got, ref, j, layout, what):
    """instance j of `got` against the batch-of-one reference: bitwise on the
    lane-per-filter layout (the single calls' arithmetic), TOL_LOG on the rows"""
    mine = tuple(a[j:j + 1] for a in got[:3])
    assert all(np.isfinite(a).all() for a in mine)
    if layout == 0:
        same(mine, ref[:3])
    else:
        close(mine, ref, TOL_LOG, what)


def check_screened(bad_log, layout, skipped, short):
    """skipped: {instance: skip of play_vel_log}; short: {instance: (DVL, pressure) updates not applied}"""
    B = bad_log["batch"]
    g = handle(bad_log, layout)
    t = g.run_log_track(g.upload_log(bad_log), applied=True)
    got, (ref, ref_applied) = snap(g), clean_track(layout)
    others = np.ones(B, bool)
    others[list(skipped)] = False
    assert not ref[3].any()
    same(got, ref, others)  # status included: zero
    want = ref_applied.copy()
    for j, s in short.items():
        want[j] -= np.array(s, np.uint32)
    np.testing.assert_array_equal(t.applied(), want)
    for j, skip in skipped.items():
        assert got[3][j] == NAN, got[3]  # exactly UWVK_ST_NAN: no NOTPD
        check_instance(got, alone(j, skip), j, layout, "instance %d layout %d" % (j, layout))
    return g


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", TS.UPDATE_CASES)
def test_nonfinite_sample_is_skipped_for_its_instance(case, layout):
    c = TS.CASES[case]
    check_screened(TS.poison(TS.clean(), case), layout, {TS.J: c["skip"]}, {TS.J: c["applied"]})


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", TS.INPUT_CASES)
def test_nonfinite_input_skips_the_predict(case, layout):
    c = TS.CASES[case]
    j, e = TS.J, c["epoch"]
    bad = TS.poison(TS.clean(), case)
    g = check_screened(bad, layout, {j: c["skip"]}, {})
    g.predict(bad["dt"])  # the stored inputs: the last epoch's, finite for every instance
    check_instance(snap(g), alone(j, c["skip"], then_predict=True), j, layout, "bare predict")
    # the range that ends with the bad epoch: instance j keeps the inputs of epoch e - 1
    g = handle(bad, layout)
    g.run_log_track(g.upload_log(bad), first=0, count=e + 1)
    g.predict(bad["dt"])
    got = snap(g)
    assert got[3][j] == NAN and not got[3][np.arange(TS.B) != j].any()
    check_instance(got, alone(j, c["skip"], count=e + 1, then_predict=True), j, layout, "bare predict after the cut")
    ref = handle(TS.clean(), layout)
    ref.run_log(ref.upload_log(TS.clean()), 0, e + 1)
    ref.predict(bad["dt"])
    same(got, snap(ref), np.arange(TS.B) != j)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_instances_of_one_wave_skip_at_different_epochs(layout):
    (ja, ea), (jb, eb) = TS.PAIR
    assert ja // 4 == jb // 4 and ea != eb
    check_screened(TS.poison_pair(TS.clean()), layout, {ja: dict(predict=[ea]), jb: dict(predict=[eb])}, {})


def test_an_instance_without_a_finite_epoch_keeps_its_inputs():
    """every epoch of the range bad for instance j: no predict at all, the
    updates still run, and the handle's stored gyro / efforts stay what they were"""
    j, first, n = TS.J, 1, 4
    log = TS.clean()
    bad = dict(log, gyro=log["gyro"].copy())
    bad["gyro"][first:first + n, j, 1] = np.inf
    for layout in LAYOUTS:
        g = handle(bad, layout)
        g.run_log_track(g.upload_log(bad), first=first, count=n)
        g.predict(bad["dt"])
        one = VS.take(log, j)
        ref = handle(one)  # VS.start's set_gyro(gyro[0]) and zero efforts are the stored inputs
        play_vel_log(ref, one, first, n, skip=dict(predict=range(first, first + n)))
        ref.predict(one["dt"])
        got = snap(g)
        assert got[3][j] == NAN
        check_instance(got, snap(ref), j, layout, "no finite epoch, layout %d" % layout)


# ---- 7. errors leave everything alone ----------------------------------------
def test_errors_leave_the_state_alone():
    B = 5
    log = scene("dense", B)
    g = handle(log)
    dlog = g.upload_log(log)
    g.run_log_track(dlog, first=0, count=3)
    before = snap(g)
    E = log["epochs"]

    def refused(code, want, out):
        assert code == want and untouched(out)
        same(snap(g), before)

    code, out = raw_track(g, dlog, 0, E, 5, 1)
    refused(code, EINVAL, out)                                                                # 2 records, room for 1
    code, out = raw_track(g, dlog, 0, E, 0, 4)
    refused(code, EINVAL, out)                                                                # every = 0
    code, out = raw_track(g, dlog, 0, E, -3, 4)
    refused(code, EINVAL, out)
    code, out = raw_track(g, dlog, 0, E, 5, 4, outputs=())
    refused(code, EINVAL, out)                                                                # all three buffers NULL
    for first, count in ((0, E + 1), (-1, 2), (3, -1)):
        code, out = raw_track(g, dlog, first, count, 5, 4)
        refused(code, EINVAL, out)
    # a host index past the payload, inside the range only
    e = int(np.flatnonzero(log["flags"] & abi.EV_DVL)[1])
    keep = int(dlog.host["dvl_index"][e])
    dlog.host["dvl_index"][e] = dlog.hs.n_dvl
    code, out = raw_track(g, dlog, 3, E - 3, 5, 4)
    refused(code, EINVAL, out)
    assert g.log_check(dlog, 3, E - 3) == EINVAL and g.log_check(dlog, 3, e - 3) == 0
    dlog.host["dvl_index"][e] = keep
    assert g.log_check(dlog) == 0
    with pytest.raises(engine.UWVKError) as err:
        g.run_log_track(dlog, 5, capacity=1)
    assert err.value.code == EINVAL
    same(snap(g), before)
    # no motion model: after the log and track checks
    bare = engine.VelocityUKFBatch(B)
    bare.init(log["x0"], log["P0"])
    x0, P0 = bare.get_state()
    code, out = raw_track(bare, dlog, 0, E, 5, 4)
    assert code == ENOMODEL and untouched(out)
    code, out = raw_track(bare, dlog, 0, E, 0, 4)
    assert code == EINVAL and untouched(out)
    np.testing.assert_array_equal(bare.get_state()[0], x0)
    np.testing.assert_array_equal(bare.get_state()[1], P0)
    assert not bare.get_status().any()
    L = engine.lib()
    assert L.uwvk_vel_run_log_track(None, C.byref(dlog.s), C.byref(dlog.hs), C.c_int64(0), C.c_int64(1), None,
                                    None) == EINVAL
    assert L.uwvk_vel_run_log_track(g.h, C.byref(dlog.s), None, C.c_int64(0), C.c_int64(1), None, None) == EINVAL
    # and the handle still runs: the rest of the log equals one call
    g.run_log_track(dlog, first=3)
    same(snap(g), run(log, None))
