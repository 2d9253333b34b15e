"""The track recorder (uwvk_pose_run_log_track, csrc/uwvk_track.hip): while
run_log runs, after every `every`-th epoch of the log a record of all
instances (means, the diagonal of Sigma, ensemble statistics) goes to device
buffers.  Its contract: bitwise what uwvk_pose_run_log gives on each segment
between record epochs with get_state / ensemble_stats at each cut, on every
path run_log has (pair, one-instance PD, general, 26 DOF, literal, both SO3
sides), with the launches of each segment planned on their own."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from uwvk import engine
    if not engine.device_available(0):
        pytest.fail("no gfx950 device / libuwvk.so not loadable: the HIP path is mandatory")
    return engine


def _handle(eng, log, dof=53, pd=True, right=True, literal=False):
    from uwvk import synth
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    B = log["gyro"].shape[1]
    g = eng.PoseUKFBatch(B, dof)
    g.set_param_block(pd)
    g.set_so3_right(right)
    if literal:
        g.set_literal_apply_delta(True)
    g.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    g.set_process_noise_from_config(cfg, log["dt"])
    return g


def _by_cuts(eng, g, log, cuts, records, truth=None):
    """run_log over the pieces between `cuts`, the state (and the statistics
    against truth[r]) read after each cut that is in `records`."""
    B = log["gyro"].shape[1]
    dlog = g.upload_log(log)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    xs, vs, st = [], [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        g.run_log(dlog, a, b - a, accept_counts=acc)
        if b in records:
            x, P = g.get_state()
            xs.append(x)
            vs.append(np.diagonal(P, axis1=1, axis2=2).copy())
            if truth is not None:
                st.append(g.ensemble_stats(truth[len(st)]))
    x, P = g.get_state()
    return dict(mean=np.array(xs), variance=np.array(vs), stats=np.array(st), x=x, P=P,
                acc=acc.read(np.uint32, (B, 4)), status=g.get_status(), pd=g.param_block(), pair=g.pair_active())


def _tracked(eng, g, log, every, ranges, **kw):
    B = log["gyro"].shape[1]
    dlog = g.upload_log(log)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    tracks = [g.run_log_track(dlog, every, a, n, accept_counts=acc, **kw) for a, n in ranges]
    x, P = g.get_state()
    cat = lambda f: np.concatenate([f(t) for t in tracks])  # noqa: E731
    return dict(tracks=tracks, epochs=cat(lambda t: t.epochs), mean=cat(lambda t: t.mean()),
                variance=cat(lambda t: t.variance()), x=x, P=P, acc=acc.read(np.uint32, (B, 4)),
                status=g.get_status(), pd=g.param_block(), pair=g.pair_active())


def _same(got, ref, names=("mean", "variance", "x", "P", "acc", "status", "pd", "pair")):
    for k in names:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


# B, dof, pd option, SO3 right side, (pair kernel, PD kernel) expected at the start
PATHS = [
    pytest.param(6, 53, True, True, (1, 1), id="pair"),
    pytest.param(6, 53, True, False, (1, 1), id="pair_left"),
    pytest.param(5, 53, True, True, (0, 1), id="odd_batch_pd"),
    pytest.param(6, 26, True, True, (1, 0), id="dof26"),
    pytest.param(6, 53, False, True, (0, 0), id="general"),
]


@pytest.mark.parametrize("B,dof,pd,right,kernels", PATHS)
def test_track_bitwise(eng, B, dof, pd, right, kernels):
    """One tracked call against run_log cut at the record epochs: records after
    epochs 24, 49, 74 and 99, the last 20 epochs without one."""
    from uwvk import synth
    log = synth.make_pose_log(B, 120, "C3", dof=dof)
    ga, gb = (_handle(eng, log, dof, pd, right) for _ in range(2))
    assert (ga.pair_active(), ga.param_block()) == kernels
    got = _tracked(eng, ga, log, 25, [(0, 120)])
    ref = _by_cuts(eng, gb, log, [0, 25, 50, 75, 100, 120], {25, 50, 75, 100})
    np.testing.assert_array_equal(got["epochs"], [24, 49, 74, 99])
    assert got["mean"].shape == (4, B, dof + 1) and got["variance"].shape == (4, B, dof)
    _same(got, ref)
    assert not got["status"].any() and (got["variance"] > 0).all()


def test_track_bitwise_literal(eng):
    """The literal path: one launch per epoch, a snapshot after the due ones."""
    from uwvk import synth
    log = synth.make_pose_log(6, 12, "C3")
    ga, gb = (_handle(eng, log, literal=True) for _ in range(2))
    got = _tracked(eng, ga, log, 5, [(0, 12)])
    ref = _by_cuts(eng, gb, log, [0, 5, 10, 12], {5, 10})
    np.testing.assert_array_equal(got["epochs"], [4, 9])
    _same(got, ref)
    assert got["pd"] == 0


@pytest.mark.parametrize("dof", [53, 26])
def test_track_all_events_match_oracle(eng, dof):
    """The compressed C4 log of test_gpu_pd.py::test_pair_matches_oracle
    (pressure, ADCP and BodyEfforts epochs; the efforts epochs 399 and 899 are
    record epochs): every record against the oracle advanced piecewise."""
    from helpers import init_both, state_err
    import oracle_ctypes as orc
    from uwvk import abi, synth
    B, E, every = 6, 900, 100
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    log = synth.make_pose_log(B, E, "C4", dof=dof, dropout_on=0.4, dropout_off=0.1, adcp_every=150)
    fl = log["flags"]
    for bit in (abi.EV_PRESSURE, abi.EV_ADCP, abi.EV_EFFORTS):
        assert ((fl & bit) != 0).any()
    rec = np.arange(every - 1, E, every)
    assert ((fl[rec] & abi.EV_EFFORTS) != 0).any()  # a record right after a BodyEfforts update
    o = orc.OraclePoseBatch(B, dof)
    g = eng.PoseUKFBatch(B, dof)
    init_both(o, g, cfg, uwv, log)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    tr = g.run_log_track(g.upload_log(log), every, accept_counts=acc)
    np.testing.assert_array_equal(tr.epochs, rec)
    mean, var = tr.mean(), tr.variance()
    co = np.zeros((B, 4), np.uint32)
    for r, e in enumerate(rec):
        co += o.run_log(log, e + 1 - every, every)
        xo, Po = o.get_state()
        do = np.diagonal(Po, axis1=1, axis2=2)
        es = state_err(mean[r], xo, Po, dof).max()
        ev = (np.abs(var[r] - do) / do).max()
        print("dof %d record %d (epoch %d): state %.3e variance %.3e" % (dof, r, e, es, ev))
        assert es < 1e-7 and ev < 1e-7, (r, es, ev)
    np.testing.assert_array_equal(co, acc.read(np.uint32, (B, 4)))
    assert not g.get_status().any()


def test_track_calls_compose(eng):
    """Adjacent ranges: (0, 70) then (70, 50) give 2 + 2 records, those of
    run_log cut at 25, 50, 70, 75, 100 and 120."""
    from uwvk import synth
    log = synth.make_pose_log(6, 120, "C3")
    ga, gb = (_handle(eng, log) for _ in range(2))
    got = _tracked(eng, ga, log, 25, [(0, 70), (70, 50)])
    assert [len(t.epochs) for t in got["tracks"]] == [2, 2]
    np.testing.assert_array_equal(got["epochs"], [24, 49, 74, 99])
    ref = _by_cuts(eng, gb, log, [0, 25, 50, 70, 75, 100, 120], {25, 50, 75, 100})
    _same(got, ref)


def test_track_stats(eng):
    """The statistics of a record are ensemble_stats at that cut, bitwise (the
    same two kernels); 70 instances: two blocks of k_pose_stats."""
    from uwvk import synth
    B, E, every = 70, 60, 20
    log = synth.make_pose_log(B, E, "C3")
    truth = np.array([log["truth"].state(e + 1, 53) for e in (19, 39, 59)])
    ga, gb = (_handle(eng, log) for _ in range(2))
    tr = ga.run_log_track(ga.upload_log(log), every, mean=False, variance=False, stats=True, truth=truth)
    ref = _by_cuts(eng, gb, log, [0, 20, 40, 60], {20, 40, 60}, truth=truth)
    assert tr.mean() is None and tr.variance() is None
    st = tr.stats()
    assert st.shape == (3, 3 * 54 + 2)
    np.testing.assert_array_equal(st, ref["stats"])
    assert (st[:, -1] == 0).all() and np.isfinite(st).all()  # every instance in the NEES sum
    xa, Pa = ga.get_state()
    np.testing.assert_array_equal(xa, ref["x"])
    np.testing.assert_array_equal(Pa, ref["P"])
    # no truth: ensemble_stats' None
    gc, gd = (_handle(eng, log) for _ in range(2))
    t0 = gc.run_log_track(gc.upload_log(log), 60, mean=False, variance=False, stats=True)
    gd.run_log(gd.upload_log(log))
    np.testing.assert_array_equal(t0.stats()[0], gd.ensemble_stats(None))


def test_track_arguments(eng):
    from uwvk import synth
    B, E = 6, 60
    log = synth.make_pose_log(B, E, "C3")
    g, ref = (_handle(eng, log) for _ in range(2))
    dlog = g.upload_log(log)
    x0, P0 = g.get_state()
    for kw in (dict(every=0), dict(every=-5), dict(every=20, mean=False, variance=False, stats=False),
               dict(every=20, capacity=2)):  # 3 records in 60 epochs
        with pytest.raises(eng.UWVKError) as ei:
            g.run_log_track(dlog, **kw)
        assert ei.value.code == 1, kw  # UWVK_EINVAL
        x, P = g.get_state()
        np.testing.assert_array_equal(x, x0)
        np.testing.assert_array_equal(P, P0)
    # no epochs: OK, no record, nothing changes
    t = g.run_log_track(dlog, 20, first=19, count=0)
    assert len(t.epochs) == 0 and t.mean().shape == (0, B, 54)
    np.testing.assert_array_equal(g.get_state()[1], P0)
    # a range without a record epoch
    assert len(g.run_log_track(dlog, 20, first=0, count=19).epochs) == 0
    assert list(g.run_log_track(dlog, 20, first=19, count=1).epochs) == [19]
    # track = NULL is run_log
    acc, acc_ref = (eng.DeviceBuffer(np.zeros((B, 4), np.uint32)) for _ in range(2))
    eng._chk(g.L.uwvk_pose_run_log_track(g.h, C.byref(dlog.s), C.c_int64(20), C.c_int64(40), acc.ptr, None))
    g.synchronize()
    rlog = ref.upload_log(log)
    ref.run_log(rlog, 0, 19)  # the pieces g has run so far
    ref.run_log(rlog, 19, 1)
    ref.run_log(rlog, 20, 40, accept_counts=acc_ref)
    for a, b in zip(g.get_state(), ref.get_state()):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(acc.read(np.uint32, (B, 4)), acc_ref.read(np.uint32, (B, 4)))


def test_mission_replay(eng):
    """mission.replay: upload, tracked run, numpy arrays back."""
    from uwvk import mission, synth
    log = synth.make_pose_log(6, 50, "C3")
    g = _handle(eng, log)
    out = mission.replay(g, log, 25)
    np.testing.assert_array_equal(out["epochs"], [24, 49])
    x, P = g.get_state()
    np.testing.assert_array_equal(out["mean"][-1], x)
    np.testing.assert_array_equal(out["variance"][-1], np.diagonal(P, axis1=1, axis2=2))
    assert out["stats"] is None
    truth = np.array([log["truth"].state(e + 1, 53) for e in out["epochs"]])
    g2 = _handle(eng, log)
    out2 = mission.replay(g2, log, 25, truth=truth)
    np.testing.assert_array_equal(out2["mean"], out["mean"])
    np.testing.assert_array_equal(out2["stats"][-1], g2.ensemble_stats(truth[-1]))
