"""BottomUKFBatch.run_log (uwvk_bottom_run_log, k_bottom_run in csrc/uwvk_small.hip)
against the single calls on a second handle (play_bottom_log): bitwise in mu,
Sigma and the status words, including the track records, adjacent ranges, the
4096-epoch launch boundary, the per-instance skips and the not-positive-definite
rule; and against the CPU oracle to the 1e-9 sigma of tests/test_small_filters.py.
Batches of at most 37; the longest log (4100 epochs) takes about a second."""
import numpy as np
import pytest

import oracle_ctypes as O
import small_scenes as S
import visual_scene as V
from uwvk import abi, engine
from uwvk.small import BottomLogRecorder, BottomUKFBatch, play_bottom_log

pytestmark = pytest.mark.gpu
TOL = 1e-9
NOTPD, NAN = 0x1, 0x2
DT = 0.2


def make(x, P, cls=BottomUKFBatch):
    f = cls(len(x))
    f.init(x, P)
    f.set_process_noise(S.BOTTOM_Q)
    return f


def snap(f):
    x, P = f.get_state()
    return x, P, f.get_status()


def same(a, b, rows=slice(None)):
    """(x, P[, status]) tuples bitwise equal on `rows`"""
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u[rows], v[rows])


def counter(f):
    return engine.DeviceBuffer(np.zeros((f.batch, 2), np.uint32), f.device)


def counts(f, buf):
    return buf.read(np.uint32, (f.batch, 2), f.stream)


def copy_log(log):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in log.items()}


_RECORDED = {}


def recorded(B, steps=30, seed_state=5, tilt=0.1):
    """bottom_sequence recorded and, in parallel, applied to the oracle: (x0, P0, log, oracle state)"""
    key = (B, steps, seed_state, tilt)
    if key not in _RECORDED:
        x, P = V.bottom_state(B, seed=seed_state, tilt=tilt)
        o = make(x, P, O.OracleBottomBatch)
        rec = BottomLogRecorder(B, DT)
        S.bottom_sequence((rec, o), B, steps=steps)
        _RECORDED[key] = (x, P, rec.log(), o.get_state())
    x, P, log, ostate = _RECORDED[key]
    return x.copy(), P.copy(), copy_log(log), ostate


def run_and_play(x, P, log, **kw):
    """-> (run handle, played handle, issued counts): the run on one handle, the single calls on a second"""
    f, g = make(x, P), make(x, P)
    f.run_log(f.upload_log(log), **kw)
    issued = play_bottom_log(g, log)
    return f, g, issued


@pytest.mark.parametrize("B", [37, 1])  # 37: 4 blocks of 8 and a block of 5
def test_run_is_the_single_calls_and_the_oracle(B):
    x, P, log, (xo, Po) = recorded(B)
    assert log["epochs"] == 30 and log["range_var"] is not None
    f, g, _ = run_and_play(x, P, log)
    same(snap(f), snap(g))
    assert not f.get_status().any()
    xg, Pg = f.get_state()
    assert (xg != x).any() and (Pg != P).any()
    es, ec = S.bottom_err(xg, Pg, xo, Po)
    print("B = %d against the oracle: state %.3g sigma, covariance %.3g" % (B, es, ec))
    assert es < TOL and ec < TOL, (es, ec)
    # the handle's velocity is the last epoch's, as after the single calls
    f.predict(DT)
    g.predict(DT)
    same(snap(f), snap(g))


def test_four_beams_in_one_epoch_shared_covariance():
    B, E = 9, 12
    rng = np.random.default_rng(17)
    x, P = V.bottom_state(B)
    rec = BottomLogRecorder(B, DT)
    for e in range(E):
        rec.set_velocity(np.c_[rng.normal(0.5, 0.1, B), rng.normal(0, 0.1, B), rng.normal(0, 0.05, B)])
        rec.predict(DT)
        for d, o in S.BEAMS:
            rec.update_range(10.0 / 0.866 + rng.normal(0, 0.05, B), 0.02, d, o)
        if e % 3 == 2:
            rec.update_normal(V.unit(np.c_[rng.normal(0, 0.03, (B, 2)), np.ones(B)]), np.eye(2) * 4e-4)
    log = rec.log()
    assert log["range_var"] is None and log["range_cov"] == 0.02
    assert (log["flags"] & 0xF == 0xF).all() and (log["flags"][2::3] & abi.BEV_NORMAL).all()
    f, g = make(x, P), make(x, P)
    ap = counter(f)
    f.run_log(f.upload_log(log), applied=ap)
    issued = play_bottom_log(g, log)
    same(snap(f), snap(g))
    assert not f.get_status().any()
    np.testing.assert_array_equal(counts(f, ap), issued)
    np.testing.assert_array_equal(issued, np.tile([4 * E, E // 3], (B, 1)))


def test_adjacent_ranges_and_the_launch_boundary():
    """4100 epochs of predict and one beam: more than one 4096-epoch launch"""
    B, E, rows = 9, 4100, 16
    rng = np.random.default_rng(23)
    x, P = V.bottom_state(B)
    e = np.arange(E)
    log = dict(epochs=E, dt=DT, beams=4, flags=(1 << (e % 4)).astype(np.uint32),
               velocity=np.stack([rng.normal(0.5, 0.1, (E, B)), rng.normal(0, 0.1, (E, B)),
                                  rng.normal(0, 0.05, (E, B))], -1),
               beam_direction=np.array([b[0] for b in S.BEAMS]), beam_origin=np.array([b[1] for b in S.BEAMS]),
               range_index=(e % rows).astype(np.int32), range=10.0 / 0.866 + rng.normal(0, 0.05, (rows, 4, B)),
               range_var=rng.uniform(0.01, 0.03, (rows, 4, B)), range_cov=0.0,
               normal_index=np.zeros(E, np.int32), normal=np.zeros((0, B, 3)), normal_cov=np.eye(2))
    one, two, played = make(x, P), make(x, P), make(x, P)
    one.run_log(one.upload_log(log))
    d = two.upload_log(log)
    two.run_log(d, 0, 4090, sync=False)
    two.run_log(d, 4090, 10)
    play_bottom_log(played, log)
    same(snap(one), snap(two))
    same(snap(one), snap(played))
    assert not one.get_status().any()


def test_track_records():
    B, E, every = 37, 30, 4
    x, P, log, _ = recorded(B)
    f, g, h = make(x, P), make(x, P), make(x, P)
    mean, var = f.run_log(f.upload_log(log), every=every)
    assert mean.shape == (7, B, 4) and var.shape == (7, B, 3)
    r = 0
    for e in range(E):
        play_bottom_log(g, log, e, 1)
        if (e + 1) % every == 0:
            xg, Pg = g.get_state()
            np.testing.assert_array_equal(mean[r], xg)
            np.testing.assert_array_equal(var[r], np.diagonal(Pg, axis1=1, axis2=2))
            r += 1
    assert r == 7
    same(snap(f), snap(g))
    # adjacent calls: their records concatenate to those of one call
    d = h.upload_log(log)
    m1, v1 = h.run_log(d, 0, 10, every=every)
    m2, v2 = h.run_log(d, 10, 20, every=every)
    assert len(m1) == 2 and len(m2) == 5
    np.testing.assert_array_equal(np.concatenate([m1, m2]), mean)
    np.testing.assert_array_equal(np.concatenate([v1, v2]), var)
    same(snap(h), snap(f))
    # one output switched off
    k = make(x, P)
    m3, v3 = k.run_log(k.upload_log(log), every=every, variance=False)
    assert v3 is None
    np.testing.assert_array_equal(m3, mean)
    # a bad track: UWVK_EINVAL, nothing queued, the state untouched
    before = snap(f)
    d = f.upload_log(log)
    for kw in (dict(every=every, capacity=6), dict(every=0), dict(every=every, mean=False, variance=False)):
        with pytest.raises(engine.UWVKError) as err:
            f.run_log(d, **kw)
        assert err.value.code == 1, kw
        same(snap(f), before)


def poisoned(B, spoil, epochs=10):
    """the recorded sequence with and without spoil(log): (run, played, issued, applied, clean run)"""
    x, P, log, _ = recorded(B, steps=epochs)
    clean = make(x, P)
    clean.run_log(clean.upload_log(log))
    assert not clean.get_status().any()
    spoil(log)
    f, g = make(x, P), make(x, P)
    ap = counter(f)
    f.run_log(f.upload_log(log), applied=ap)
    issued = play_bottom_log(g, log)
    return f, g, issued, counts(f, ap), clean


def test_non_finite_range_and_variance_are_skipped_per_instance():
    B = 16  # the poisoned instances share their waves with good ones

    def spoil(log):
        log["range"][2, 2, 5] = np.nan      # epoch 2 is beam 2
        log["range_var"][3, 3, 9] = np.inf  # epoch 3 is beam 3
    f, g, issued, applied, clean = poisoned(B, spoil)
    same(snap(f)[:2], snap(g)[:2])          # the twin with those instances masked out of those steps
    st = f.get_status()
    np.testing.assert_array_equal(st, np.where(np.isin(np.arange(B), [5, 9]), NAN, 0))
    assert not g.get_status().any()         # the single calls' mask leaves no bit
    want = np.tile([10, 2], (B, 1))
    want[[5, 9], 0] -= 1
    np.testing.assert_array_equal(applied, want)
    np.testing.assert_array_equal(issued, want)
    others = ~np.isin(np.arange(B), [5, 9])
    same(snap(f)[:2], snap(clean)[:2], others)
    assert (f.get_state()[0][~others] != clean.get_state()[0][~others]).any(axis=1).all()


def test_zero_length_normal_is_skipped_per_instance():
    B = 16

    def spoil(log):
        log["normal"][1, 3] = 0.0  # the second normal (epoch 9)
    f, g, issued, applied, clean = poisoned(B, spoil)
    same(snap(f)[:2], snap(g)[:2])
    np.testing.assert_array_equal(f.get_status(), np.where(np.arange(B) == 3, NAN, 0))
    want = np.tile([10, 2], (B, 1))
    want[3, 1] -= 1
    np.testing.assert_array_equal(applied, want)
    np.testing.assert_array_equal(issued, want)
    others = np.arange(B) != 3
    same(snap(f)[:2], snap(clean)[:2], others)
    assert (f.get_state()[0][3] != clean.get_state()[0][3]).any()


def test_non_finite_velocity_skips_that_instances_predict():
    B, E = 16, 11
    x, P, log, _ = recorded(B, steps=10)
    rng = np.random.default_rng(29)
    log["epochs"] = E                       # an eleventh epoch: a predict and no update
    log["flags"] = np.r_[log["flags"], np.uint32(0)]
    log["range_index"] = np.r_[log["range_index"], np.int32(0)]
    log["normal_index"] = np.r_[log["normal_index"], np.int32(0)]
    log["velocity"] = np.concatenate([log["velocity"], rng.normal(0.3, 0.1, (1, B, 3))])
    clean, f, short = make(x, P), make(x, P), make(x, P)
    clean.run_log(clean.upload_log(log))
    short.run_log(short.upload_log(log), 0, E - 1)
    log["velocity"][E - 1, 7, 1] = np.nan
    f.run_log(f.upload_log(log))
    others = np.arange(B) != 7
    same(snap(f)[:2], snap(short)[:2], 7)    # its state after epochs - 1
    same(snap(f)[:2], snap(clean)[:2], others)
    assert (clean.get_state()[0][7] != short.get_state()[0][7]).any()
    np.testing.assert_array_equal(f.get_status(), np.where(others, 0, NAN))
    # its stored velocity keeps its last finite value, that of epoch 9
    f.predict(DT)
    short.predict(DT)
    same(snap(f)[:2], snap(short)[:2], 7)


@pytest.mark.parametrize("case", ["sigma_at_init", "negative_range_variance"])
def test_not_positive_definite_keeps_the_state_and_carries_on(case):
    """the two cases of tests/test_gpu_small_edges.py on one instance of B = 16 in a 6-epoch log"""
    B, E = 16, 6
    x, P, log, _ = recorded(B, steps=E, seed_state=41, tilt=0.2)
    healthy = make(x, P)
    healthy.run_log(healthy.upload_log(log))
    assert not healthy.get_status().any()
    if case == "sigma_at_init":
        j = 10
        P[j, 0, 0] = -0.1                   # a negative leading pivot: every step of the run fails
    else:
        j = 12
        log["range_var"][0, 0, j] = -0.05   # Sigma - C K^T indefinite: apply_delta's re-spread fails
    f, g = make(x, P), make(x, P)
    ap = counter(f)
    f.run_log(f.upload_log(log), applied=ap)
    issued = play_bottom_log(g, log)
    same(snap(f), snap(g))                   # the twin keeps the state from before the failed step and carries on
    others = np.arange(B) != j
    np.testing.assert_array_equal(f.get_status(), np.where(others, 0, NOTPD))
    same(snap(f)[:2], snap(healthy)[:2], others)
    applied = counts(f, ap)
    np.testing.assert_array_equal(applied[others], issued[others])
    xf, Pf = f.get_state()
    x0, P0 = make(x, P).get_state()
    if case == "sigma_at_init":
        np.testing.assert_array_equal(xf[j], x0[j])
        np.testing.assert_array_equal(Pf[j], P0[j])
        np.testing.assert_array_equal(applied[j], [0, 0])
    else:
        assert (xf[j] != x0[j]).any() and np.isfinite(Pf[j]).all() and np.linalg.eigvalsh(Pf[j]).min() > 0
        np.testing.assert_array_equal(applied[j], issued[j] - [1, 0])  # the later steps ran on it


def test_errors_leave_nothing_behind():
    B = 16
    x, P, log, _ = recorded(B, steps=10)
    f = make(x, P)
    f.run_log(f.upload_log(log), 0, 4)
    before = snap(f)
    bad = copy_log(log)
    bad["range_index"][6] = len(bad["range"])
    with pytest.raises(engine.UWVKError) as err:
        f.run_log(f.upload_log(bad), 4, 6)
    assert err.value.code == 1  # UWVK_EINVAL
    same(snap(f), before)
    f.run_log(f.upload_log(bad), 4, 2)  # a range without the bad epoch runs
    assert (f.get_state()[0] != before[0]).any()
    fresh = BottomUKFBatch(B)
    with pytest.raises(engine.UWVKError) as err:
        fresh.run_log(fresh.upload_log(log))
    assert err.value.code == 7  # UWVK_ENOTINIT
