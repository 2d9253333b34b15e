"""IndirectPoseUKFBatch.run_log (uwvk_ipose_run_log, k_ipose_run in csrc/uwvk_small.hip)
against the single calls on a second handle (play_ipose_log): bitwise in mu,
Sigma and the status words, including the mean / variance records, adjacent
ranges, the 4096-epoch launch boundary, the per-instance skips and the
not-positive-definite rule; the corrected-pose records against
get_corrected_pose to the rounding bound of include/uwvk.h; and against the CPU
oracle to the tolerance of tests/test_gpu_small_edges.py.
Batches of at most 9; the longest log (4100 epochs) takes about a second."""
import numpy as np
import pytest

import ipose_run_scenes as R
import oracle_ctypes as O
import small_scenes as S
from test_gpu_small_edges import TOL, IPoseCase, _ipose_with_indefinite
from uwvk import engine
from uwvk.small import IndirectPoseUKFBatch, play_ipose_log

pytestmark = pytest.mark.gpu
NOTPD, NAN = 0x1, 0x2
EPS = 2.0 ** -52
SIDES = pytest.mark.parametrize("right", [True, False], ids=["right", "left"])


def make(B, right=True):
    f = IndirectPoseUKFBatch(B)
    if not right:
        f.set_so3_right(False)
    return R.init(f, B)


def snap(f):
    x, P = f.get_state()
    return x, P, f.get_status()


def same(a, b, rows=slice(None)):
    """(x, P[, status]) tuples bitwise equal on `rows`"""
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u[rows], v[rows])


def counter(f):
    return engine.DeviceBuffer(np.zeros(f.batch, np.uint32), f.device)


def counts(f, buf):
    return buf.read(np.uint32, (f.batch,), f.stream)


_LOGS = {}


def recorded(B, **kw):
    key = (B,) + tuple(sorted((k, str(v)) for k, v in kw.items()))
    if key not in _LOGS:
        _LOGS[key] = R.record(B, **kw)
    return R.copy_log(_LOGS[key])


def run_and_play(log, right=True, **kw):
    """-> (run handle, played handle, issued counts, applied counts)"""
    B = log["batch"]
    f, g = make(B, right), make(B, right)
    ap = counter(f)
    f.run_log(f.upload_log(log), applied=ap, **kw)
    issued = play_ipose_log(g, log)
    return f, g, issued, counts(f, ap)


# ---- 1. parity ----------------------------------------------------------------
@SIDES
@pytest.mark.parametrize("B", [5, 1])  # 5: two full blocks and a half-empty one; 1: a lone slot
def test_run_is_the_single_calls_and_the_oracle(B, right):
    log = recorded(B)
    assert log["epochs"] == 6 and log["dt_epoch"] is not None and list(np.diff(log["visual_offset"])) == list(R.ROWS6)
    assert (log["pose_ref"][1] != log["pose_ref"][0]).any()
    with O.so3_side(right):  # the oracle first, on the CPU: its calls raise on any failure, so the scene is valid
        o = R.init(O.OracleIndirectPoseBatch(B), B)
        play_ipose_log(o, log)
        xo, Po = o.get_state()
    assert np.isfinite(xo).all() and all(np.linalg.eigvalsh(P).min() > 0 for P in Po)
    f, g, issued, applied = run_and_play(log, right)
    x0 = make(B, right).get_state()
    same(snap(f), snap(g))
    assert not f.get_status().any()
    xg, Pg = f.get_state()
    assert (xg != x0[0]).any() and (Pg != x0[1]).any()
    np.testing.assert_array_equal(applied, issued)
    np.testing.assert_array_equal(applied, np.full(B, sum(R.ROWS6)))
    es, ec = S.ipose_err(xg, Pg, xo, Po)
    print("B = %d against the oracle: state %.3g sigma, covariance %.3g" % (B, es, ec))
    assert es < TOL and ec < TOL, (es, ec)
    # the handle's reference is the last epoch's, as after the single calls
    np.testing.assert_array_equal(f.get_corrected_pose(), g.get_corrected_pose())
    assert (f.get_corrected_pose()[:, :3] != make(B, right).get_corrected_pose()[:, :3]).any()


# ---- 2. shared against per-instance inputs ---------------------------------------
@SIDES
def test_shared_against_per_instance_inputs(right):
    B = 5
    log = recorded(B, shared_marker=True)
    assert log["feature_cov"] is None and log["marker_pose"] is None
    per = R.per_instance(log)
    assert per["shared_feature_cov"] is None and per["shared_marker_pose"] is None
    f, g = make(B, right), make(B, right)
    f.run_log(f.upload_log(log))
    g.run_log(g.upload_log(per))
    same(snap(f), snap(g))
    assert not f.get_status().any()
    h = make(B, right)
    play_ipose_log(h, log)
    same(snap(f), snap(h))
    # differing per-instance covariances: the oracle
    log = recorded(B, fcov=S.per_instance_fcov(B, 4))
    assert log["feature_cov"] is not None and (log["feature_cov"][0, 0] != log["feature_cov"][0, 1]).any()
    with O.so3_side(right):
        o = R.init(O.OracleIndirectPoseBatch(B), B)
        play_ipose_log(o, log)
    f = make(B, right)
    f.run_log(f.upload_log(log))
    assert not f.get_status().any()
    es, ec = S.ipose_err(*f.get_state(), *o.get_state())
    assert es < TOL and ec < TOL, (es, ec)


# ---- 3. adjacent ranges and the launch boundary ----------------------------------
def test_adjacent_ranges_and_the_launch_boundary():
    """4100 epochs: more than one 4096-epoch launch, visual rows on both sides of the boundary"""
    B, E = 3, 4100
    rows = np.zeros(E, int)
    rows[[0, 7, 2000, 4095, 4096, 4099]] = 1
    log = recorded(B, rows=tuple(rows), dts=(0.01,))
    assert log["epochs"] == E and log["pose_ref"].shape == (E, B, 7) and log["dt"] == 0.01
    whole = make(B)
    ap = counter(whole)
    whole.run_log(whole.upload_log(log), applied=ap)
    np.testing.assert_array_equal(counts(whole, ap), np.full(B, 6))
    assert not whole.get_status().any()
    for cut in (1, 4096, 4097):
        f = make(B)
        d = f.upload_log(log)
        f.run_log(d, 0, cut, sync=False)
        f.run_log(d, cut, E - cut)
        same(snap(f), snap(whole))
        np.testing.assert_array_equal(f.get_corrected_pose(), whole.get_corrected_pose())


# ---- 4. track records ------------------------------------------------------------
def test_track_records():
    B, E = 5, 7
    log = recorded(B, rows=(0, 1, 2, 1, 0, 2, 1))
    assert log["epochs"] == E
    g = make(B)
    cuts = []
    for e in range(E):
        play_ipose_log(g, log, e, 1)
        if (e + 1) % 2 == 0:
            cuts.append(g.get_state() + (g.get_corrected_pose(),))
    assert len(cuts) == 3
    f = make(B)
    d = f.upload_log(log)
    mean, var, corr = f.run_log(d, every=2)
    assert mean.shape == (3, B, 7) and var.shape == (3, B, 6) and corr.shape == (3, B, 7)
    for k, (x, P, c) in enumerate(cuts):
        np.testing.assert_array_equal(mean[k], x)
        np.testing.assert_array_equal(var[k], np.diagonal(P, axis1=1, axis2=2))
        # the bound of include/uwvk.h: about ten rounded products of magnitude <= |t_ref| + 4 |p_err|
        # per translation component, four products of unit quaternions per quaternion component
        ref = log["pose_ref"][2 * k + 1]
        bt = 32 * EPS * (np.abs(ref[:, :3]).max(axis=1) + 4 * np.abs(x[:, :3]).max(axis=1))
        et, eq = np.abs(corr[k][:, :3] - c[:, :3]), np.abs(corr[k][:, 3:] - c[:, 3:])
        print("record %d: corrected translation %.3g of its bound, quaternion %.3g eps" %
              (k, (et / bt[:, None]).max(), eq.max() / EPS))
        assert (et <= bt[:, None]).all() and (eq <= 16 * EPS).all()
        # not the reference alone: a record that copied pose_ref is further off than the bound
        assert (np.abs(corr[k][:, :3] - ref[:, :3]).max(axis=1) > bt).all()
        assert (np.abs(corr[k][:, 3:] - ref[:, 3:]).max(axis=1) > 16 * EPS).all()
    same(snap(f), snap(g))
    # each buffer switched off in turn
    for off in ("mean", "variance", "corrected"):
        h = make(B)
        out = h.run_log(d, every=2, **{off: False})
        for name, got, want in zip(("mean", "variance", "corrected"), out, (mean, var, corr)):
            if name == off:
                assert got is None
            else:
                np.testing.assert_array_equal(got, want)
        same(snap(h), snap(f))
    # records of adjacent calls are the records of one call
    h = make(B)
    a = h.run_log(d, 0, 3, every=2)
    b = h.run_log(d, 3, 4, every=2)
    assert len(a[0]) == 1 and len(b[0]) == 2
    for u, v, w in zip(a, b, (mean, var, corr)):
        np.testing.assert_array_equal(np.concatenate([u, v]), w)


# ---- 5. per-instance skips --------------------------------------------------------
def skip_log(B=5):
    """four epochs, a row each, per-instance covariances and marker poses"""
    log = recorded(B, rows=(1, 1, 1, 1), fcov=S.per_instance_fcov(B, 4))
    assert log["feature_cov"] is not None and log["marker_pose"] is not None
    return log


_CLEAN = {}


def clean_run(B=5):
    if B not in _CLEAN:
        f = make(B)
        f.run_log(f.upload_log(skip_log(B)))
        assert not f.get_status().any()
        _CLEAN[B] = snap(f)
    return _CLEAN[B]


@pytest.mark.parametrize("what, row, j, value", [("features", 1, 2, np.nan), ("feature_cov", 2, 0, np.inf),
                                                 ("marker_pose", 1, 4, np.nan)])
def test_non_finite_payload_skips_the_row_for_that_instance(what, row, j, value):
    B = 5
    log = skip_log(B)
    log[what][row, j].reshape(-1)[-2] = value
    f, g, issued, applied = run_and_play(log)
    others = np.arange(B) != j
    same(snap(f)[:2], snap(g)[:2])          # the single calls with j masked out at that row
    same(snap(f), clean_run(B), others)     # the others: the clean run
    assert (snap(f)[0][j] != clean_run(B)[0][j]).any()
    st = f.get_status()
    assert st[j] == NAN and not st[others].any(), st
    np.testing.assert_array_equal(applied, issued)
    np.testing.assert_array_equal(applied, np.where(others, 4, 3))


def test_non_finite_reference_keeps_the_last_finite_one():
    B, j = 5, 1
    log = skip_log(B)
    log["pose_ref"][2, j, 5] = np.nan
    log["pose_ref"][3, j, 0] = np.inf
    f, g, issued, applied = run_and_play(log)   # play gives j the reference of epoch 1 at epochs 2 and 3
    others = np.arange(B) != j
    same(snap(f)[:2], snap(g)[:2])
    same(snap(f), clean_run(B), others)
    assert (snap(f)[0][j] != clean_run(B)[0][j]).any()
    st = f.get_status()
    assert st[j] == NAN and not st[others].any(), st
    np.testing.assert_array_equal(applied, np.full(B, 4))   # the predicts and the rows still ran
    # the stored reference: epoch 1's for j, the last epoch's for the others (what play set on g)
    np.testing.assert_array_equal(f.get_corrected_pose(), g.get_corrected_pose())
    h = make(B)
    h.run_log(h.upload_log(skip_log(B)))
    differs = (f.get_corrected_pose()[:, :3] != h.get_corrected_pose()[:, :3]).any(axis=1)
    np.testing.assert_array_equal(differs, ~others)


# ---- 6. UWVK_ST_NOTPD ---------------------------------------------------------------
def test_failed_visual_row_is_discarded_as_a_whole():
    """instance j's third feature has a negative pixel variance at row 0 (the
    input of test_ipose_visual_notpd_from_inputs: Sigma - C K^T indefinite, the
    re-spread fails): status words only, nothing here can fault"""
    B, j = 5, 3
    healthy = recorded(B, rows=(1, 0, 1), fcov=S.per_instance_fcov(B, 4))
    log = R.copy_log(healthy)
    log["feature_cov"][0, j, 2] = (-0.01 * np.eye(2)).reshape(4)
    others = np.arange(B) != j
    f, g, issued, applied = run_and_play(log)
    same(snap(f), snap(g))  # the status words too: the single call discards the row in the same way
    st = f.get_status()
    assert st[j] == NOTPD and not st[others].any(), st
    np.testing.assert_array_equal(applied, np.where(others, 2, 1))
    h = make(B)
    h.run_log(h.upload_log(healthy))
    same(snap(f), snap(h), others)
    # after epoch 0, j is where its predict alone left it; the later epochs still change it
    a, p = make(B), make(B)
    a.run_log(a.upload_log(log), 0, 1)
    p.predict(R.DTS6[0])
    same(a.get_state(), p.get_state(), j)
    assert a.get_status()[j] == NOTPD
    assert (f.get_state()[0][j] != a.get_state()[0][j]).any() and (f.get_state()[1][j] != a.get_state()[1][j]).any()


@SIDES
def test_failed_predict_leaves_the_state_and_the_run_carries_on(right):
    """instance j's Sigma is driven indefinite before the run (_ipose_with_indefinite's
    negative-Q predict): every step of j fails its Cholesky, raises UWVK_ST_NOTPD and
    leaves (mu, Sigma); status words only, nothing here can fault"""
    c, j = IPoseCase(9, right), 5
    log = recorded(c.K, rows=(0, 1, 0))
    bad, bad2, healthy = (_ipose_with_indefinite(c, IndirectPoseUKFBatch, j, "last", b) for b in (True, True, False))
    before = bad.get_state()
    assert not bad.get_status().any()
    others = np.arange(c.K) != j
    ap = counter(bad)
    bad.run_log(bad.upload_log(log), applied=ap)
    play_ipose_log(bad2, log)
    healthy.run_log(healthy.upload_log(log))
    same(snap(bad), snap(bad2))
    st = bad.get_status()
    assert st[j] == NOTPD and not st[others].any(), st
    same(bad.get_state(), before, j)
    same(snap(bad), snap(healthy), others)
    assert (bad.get_state()[0][others] != before[0][others]).any()
    np.testing.assert_array_equal(counts(bad, ap), np.where(others, 1, 0))


# ---- 7. errors ---------------------------------------------------------------------
def test_errors_leave_everything_untouched():
    B = 2
    log = R.fault_log(B)
    f = make(B)
    before = snap(f)
    ap = counter(f)

    def refused(code, d, first, count, **kw):
        with pytest.raises(engine.UWVKError) as ei:
            f.run_log(d, first, count, applied=ap, **kw)
        assert ei.value.code == code, (ei.value.code, code)

    for name, mutate, first, count, code in R.FAULTS:
        d = f.upload_log(R.copy_log(log))  # the struct points into the host arrays it is given
        if mutate:
            mutate(d.s, d.host)
        print(name)
        refused(code, d, first, count)
    d = f.upload_log(log)
    refused(R.EINVAL, d, 0, 6, every=0)
    refused(R.EINVAL, d, 0, 6, every=2, capacity=2)
    refused(R.EINVAL, d, 0, 6, every=2, mean=False, variance=False, corrected=False)
    zero = engine.C.c_int64(0)
    assert f._fn("run_log")(f.h, None, zero, zero, None, None) == R.EINVAL  # a NULL log
    fresh = IndirectPoseUKFBatch(B)
    with pytest.raises(engine.UWVKError) as ei:
        fresh.run_log(fresh.upload_log(log))
    assert ei.value.code == R.ENOTINIT
    with pytest.raises(engine.UWVKError) as ei:
        fresh.run_log(fresh.upload_log(log), 0, 6, every=0)  # the track is checked before the state
    assert ei.value.code == R.EINVAL
    same(snap(f), before)
    assert not counts(f, ap).any()
    # a following good run is the run on a fresh handle
    f.run_log(d, applied=ap)
    g = make(B)
    g.run_log(g.upload_log(log))
    same(snap(f), snap(g))
    assert (snap(f)[0] != before[0]).any()
    np.testing.assert_array_equal(counts(f, ap), np.full(B, 6))
