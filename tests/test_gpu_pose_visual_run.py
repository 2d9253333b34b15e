"""Visual-landmark rows in run_log (uwvk_pose_run_log_visual): one launch per
visual epoch runs all of its rows with the augmented (mu, Sigma) in LDS
(k_pose_visual_run).  The contract: bitwise what the run gives cut after every
event epoch, with at each cut the single calls XY -> Z -> Geographic -> delayed
XY -> one uwvk_pose_update_visual_landmark per row (mask = the instances whose
payload of that row is finite, the shared arrays passed as shared) and then the
latches; on the pair path, the one-instance path, both DOFs, both SO3 sides and
a dense handle; alone, with fixes, a delayed arrival, a latch and a track on one
epoch, and over split ranges; and the oracle, to the tolerance
tests/test_small_filters.py::test_gpu_pose_visual_landmark holds the single
call to.

Common shape (tests/pose_visual_run_scenes.py, validated on the CPU by
tests/test_pose_visual_run_scenes.py): 24 epochs, visual rows at epochs 5 (one),
11 (two), 12 (one) and 23 (one, the last epoch); 4 features."""
import functools

import numpy as np
import pytest

import pose_visual_run_scenes as R
from helpers import cov_err, state_err
from test_gpu_delayed import _delayed_at, make_delayed
from test_gpu_fixes import XY, Z, _handle, _update_at, make_fixes

pytestmark = pytest.mark.gpu

TOL = 1e-9  # tests/test_small_filters.py::test_gpu_pose_visual_landmark
NOTPD_ST, NAN_ST = 0x1, 0x2  # UWVK_ST_NOTPD, UWVK_ST_NAN
NAMES = ("x", "P", "acc", "status", "applied", "pd", "pair")


@pytest.fixture(scope="module")
def eng():
    from uwvk import engine
    if not engine.device_available(0):
        pytest.fail("no gfx950 device / libuwvk.so not loadable: the HIP path is mandatory")
    return engine


def test_status_bits():
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uwvk.h")) as f:
        h = f.read()
    for name, bit in (("UWVK_ST_NAN", NAN_ST), ("UWVK_ST_NOTPD", NOTPD_ST)):
        assert int(re.search(r"#define %s (0x[0-9a-fA-F]+)u" % name, h).group(1), 16) == bit, name


def handle(eng, log, dof=53, right=True, dense=False):
    g = _handle(eng, log, dof, True, right)
    if dense:
        g.set_dense_sigma(True)
    return g


def same(got, ref, names=NAMES, rows=None):
    for k in names:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        if rows is not None and a.ndim and k not in ("pd", "pair"):
            a, b = (a[:, rows], b[:, rows]) if k in ("mean", "variance", "latched") else (a[rows], b[rows])
        np.testing.assert_array_equal(a, b, err_msg=k)


def by_cuts(eng, g, log, vis, fx=None, dl=None, records=(), first=0, end=None):
    """The cut run: plain run_log between the event epochs; at a cut the fixes
    and the delayed update as single calls, one update_visual per row of the
    epoch (mask: the instances with a finite payload of that row), then the
    latches (get_state), then the record."""
    B, E = log["gyro"].shape[1], log["epochs"]
    end = E if end is None else end
    dlog = g.upload_log(log)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    facc, dacc, applied = np.zeros((B, 3), np.uint32), np.zeros(B, np.uint32), np.zeros(B, np.uint32)
    off = vis["visual_offset"]
    ev = set(records)
    if fx is not None:
        ev |= {int(e) for e in np.flatnonzero(fx["flags"])}
    latched = None
    if dl is not None:
        latched = np.array(dl["latched"], dtype=np.float64)
        ev |= {int(e) for e in np.flatnonzero(dl["index"] >= 0)} | {int(L) for L in dl["latch_epoch"] if L >= 0}
    cuts = R.cuts_of(off, first, end, ev)
    xs, vs = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        g.run_log(dlog, a, b - a, accept_counts=acc)
        e = b - 1
        if fx is not None and fx["flags"][e]:
            _update_at(g, fx, e, None, facc)
        if dl is not None:
            _delayed_at(g, dl, e, latched, None, dacc)
        for r in range(off[e], off[e + 1]):
            mask = R.finite_mask(vis, r, B)
            args = list(R.row_args(vis, r, B))
            args[0] = np.where(mask[:, None, None].astype(bool), args[0], 0.0)  # (a masked instance's payload is not read)
            before = g.get_state()[0]
            g.update_visual(*args, mask=None if mask.all() else mask)
            applied += (g.get_state()[0] != before).any(1).astype(np.uint32)
        if dl is not None:
            for r in np.flatnonzero(dl["latch_epoch"] == e):
                latched[r] = g.get_state()[0][:, 0:2]
        if e in records:
            x, P = g.get_state()
            xs.append(x)
            vs.append(np.diagonal(P, axis1=1, axis2=2).copy())
    x, P = g.get_state()
    return dict(mean=np.array(xs), variance=np.array(vs), x=x, P=P, acc=acc.read(np.uint32, (B, 4)), facc=facc,
                dacc=dacc, latched=latched, applied=applied, status=g.get_status(), pd=g.param_block(),
                pair=g.pair_active())


def in_run(eng, g, log, vis, fx=None, dl=None, ranges=None, every=None):
    B = log["gyro"].shape[1]
    dlog = g.upload_log(log)
    dfx = None if fx is None else g.upload_fixes(fx, counts=True)
    ddl = None if dl is None else g.upload_delayed(dl, counts=True)
    dvis = g.upload_visual(vis, counts=True)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    out = {}
    ranges = [(0, log["epochs"])] if ranges is None else ranges
    if every is None:
        for a, n in ranges:
            g.run_log(dlog, a, n, accept_counts=acc, fixes=dfx, delayed=ddl, visual=dvis)
    else:
        tracks = [g.run_log_track(dlog, every, a, n, accept_counts=acc, fixes=dfx, delayed=ddl, visual=dvis)
                  for a, n in ranges]
        out = dict(epochs=np.concatenate([t.epochs for t in tracks]), mean=np.concatenate([t.mean() for t in tracks]),
                   variance=np.concatenate([t.variance() for t in tracks]))
    x, P = g.get_state()
    out.update(x=x, P=P, acc=acc.read(np.uint32, (B, 4)), status=g.get_status(), pd=g.param_block(),
               pair=g.pair_active(), applied=dvis.applied(g.stream))
    if dfx is not None:
        out["facc"] = dfx.accept_counts(g.stream)
    if ddl is not None:
        out.update(dacc=ddl.accept_counts(g.stream), latched=ddl.latched(g.stream))
    return out


# B, dof, SO3 right side, dense, (pair kernel, PD kernel) at the start
MAIN = [
    pytest.param(4, 53, True, False, (1, 1), id="pair"),
    pytest.param(3, 53, True, False, (0, 1), id="one_instance"),
    pytest.param(4, 26, True, False, (1, 0), id="dof26"),
    pytest.param(4, 53, False, False, (1, 1), id="pair_left"),
    pytest.param(4, 26, False, False, (1, 0), id="dof26_left"),
    pytest.param(4, 53, True, True, None, id="dense"),
]


@functools.lru_cache(maxsize=None)
def _main(eng, B, dof, right, dense):
    """(in-run result, cut-run result, kernels at the start) of the common scene; computed once, left unchanged."""
    sc = R.scene(B, dof, right)
    ga, gb = (handle(eng, sc["log"], dof, right, dense) for _ in range(2))
    start = (ga.pair_active(), ga.param_block())
    return in_run(eng, ga, sc["log"], sc["visual"]), by_cuts(eng, gb, sc["log"], sc["visual"]), start


@pytest.mark.parametrize("B,dof,right,dense,kernels", MAIN)
def test_visual_run_bitwise(eng, B, dof, right, dense, kernels):
    """mu, Sigma, status, accept_counts and applied against the cut run with
    single calls; every instance took all five rows; a visual epoch ends the
    parameter-decoupled kernels as the single call does."""
    got, ref, start = _main(eng, B, dof, right, dense)
    assert kernels is None or start == kernels
    same(got, ref)
    assert not got["status"].any() and np.isfinite(got["x"]).all() and np.isfinite(got["P"]).all()
    np.testing.assert_array_equal(got["applied"], [5] * B)
    assert got["pd"] == 0 and (got["pair"] == 1) == (dof == 26 and not dense)


@pytest.mark.parametrize("B,dof,right,dense,kernels", MAIN)
def test_visual_run_matches_oracle(eng, B, dof, right, dense, kernels):
    """The same run against the oracle's cut run, at the single call's tolerance."""
    got, _, _ = _main(eng, B, dof, right, dense)
    sc = R.scene(B, dof, right)
    es, ec = state_err(got["x"], sc["x"], sc["P"], dof).max(), cov_err(got["P"], sc["P"]).max()
    print("state err %.3g sigma, cov err %.3g" % (es, ec))
    assert es < TOL and ec < TOL, (es, ec)
    np.testing.assert_array_equal(got["acc"], sc["acc"])


def test_fix_arrival_visual_latch_and_record_on_one_epoch(eng):
    """Epoch 11: an XY and a Z fix, the arrival of the row latched at epoch 5,
    two visual rows, the latch of a second delayed row, and a record (every = 6):
    the records, `latched` and all counts are the cut run's, so the latch and the
    record saw the visual rows."""
    B = 4
    sc = R.scene(B)
    log, vis = sc["log"], sc["visual"]
    fx = make_fixes(log, [(11, XY | Z)])
    dl = make_delayed(log, [(5, 11), (11, 20)])
    got = in_run(eng, handle(eng, log), log, vis, fx, dl, every=6)
    ref = by_cuts(eng, handle(eng, log), log, vis, fx, dl, records=(5, 11, 17, 23))
    np.testing.assert_array_equal(got["epochs"], (5, 11, 17, 23))
    same(got, ref, ("mean", "variance", "facc", "dacc", "latched") + NAMES)
    assert not got["status"].any()
    np.testing.assert_array_equal(got["applied"], [5] * B)
    np.testing.assert_array_equal(got["dacc"], [2] * B)
    # row 1 latches at the record epoch 11: that record's position, after the epoch's two visual rows
    np.testing.assert_array_equal(got["latched"][1], got["mean"][1][:, 0:2])
    # and the visual rows moved it: without them the latch holds another position
    without = in_run(eng, handle(eng, log), log, dict(vis, visual_offset=np.zeros(25, np.int64)), fx, dl, every=6)
    assert np.abs(without["latched"][1] - got["latched"][1]).max() > 1e-6
    # split after the combined epoch, on one set of device objects
    two = in_run(eng, handle(eng, log), log, vis, fx, dl, ranges=[(0, 12), (12, 12)], every=6)
    same(two, ref, ("mean", "variance", "facc", "dacc", "latched") + NAMES)


def test_shared_and_per_instance_forms(eng):
    """The shared feature covariance and marker pose against the same values per instance."""
    B = 4
    sc = R.scene(B, shared_marker=True)
    log, vis = sc["log"], sc["visual"]
    shared = in_run(eng, handle(eng, log), log, vis)
    per = in_run(eng, handle(eng, log), log, R.per_instance(vis, B))
    same(shared, per)
    same(shared, by_cuts(eng, handle(eng, log), log, vis))
    np.testing.assert_array_equal(shared["applied"], [5] * B)
    assert not shared["status"].any()
    es, ec = state_err(shared["x"], sc["x"], sc["P"], 53).max(), cov_err(shared["P"], sc["P"]).max()
    assert es < TOL and ec < TOL, (es, ec)


@pytest.mark.parametrize("B", [4, 3])
def test_split_ranges(eng, B):
    """[0, 12) + [12, 24) on one DevicePoseVisual give bitwise [0, 24)."""
    sc = R.scene(B)
    whole, _, _ = _main(eng, B, 53, True, False)
    two = in_run(eng, handle(eng, sc["log"]), sc["log"], sc["visual"], ranges=[(0, 12), (12, 12)])
    same(two, whole)


def test_nan_pixel_skips_the_row_for_that_instance_only(eng):
    """A NaN pixel of instance 1 in the first row of epoch 11."""
    B, j = 4, 1
    sc = R.scene(B)
    log, vis = sc["log"], R.copy_visual(sc["visual"])
    r = int(vis["visual_offset"][11])
    vis["features"][r, j, 2, 1] = np.nan
    got = in_run(eng, handle(eng, log), log, vis)
    ref = by_cuts(eng, handle(eng, log), log, vis)
    assert ref["applied"][j] == 4 and not ref["status"].any()  # the masked single call raises nothing
    same(got, ref, ("x", "P", "acc", "applied", "pd", "pair"))
    np.testing.assert_array_equal(got["status"], [0, NAN_ST, 0, 0])
    np.testing.assert_array_equal(got["applied"], [5, 4, 5, 5])
    clean, _, _ = _main(eng, B, 53, True, False)
    others = np.arange(B) != j
    same(got, clean, ("x", "P", "acc", "applied"), rows=others)
    assert np.abs(got["x"][j] - clean["x"][j]).max() > 0 and np.isfinite(got["x"]).all()


def test_failed_row_is_discarded_and_the_next_row_still_runs(eng):
    """fcov = -0.01 I for one feature of instance 2 (the input of
    test_pose_visual_notpd_from_inputs) in the first of epoch 11's two rows: the
    update fails for that instance after an earlier feature has already changed
    Sigma in LDS; the row is discarded as a whole and the second row applied."""
    B, j = 4, 2
    sc = R.scene(B)
    log = sc["log"]
    vis = R.copy_visual(R.per_instance(sc["visual"], B))
    r = int(vis["visual_offset"][11])
    vis["feature_cov"][r, j, 1] = (-0.01 * np.eye(2)).reshape(4)
    got = in_run(eng, handle(eng, log), log, vis)
    ref = by_cuts(eng, handle(eng, log), log, vis)  # the failing single call: UWVK_ST_NOTPD, state untouched
    same(got, ref)
    np.testing.assert_array_equal(got["status"], [0, 0, NOTPD_ST, 0])
    np.testing.assert_array_equal(got["applied"], [5, 5, 4, 5])
    # instance 2 is the run with that row masked out for it: the second row of epoch 11 and the later rows applied
    skipped = R.copy_visual(R.per_instance(sc["visual"], B))
    skipped["features"][r, j] = np.nan
    masked = by_cuts(eng, handle(eng, log), log, skipped)
    same(got, masked, ("x", "P", "acc", "applied"))
    # the partner instances are the clean run
    clean, _, _ = _main(eng, B, 53, True, False)
    same(got, clean, ("x", "P", "acc", "applied"), rows=np.arange(B) != j)
    assert np.isfinite(got["x"]).all() and np.isfinite(got["P"]).all()


def test_failed_second_row_replays_the_first(eng):
    """The same input in the second of epoch 11's rows: when it fails, the first
    row's result is no longer in HBM, so the instance reloads the epoch's state
    and runs the first row again; that replay must give the first row's result
    bit for bit, which the cut run (a store after the first row) holds it to."""
    B, j = 4, 2
    sc = R.scene(B)
    log = sc["log"]
    vis = R.copy_visual(R.per_instance(sc["visual"], B))
    r = int(vis["visual_offset"][11]) + 1
    vis["feature_cov"][r, j, 1] = (-0.01 * np.eye(2)).reshape(4)
    got = in_run(eng, handle(eng, log), log, vis)
    same(got, by_cuts(eng, handle(eng, log), log, vis))
    np.testing.assert_array_equal(got["status"], [0, 0, NOTPD_ST, 0])
    np.testing.assert_array_equal(got["applied"], [5, 5, 4, 5])
    skipped = R.copy_visual(R.per_instance(sc["visual"], B))
    skipped["features"][r, j] = np.nan
    same(got, by_cuts(eng, handle(eng, log), log, skipped), ("x", "P", "acc", "applied"))
    clean, _, _ = _main(eng, B, 53, True, False)
    same(got, clean, ("x", "P", "acc", "applied"), rows=np.arange(B) != j)
    # the first row of epoch 11 was applied to instance 2: it is not the run with both rows masked out
    both = R.copy_visual(skipped)
    both["features"][r - 1, j] = np.nan
    assert np.abs(by_cuts(eng, handle(eng, log), log, both)["x"][j] - got["x"][j]).max() > 0


def test_more_rows_on_an_epoch_than_one_launch_takes(eng):
    """66 rows on one epoch run as two launches (64 + 2): bitwise the 66 single
    calls, with a failed row in the second launch (row 65 of instance 1)."""
    B, dof = 2, 26
    sc = R.many_rows_scene(B, dof)
    log, vis = sc["log"], sc["visual"]
    got = in_run(eng, handle(eng, log, dof), log, vis)
    same(got, by_cuts(eng, handle(eng, log, dof), log, vis))
    np.testing.assert_array_equal(got["applied"], [R.MANY_ROWS] * B)
    assert not got["status"].any()
    bad = R.copy_visual(R.per_instance(vis, B))
    bad["feature_cov"][65, 1, 0] = (-0.01 * np.eye(2)).reshape(4)
    got = in_run(eng, handle(eng, log, dof), log, bad)
    same(got, by_cuts(eng, handle(eng, log, dof), log, bad))
    np.testing.assert_array_equal(got["status"], [0, NOTPD_ST])
    np.testing.assert_array_equal(got["applied"], [R.MANY_ROWS, R.MANY_ROWS - 1])


def test_one_feature(eng):
    B = 4
    sc = R.scene(B, rows_at=((5, 1),), nf=1)
    log, vis = sc["log"], sc["visual"]
    got = in_run(eng, handle(eng, log), log, vis)
    same(got, by_cuts(eng, handle(eng, log), log, vis))
    np.testing.assert_array_equal(got["applied"], [1] * B)
    assert not got["status"].any()
    es, ec = state_err(got["x"], sc["x"], sc["P"], 53).max(), cov_err(got["P"], sc["P"]).max()
    assert es < TOL and ec < TOL, (es, ec)


def test_no_rows_is_run_log_delayed(eng):
    """A visual struct without a row in the range: bitwise uwvk_pose_run_log_delayed,
    the parameter-decoupled kernels kept; visual = NULL through the entry point too."""
    import ctypes as C
    B = 4
    sc = R.scene(B)
    log, vis = sc["log"], sc["visual"]
    fx, dl = make_fixes(log, [(3, XY)]), make_delayed(log, [(1, 4)])
    names = ("x", "P", "acc", "facc", "dacc", "latched", "status", "pd", "pair")

    def plain(a, n):
        g = handle(eng, log)
        dlog, dfx, ddl = g.upload_log(log), g.upload_fixes(fx, counts=True), g.upload_delayed(dl, counts=True)
        acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
        g.run_log(dlog, a, n, accept_counts=acc, fixes=dfx, delayed=ddl)
        x, P = g.get_state()
        return dict(x=x, P=P, acc=acc.read(np.uint32, (B, 4)), facc=dfx.accept_counts(g.stream),
                    dacc=ddl.accept_counts(g.stream), latched=ddl.latched(g.stream), status=g.get_status(),
                    pd=g.param_block(), pair=g.pair_active())

    ref = plain(0, 5)
    got = in_run(eng, handle(eng, log), log, vis, fx, dl, ranges=[(0, 5)])  # the first row is at epoch 5
    same(got, ref, names)
    assert got["pd"] == 1 and got["pair"] == 1 and not got["applied"].any()
    # no rows at all: no offsets, no arrays
    empty = dict(n_features=0, cov_marker_pose=np.zeros(36), camera=np.zeros(4), camera_in_imu=np.zeros(7))
    ref = plain(0, 24)
    got = in_run(eng, handle(eng, log), log, empty, fx, dl)
    same(got, ref, names)
    # visual = NULL
    g = handle(eng, log)
    dlog, dfx, ddl = g.upload_log(log), g.upload_fixes(fx, counts=True), g.upload_delayed(dl, counts=True)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    eng._chk(g.L.uwvk_pose_run_log_visual(g.h, C.byref(dlog.s), C.byref(dfx.s), C.byref(ddl.s), None, C.c_int64(0),
                                          C.c_int64(24), acc.ptr, None))
    g.synchronize()
    x, P = g.get_state()
    np.testing.assert_array_equal(x, ref["x"])
    np.testing.assert_array_equal(P, ref["P"])


def test_failing_check_queues_nothing(eng):
    """The check's code comes back first and the state is untouched."""
    B = 4
    sc = R.scene(B)
    log = sc["log"]
    g = handle(eng, log)
    dlog = g.upload_log(log)
    before = g.get_state()
    for field, value, code in (("camera", np.array([600.0, np.nan, 320.0, 240.0]), R.ENAN),
                               ("n_features", 0, R.EINVAL)):
        dvis = g.upload_visual(dict(sc["visual"], **{field: value}), counts=True)
        with pytest.raises(eng.UWVKError) as e:
            g.run_log(dlog, visual=dvis)
        assert e.value.code == code
        # a range without rows does not use the faulty input
        g2 = handle(eng, log)
        g2.run_log(g2.upload_log(log), 0, 5, visual=g2.upload_visual(dict(sc["visual"], **{field: value})))
    after = g.get_state()
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    assert g.param_block() == 1 and not g.get_status().any()
