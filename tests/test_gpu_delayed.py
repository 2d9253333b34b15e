"""Delayed XY fixes in run_log (uwvk_pose_run_log_delayed): each row's own XY
position is latched on the device after its latch epoch L and the delayed update
(k_psp_fix's fourth kind) runs at its arrival epoch A with that position.  The
contract: bitwise what uwvk_pose_run_log gives cut after every latch, fix and
arrival epoch, with at each cut the single calls XY -> Z -> Geographic ->
uwvk_pose_update_delayed_xy (delayed_xy the x[:, 0:2] uwvk_pose_get_state
returned at the row's latch cut) and then the latches; on every path run_log
has, alone, with the track and over split ranges; and the oracle advanced
piecewise, to the tolerance of the track's oracle test.

Shapes, fixes and per-instance offsets are those of test_gpu_fixes.py."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_fixes import (GEO, ORACLE_PLAN, PATHS, PLAN, XY, Z, _handle, _same, _update_at, make_fixes,
                            oracle_case_fixes)

pytestmark = pytest.mark.gpu

# (latch epoch, arrival epoch) per payload row: an arrival on an XY epoch (30) and on the XY|Z|GEO epoch (59), a
# latch one epoch before a fix epoch (58), two rows in flight at once, two rows sharing a latch epoch (89), an
# arrival on the last epoch
ROWS = [(9, 30), (31, 59), (58, 60), (70, 90), (80, 100), (89, 110), (89, 119)]
COV = np.diag([0.05 ** 2, 0.06 ** 2])
NAMES = ("x", "P", "acc", "facc", "dacc", "latched", "status", "pd", "pair")


@pytest.fixture(scope="module")
def eng():
    from uwvk import engine
    if not engine.device_available(0):
        pytest.fail("no gfx950 device / libuwvk.so not loadable: the HIP path is mandatory")
    return engine


def make_delayed(log, rows, filled=None):
    """The delayed dict of DevicePoseDelayed for rows = [(L, A), ...]: each value
    is the truth XY after epoch L plus make_fixes' per-instance XY offsets.
    filled: {row: (value epoch, latched [batch][2])} for caller-filled rows (L = -1)."""
    B, E = log["gyro"].shape[1], log["epochs"]
    b = np.arange(B)
    off_xy = np.stack([0.03 * ((b % 3) - 1), 0.02 * ((b % 4) - 1.5)], 1)
    filled = filled or {}
    d = dict(index=np.full(E, -1, np.int32), latch_epoch=np.array([L for L, _ in rows], np.int32), xy_cov=COV.copy(),
             xy=np.empty((len(rows), B, 2)), latched=np.zeros((len(rows), B, 2)))
    for r, (L, A) in enumerate(rows):
        at = filled[r][0] if L < 0 else L
        d["xy"][r] = log["truth"].pos[at + 1][None, :2] + off_xy
        if L < 0:
            d["latched"][r] = filled[r][1]
        d["index"][A] = r
    return d


def _no_fixes(log):
    return dict(flags=np.zeros(log["epochs"], np.uint32))


def _delayed_at(h, dl, e, latched, masks=None, dacc=None):
    """The single call of the row arriving at epoch e, delayed_xy from `latched`."""
    r = dl["index"][e]
    if r < 0:
        return
    mu, lt, kw = dl["xy"][r].copy(), latched[r].copy(), {}
    if masks is not None and e in masks:  # a non-finite sample: that instance masked out
        kw["mask"] = masks[e]
        mu[~kw["mask"].astype(bool)] = 0.0
        lt[~kw["mask"].astype(bool)] = 0.0
    acc = h.update("delayed_xy", mu, dl["xy_cov"], extra=lt, **kw)
    if dacc is not None:
        dacc += acc


def _events(fx, dl, first, end):
    ev = {e for e in np.flatnonzero(fx["flags"]) if first <= e < end}
    ev |= {e for e in np.flatnonzero(dl["index"] >= 0) if first <= e < end}
    ev |= {int(L) for L in dl["latch_epoch"] if first <= L < end}
    return ev


def _by_cuts(eng, g, log, fx, dl, records=(), masks=None):
    """run_log cut after every fix, arrival, latch and record epoch: at a cut
    the fixes and the delayed update as host calls, then the latches (get_state),
    then the record."""
    B, E = log["gyro"].shape[1], log["epochs"]
    dlog = g.upload_log(log)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    facc, dacc = np.zeros((B, 3), np.uint32), np.zeros(B, np.uint32)
    latched = np.array(dl["latched"], dtype=np.float64)
    cuts = sorted({0, E} | {e + 1 for e in _events(fx, dl, 0, E)} | {e + 1 for e in records})
    xs, vs = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        g.run_log(dlog, a, b - a, accept_counts=acc)
        if fx["flags"][b - 1]:
            _update_at(g, fx, b - 1, None, facc)
        _delayed_at(g, dl, b - 1, latched, masks, dacc)
        for r in np.flatnonzero(dl["latch_epoch"] == b - 1):
            latched[r] = g.get_state()[0][:, 0:2]
        if b - 1 in records:
            x, P = g.get_state()
            xs.append(x)
            vs.append(np.diagonal(P, axis1=1, axis2=2).copy())
    x, P = g.get_state()
    return dict(mean=np.array(xs), variance=np.array(vs), x=x, P=P, acc=acc.read(np.uint32, (B, 4)), facc=facc,
                dacc=dacc, latched=latched, status=g.get_status(), pd=g.param_block(), pair=g.pair_active())


def _in_run(eng, g, log, fx, dl, ranges=None, every=None, no_fixes=False):
    B = log["gyro"].shape[1]
    dlog = g.upload_log(log)
    dfx = None if no_fixes else g.upload_fixes(fx, counts=True)
    ddl = None if dl is None else g.upload_delayed(dl, counts=True)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    out = {}
    ranges = [(0, log["epochs"])] if ranges is None else ranges
    if every is None:
        for a, n in ranges:
            g.run_log(dlog, a, n, accept_counts=acc, fixes=dfx, delayed=ddl)
    else:
        tracks = [g.run_log_track(dlog, every, a, n, accept_counts=acc, fixes=dfx, delayed=ddl) for a, n in ranges]
        out = dict(epochs=np.concatenate([t.epochs for t in tracks]), mean=np.concatenate([t.mean() for t in tracks]),
                   variance=np.concatenate([t.variance() for t in tracks]))
    x, P = g.get_state()
    out.update(x=x, P=P, acc=acc.read(np.uint32, (B, 4)), status=g.get_status(), pd=g.param_block(),
               pair=g.pair_active(), facc=np.zeros((B, 3), np.uint32) if dfx is None else dfx.accept_counts(g.stream))
    if ddl is not None:
        out.update(dacc=ddl.accept_counts(g.stream), latched=ddl.latched(g.stream))
    return out


@pytest.mark.parametrize("B,dof,pd,right,kernels", PATHS)
def test_delayed_bitwise(eng, B, dof, pd, right, kernels):
    """One run with fixes and delayed rows against the cut run; all seven rows
    accepted by every instance; the kernel pair of the start still holds."""
    from uwvk import synth
    log = synth.make_pose_log(B, 120, "C3", dof=dof)
    fx, dl = make_fixes(log, PLAN), make_delayed(log, ROWS)
    ga, gb, gn = (_handle(eng, log, dof, pd, right) for _ in range(3))
    assert (ga.pair_active(), ga.param_block()) == kernels
    got = _in_run(eng, ga, log, fx, dl)
    ref = _by_cuts(eng, gb, log, fx, dl)
    _same(got, ref, NAMES)
    assert (got["pair"], got["pd"]) == kernels
    assert not got["status"].any() and np.isfinite(got["x"]).all() and np.isfinite(got["latched"]).all()
    np.testing.assert_array_equal(got["dacc"], [7] * B)
    # the delayed rows were applied: the final position differs from the run with the fixes alone
    without = _in_run(eng, gn, log, fx, None)
    moved = np.abs(without["x"][:, :3] - got["x"][:, :3]).max()
    print("delayed rows move the final position by %.3g m" % moved)
    assert moved > 1e-3
    # every latched row is the run's own position, not the payload
    assert np.abs(got["latched"] - dl["xy"]).max() > 0


def test_delayed_bitwise_literal(eng):
    """The literal path: the fused launch of each epoch, k_pose_update per fix
    kind, k_pose_update<MK_DELAYED> on the latched device row, then the latch."""
    from uwvk import synth
    log = synth.make_pose_log(6, 12, "C3")
    fx = make_fixes(log, [(5, XY | Z | GEO), (11, GEO)])
    dl = make_delayed(log, [(0, 5), (5, 6), (6, 11)])
    ga, gb = (_handle(eng, log, literal=True) for _ in range(2))
    got = _in_run(eng, ga, log, fx, dl)
    ref = _by_cuts(eng, gb, log, fx, dl)
    _same(got, ref, NAMES)
    assert got["pd"] == 0 and not got["status"].any()
    np.testing.assert_array_equal(got["dacc"], [3] * 6)


def test_delayed_literal_with_track(eng):
    """The literal path with a track and events together: every = 6 puts the
    records on epoch 5 (three fixes, an arrival and a latch) and on epoch 11 (a
    fix and an arrival), each taken after all of its epoch's launches."""
    from uwvk import synth
    log = synth.make_pose_log(6, 12, "C3")
    fx = make_fixes(log, [(5, XY | Z | GEO), (11, GEO)])
    dl = make_delayed(log, [(0, 5), (5, 6), (6, 11)])
    ga, gb = (_handle(eng, log, literal=True) for _ in range(2))
    got = _in_run(eng, ga, log, fx, dl, every=6)
    ref = _by_cuts(eng, gb, log, fx, dl, records=(5, 11))
    np.testing.assert_array_equal(got["epochs"], (5, 11))
    _same(got, ref, ("mean", "variance") + NAMES)
    assert got["pd"] == 0 and not got["status"].any()
    np.testing.assert_array_equal(got["dacc"], [3] * 6)
    # row 1 latches on the record epoch 5: that record's position, after the epoch's fixes and arrival
    np.testing.assert_array_equal(got["latched"][1], got["mean"][0][:, 0:2])


def test_delayed_with_track_and_split_ranges(eng):
    """every = 30: one call and the calls [0, 60), [60, 120) on one
    DevicePoseDelayed give the cut run's records, state and counts.  Row (58, 60)
    is latched in the first call and applied in the second; rows (89, .) latch on
    a record epoch."""
    from uwvk import synth
    log = synth.make_pose_log(6, 120, "C3")
    fx, dl = make_fixes(log, PLAN), make_delayed(log, ROWS)
    ga, gb, gc = (_handle(eng, log) for _ in range(3))
    rec = (29, 59, 89, 119)
    ref = _by_cuts(eng, gb, log, fx, dl, records=rec)
    names = ("mean", "variance") + NAMES
    one = _in_run(eng, ga, log, fx, dl, every=30)
    np.testing.assert_array_equal(one["epochs"], rec)
    _same(one, ref, names)
    two = _in_run(eng, gc, log, fx, dl, ranges=[(0, 60), (60, 60)], every=30)
    np.testing.assert_array_equal(two["epochs"], rec)
    _same(two, ref, names)
    # the latch of a record epoch is that record's position
    np.testing.assert_array_equal(one["latched"][5], one["mean"][2][:, 0:2])
    np.testing.assert_array_equal(one["latched"][6], one["mean"][2][:, 0:2])
    # untracked split ranges too (the reference without the record cuts: a cut is not bitwise neutral)
    three = _in_run(eng, _handle(eng, log), log, fx, dl, ranges=[(0, 60), (60, 60)])
    _same(three, _by_cuts(eng, _handle(eng, log), log, fx, dl), NAMES)


def test_equivalences(eng):
    """delayed = NULL is run_log_fixes; a DevicePoseDelayed without events too;
    fixes = NULL with delayed rows only; a caller-filled row (L = -1) is the
    single call with that position."""
    from uwvk import synth
    B, E = 6, 60
    log = synth.make_pose_log(B, E, "C3")
    fx = make_fixes(log, [(10, XY), (29, Z | GEO)])
    names = ("x", "P", "acc", "facc", "status", "pd", "pair")
    ref = _in_run(eng, _handle(eng, log), log, fx, None)
    # delayed = NULL through the new entry point
    g = _handle(eng, log)
    dlog, dfx = g.upload_log(log), g.upload_fixes(fx, counts=True)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    eng._chk(g.L.uwvk_pose_run_log_delayed(g.h, C.byref(dlog.s), C.byref(dfx.s), None, C.c_int64(0), C.c_int64(E),
                                           acc.ptr, None))
    g.synchronize()
    x, P = g.get_state()
    _same(dict(x=x, P=P, acc=acc.read(np.uint32, (B, 4)), facc=dfx.accept_counts(g.stream), status=g.get_status(),
               pd=g.param_block(), pair=g.pair_active()), ref, names)
    # rows present, no event: nothing arrives, every row caller-filled
    dl = make_delayed(log, [(20, 40)])
    dl["index"][:] = -1
    dl["latch_epoch"][:] = -1
    got = _in_run(eng, _handle(eng, log), log, fx, dl)
    _same(got, ref, names)
    assert not got["dacc"].any() and not got["latched"].any()
    # n = 0, no arrays at all
    got = _in_run(eng, _handle(eng, log), log, fx,
                  dict(index=np.full(E, -1, np.int32), latch_epoch=np.zeros(0, np.int32), xy=np.zeros((0, B, 2)),
                       xy_cov=COV))
    _same(got, ref, names)
    # fixes = NULL, delayed rows only
    dl = make_delayed(log, [(5, 20), (20, 59)])
    got = _in_run(eng, _handle(eng, log), log, None, dl, no_fixes=True)
    cut = _by_cuts(eng, _handle(eng, log), log, _no_fixes(log), dl)
    _same(got, cut, NAMES)
    np.testing.assert_array_equal(got["dacc"], [2] * B)
    # a caller-filled row: the reference's literal call form
    pos = log["truth"].pos[31][None, :2] + 0.1 * np.arange(B)[:, None] * np.array([1.0, -1.0])
    dl = make_delayed(log, [(-1, 40)], filled={0: (30, pos)})
    got = _in_run(eng, _handle(eng, log), log, fx, dl)
    gs = _handle(eng, log)
    cut = _by_cuts(eng, gs, log, fx, dl)
    _same(got, cut, NAMES)
    np.testing.assert_array_equal(got["latched"][0], pos)  # never written by the run
    np.testing.assert_array_equal(got["dacc"], [1] * B)
    assert np.abs(got["x"][:, :2] - ref["x"][:, :2]).max() > 1e-3


def test_non_finite_samples_are_skipped_per_instance(eng):
    """Instance 2's value of the row arriving at epoch 59 is NaN; instance 4's
    caller-filled latched entry of the row arriving at epoch 100 is NaN: only
    they skip that row (they still take epoch 59's other fixes), carry
    UWVK_ST_NAN and count one less; the others are bitwise the clean run."""
    from uwvk import synth
    B = 6
    log = synth.make_pose_log(B, 120, "C3")
    fx = make_fixes(log, PLAN)
    rows = list(ROWS)
    rows[4] = (-1, 100)
    filled = {4: (80, log["truth"].pos[81][None, :2] + np.zeros((B, 1)))}
    clean = _in_run(eng, _handle(eng, log), log, fx, make_delayed(log, rows, filled))
    assert not clean["status"].any()
    np.testing.assert_array_equal(clean["dacc"], [7] * B)
    dl = make_delayed(log, rows, filled)
    dl["xy"][1, 2, 1] = np.nan
    dl["latched"][4, 4, 0] = np.inf
    m59, m100 = np.ones(B, np.uint8), np.ones(B, np.uint8)
    m59[2], m100[4] = 0, 0
    got = _in_run(eng, _handle(eng, log), log, fx, dl)
    ref = _by_cuts(eng, _handle(eng, log), log, fx, dl, masks={59: m59, 100: m100})
    _same(got, ref, ("x", "P", "acc", "facc", "dacc", "pd", "pair"))
    np.testing.assert_array_equal(got["latched"][4], dl["latched"][4])  # the caller's row, untouched
    want = np.zeros(B, np.uint32)
    want[[2, 4]] = 0x2  # UWVK_ST_NAN
    np.testing.assert_array_equal(got["status"], want)
    assert not ref["status"].any()
    np.testing.assert_array_equal(got["dacc"], [7, 7, 6, 7, 6, 7])
    others = [0, 1, 3, 5]
    np.testing.assert_array_equal(got["x"][others], clean["x"][others])
    np.testing.assert_array_equal(got["P"][others], clean["P"][others])
    assert np.isfinite(got["x"]).all() and np.isfinite(got["P"]).all()
    for i in (2, 4):
        assert np.abs(got["x"][i] - clean["x"][i]).max() > 0


def test_non_finite_latched_row_literal(eng):
    """The literal path checks the latched row as well."""
    from uwvk import synth
    B = 6
    log = synth.make_pose_log(B, 12, "C3")
    fx = _no_fixes(log)
    filled = {0: (2, log["truth"].pos[3][None, :2] + np.zeros((B, 1)))}
    dl = make_delayed(log, [(-1, 8)], filled)
    dl["latched"][0, 3, 1] = np.nan
    mask = np.ones(B, np.uint8)
    mask[3] = 0
    got = _in_run(eng, _handle(eng, log, literal=True), log, fx, dl)
    ref = _by_cuts(eng, _handle(eng, log, literal=True), log, fx, dl, masks={8: mask})
    _same(got, ref, ("x", "P", "acc", "dacc", "pd", "pair"))
    np.testing.assert_array_equal(got["status"], [0, 0, 0, 0x2, 0, 0])
    np.testing.assert_array_equal(got["dacc"], [1, 1, 1, 0, 1, 1])
    assert np.isfinite(got["x"]).all()


def test_delayed_arguments(eng):
    """Every UWVK_EINVAL case leaves the state, the status and `latched` untouched."""
    from uwvk import abi, synth
    B, E = 6, 60
    log = synth.make_pose_log(B, E, "C3")
    fx = make_fixes(log, [(10, XY), (59, XY | Z | GEO)])
    dl = make_delayed(log, [(5, 20), (20, 40), (30, 59)])
    dl["latched"][:] = 7.5
    g = _handle(eng, log)
    dlog, dfx, ddl = g.upload_log(log), g.upload_fixes(fx), g.upload_delayed(dl)
    x0, P0 = g.get_state()

    def call(s, first=0, count=E, track=None, fixes=dfx):
        return g.L.uwvk_pose_run_log_delayed(g.h, C.byref(dlog.s), C.byref(fixes.s) if fixes is not None else None,
                                             C.byref(s) if s is not None else None, C.c_int64(first),
                                             C.c_int64(count), None, track)

    def variant(**kw):
        s = abi.PoseDelayed.from_buffer_copy(ddl.s)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    keep = []

    def arr(a):
        keep.append(np.ascontiguousarray(a, dtype=np.int32))
        return keep[-1].ctypes.data

    def with_index(e, v):
        i = dl["index"].copy()
        i[e] = v
        return arr(i)

    def with_latch(r, v):
        L = dl["latch_epoch"].copy()
        L[r] = v
        return arr(L)

    bad = dict(
        index_null=variant(index=None), latch_epoch_null=variant(latch_epoch=None), xy_null=variant(xy=None),
        latched_null=variant(latched=None), n_negative=variant(n=-1),
        index_below=variant(index=with_index(7, -2)), index_past=variant(index=with_index(7, 3)),
        index_far=variant(index=with_index(59, 1 << 20)), rows_gone=variant(n=2),
        latch_below=variant(latch_epoch=with_latch(1, -2)), latch_past=variant(latch_epoch=with_latch(1, E)),
        latch_at_arrival=variant(latch_epoch=with_latch(1, 40)), latch_after_arrival=variant(latch_epoch=with_latch(0, 33)),
    )
    for name, s in bad.items():
        assert call(s) == 1, name  # UWVK_EINVAL
        x, P = g.get_state()
        np.testing.assert_array_equal(x, x0, err_msg=name)
        np.testing.assert_array_equal(P, P0, err_msg=name)
        np.testing.assert_array_equal(ddl.latched(), dl["latched"], err_msg=name)
    assert not g.get_status().any()
    # index and arrival order are checked over [first, first + count) only; the other errors stay
    assert call(variant(index=with_index(50, 99)), 0, 0) == 0
    assert call(variant(latch_epoch=with_latch(1, 40)), 0, 0) == 0
    assert call(variant(index=with_index(50, 99)), 50, 1) == 1
    assert call(variant(latch_epoch=with_latch(1, 40)), 40, 1) == 1
    assert call(variant(latch_epoch=with_latch(1, E)), 0, 0) == 1  # every row's latch epoch, whatever the range
    assert call(ddl.s, 0, E + 1) == 1
    assert call(ddl.s, 0, E, fixes=g.upload_fixes(dict(fx, flags=np.where(np.arange(E) == 3, 0x8, 0)))) == 1
    tr = abi.PoseTrack()
    tr.every = 0
    assert call(ddl.s, 0, E, C.byref(tr)) == 1
    g.synchronize()
    np.testing.assert_array_equal(g.get_state()[1], P0)
    np.testing.assert_array_equal(ddl.latched(), dl["latched"])


def oracle_by_cuts(o, log, fx, dl, records):
    """The oracle advanced piecewise, or_pose_update_delayed_xy on its own latched positions."""
    B, E = log["gyro"].shape[1], log["epochs"]
    acc = np.zeros((B, 4), np.uint32)
    facc, dacc = np.zeros((B, 3), np.uint32), np.zeros(B, np.uint32)
    latched = np.zeros((len(dl["xy"]), B, 2))
    cuts = sorted({0, E} | {e + 1 for e in _events(fx, dl, 0, E)} | {e + 1 for e in records})
    states = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        acc += o.run_log(log, a, b - a, nthreads=B)
        if fx["flags"][b - 1]:
            _update_at(o, fx, b - 1, None, facc)
        _delayed_at(o, dl, b - 1, latched, None, dacc)
        for r in np.flatnonzero(dl["latch_epoch"] == b - 1):
            latched[r] = o.get_state()[0][:, 0:2]
        if b - 1 in records:
            states.append(o.get_state())
    return dict(states=states, acc=acc, facc=facc, dacc=dacc, latched=latched)


# one arrives on the BodyEfforts epoch 399, one is latched there, one is latched on the record epoch 599, two share
# the latch epoch 700, one arrives on a fix epoch (860)
ORACLE_ROWS = [(30, 110), (150, 399), (399, 470), (480, 560), (599, 640), (700, 760), (700, 810), (820, 860)]


@pytest.mark.parametrize("dof", [53, 26])
def test_delayed_match_oracle(eng, dof):
    """The compressed C4 log and fixes of test_fixes_match_oracle with eight
    delayed rows: every record and the final state against the oracle advanced
    piecewise, to that test's tolerance; counts equal."""
    from helpers import init_both, state_err
    import oracle_ctypes as orc
    from uwvk import abi, synth
    B, E, every = 6, 900, 100
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    log = synth.make_pose_log(B, E, "C4", dof=dof, dropout_on=0.4, dropout_off=0.1, adcp_every=150)
    fx, _ = oracle_case_fixes(log)
    dl = make_delayed(log, ORACLE_ROWS)
    assert log["flags"][399] & abi.EV_EFFORTS and (860, XY | GEO) in ORACLE_PLAN
    o, on = orc.OraclePoseBatch(B, dof), orc.OraclePoseBatch(B, dof)
    g = eng.PoseUKFBatch(B, dof)
    init_both(o, g, cfg, uwv, log)
    on.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    on.set_process_noise_from_config(cfg, 1e-3)
    got = _in_run(eng, g, log, fx, dl, every=every)
    rec = np.arange(every - 1, E, every)
    np.testing.assert_array_equal(got["epochs"], rec)
    ref = oracle_by_cuts(o, log, fx, dl, rec)
    for r, e in enumerate(rec):
        xo, Po = ref["states"][r]
        do = np.diagonal(Po, axis1=1, axis2=2)
        es = state_err(got["mean"][r], xo, Po, dof).max()
        ev = (np.abs(got["variance"][r] - do) / do).max()
        print("dof %d record %d (epoch %d): state %.3e variance %.3e" % (dof, r, e, es, ev))
        assert es < 1e-7 and ev < 1e-7, (r, es, ev)
    xo, Po = ref["states"][-1]
    assert state_err(got["x"], xo, Po, dof).max() < 1e-7
    np.testing.assert_array_equal(got["acc"], ref["acc"])
    np.testing.assert_array_equal(got["facc"], ref["facc"])
    np.testing.assert_array_equal(got["dacc"], ref["dacc"])
    assert ref["dacc"].min() > 0
    assert not got["status"].any()
    # teeth: the delayed rows move the oracle's final position by far more than the tolerance
    oracle_by_cuts(on, log, fx, make_delayed(log, []), rec)
    xn = on.get_state()[0]
    sd = np.sqrt(np.diagonal(Po, axis1=1, axis2=2)[:, :3])
    moved = (np.abs(xo[:, :3] - xn[:, :3]) / sd).max()
    print("dof %d: the delayed rows move the oracle's final position by %.3g sd" % (dof, moved))
    assert moved > 1e-7


def test_mission_replay_with_delayed(eng):
    """build_pose_log(delayed_xy=...) followed by replay equals the explicit upload path."""
    from uwvk import mission, synth
    B, E = 6, 60
    log = synth.make_pose_log(B, E, "C3")
    imu = np.arange(1, E + 1) * log["dt"]
    dref = make_delayed(log, [(5, 20), (20, 45)])
    m = mission.build_pose_log(B, imu, log["gyro"], log["acc"], log["acc_cov"],
                               xy=(imu[[10]], log["truth"].pos[11][None, :2], np.diag([0.01, 0.02])),
                               delayed_xy=(imu[[5, 20]], imu[[20, 45]], dref["xy"], COV))
    np.testing.assert_array_equal(m["delayed"]["latch_epoch"], [5, 20])
    np.testing.assert_array_equal(np.flatnonzero(m["delayed"]["index"] >= 0), [20, 45])
    for k in ("pos0", "pos_cov", "rot0", "rot_cov"):
        m[k] = log[k]
    g, r = _handle(eng, m), _handle(eng, m)
    out = mission.replay(g, m, 30)
    t = r.run_log_track(r.upload_log(m), 30, fixes=r.upload_fixes(m["fixes"]), delayed=r.upload_delayed(m["delayed"]))
    np.testing.assert_array_equal(out["mean"], t.mean())
    np.testing.assert_array_equal(out["variance"], t.variance())
    cut = _by_cuts(eng, _handle(eng, m), m, m["fixes"], dict(m["delayed"], latched=np.zeros((2, B, 2))),
                   records=(29, 59))
    np.testing.assert_array_equal(out["mean"], cut["mean"])
    np.testing.assert_array_equal(out["variance"], cut["variance"])
