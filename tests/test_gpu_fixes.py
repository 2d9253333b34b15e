"""Position fixes in run_log (uwvk_pose_run_log_fixes, k_psp_fix): XY, Z and GPS
fixes applied at their epochs inside a device-resident run, one fused launch
per fix epoch.  The contract: bitwise what uwvk_pose_run_log gives on each
segment between fix epochs with uwvk_pose_update_xy / _z / _geographic at each
cut (in that order), on every path run_log has, alone and with the track; and
the oracle advanced piecewise, to the tolerance of the track's oracle test.

Fix payloads are truth positions plus fixed per-instance offsets; GEO rows are
converted with the handle's location."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

XY, Z, GEO = 1, 2, 4
GPS_IN_BODY = (0.3, -0.1, 0.2)
KINDS = ((XY, "xy", "xy"), (Z, "z", "z"), (GEO, "geo", "geographic"))  # bit, fixes key, update kind


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


def make_fixes(log, plan, xy_sd=0.05, z_sd=0.05, geo_sd=0.5):
    """The fixes dict of DevicePoseFixes for plan = [(epoch, kinds mask), ...]:
    the truth position after that epoch plus fixed per-instance offsets."""
    from numpy_twin import nav_to_world
    from uwvk import synth
    B, E = log["gyro"].shape[1], log["epochs"]
    b = np.arange(B)
    off_xy = np.stack([0.03 * ((b % 3) - 1), 0.02 * ((b % 4) - 1.5)], 1)
    off_z = 0.04 * ((b % 2) - 0.5)
    off_geo = np.stack([0.1 * ((b % 2) - 0.5), 0.05 * ((b % 3) - 1)], 1)
    fx = dict(flags=np.zeros(E, np.uint32), gps_in_body=np.array(GPS_IN_BODY),
              xy_cov=np.diag([xy_sd ** 2, (1.2 * xy_sd) ** 2]), z_cov=np.array([z_sd ** 2]),
              geo_cov=np.array([[geo_sd ** 2, 0.01 * geo_sd ** 2], [0.01 * geo_sd ** 2, geo_sd ** 2]]))
    rows = {k: [] for _, k, _ in KINDS}
    for _, k, _ in KINDS:
        fx[k + "_index"] = np.full(E, -1, np.int32)
    for e, kinds in sorted(plan):
        p = log["truth"].pos[e + 1]
        fx["flags"][e] = kinds
        if kinds & XY:
            fx["xy_index"][e] = len(rows["xy"])
            rows["xy"].append(p[None, :2] + off_xy)
        if kinds & Z:
            fx["z_index"][e] = len(rows["z"])
            rows["z"].append(p[2] + off_z)
        if kinds & GEO:
            fx["geo_index"][e] = len(rows["geo"])
            lat, lon = nav_to_world((synth.LAT0, synth.LON0), p[0] + off_geo[:, 0], p[1] + off_geo[:, 1])
            rows["geo"].append(np.stack([lat, lon], 1))
    for _, k, _ in KINDS:
        fx[k] = np.array(rows[k]) if rows[k] else None
    return fx


def _update_at(h, fx, e, masks=None, counts=None):
    """The single-call updates of epoch e's fixes, XY -> Z -> Geographic."""
    for slot, (bit, k, kind) in enumerate(KINDS):
        if not fx["flags"][e] & bit:
            continue
        mu = np.array(fx[k][fx[k + "_index"][e]]).reshape(len(fx[k][0]), -1)  # [batch][m]
        kw = {}
        if masks is not None and (e, bit) in masks:  # a non-finite row: that instance masked out
            kw["mask"] = masks[(e, bit)]
            mu[~kw["mask"].astype(bool)] = 0.0
        if kind == "geographic":
            kw["extra"] = fx["gps_in_body"]
        acc = h.update(kind, mu, fx[k + "_cov"].reshape(1, 1) if k == "z" else fx[k + "_cov"], **kw)
        if counts is not None:
            counts[:, slot] += acc


def _by_cuts(eng, g, log, fx, first=0, count=None, records=(), masks=None):
    """run_log cut after every fix epoch (and every record epoch), the fixes as
    host updates at the cuts, the state read after each record epoch."""
    B, E = log["gyro"].shape[1], log["epochs"]
    end = E if count is None else first + count
    dlog = g.upload_log(log)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    facc = np.zeros((B, 3), np.uint32)
    cuts = sorted({first, end} | {e + 1 for e in np.flatnonzero(fx["flags"]) if first <= e < end} |
                  {e + 1 for e in records})
    xs, vs = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        g.run_log(dlog, a, b - a, accept_counts=acc)
        if fx["flags"][b - 1]:
            _update_at(g, fx, b - 1, masks, facc)
        if b - 1 in records:
            x, P = g.get_state()
            xs.append(x)
            vs.append(np.diagonal(P, axis1=1, axis2=2).copy())
    x, P = g.get_state()
    return dict(mean=np.array(xs), variance=np.array(vs), x=x, P=P, acc=acc.read(np.uint32, (B, 4)), facc=facc,
                status=g.get_status(), pd=g.param_block(), pair=g.pair_active())


def _with_fixes(eng, g, log, fx, ranges=None, every=None):
    B = log["gyro"].shape[1]
    dlog = g.upload_log(log)
    dfx = g.upload_fixes(fx, counts=True)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    out = {}
    ranges = [(0, log["epochs"])] if ranges is None else ranges
    if every is None:
        for a, n in ranges:
            g.run_log(dlog, a, n, accept_counts=acc, fixes=dfx)
    else:
        tracks = [g.run_log_track(dlog, every, a, n, accept_counts=acc, fixes=dfx) for a, n in ranges]
        out = dict(epochs=np.concatenate([t.epochs for t in tracks]), mean=np.concatenate([t.mean() for t in tracks]),
                   variance=np.concatenate([t.variance() for t in tracks]))
    x, P = g.get_state()
    out.update(x=x, P=P, acc=acc.read(np.uint32, (B, 4)), facc=dfx.accept_counts(g.stream), status=g.get_status(),
               pd=g.param_block(), pair=g.pair_active())
    return out


def _same(got, ref, names=("x", "P", "acc", "facc", "status", "pd", "pair")):
    for k in names:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


PLAN = [(0, XY), (30, XY), (59, XY | Z | GEO), (60, Z), (119, GEO)]

# B, dof, pd option, SO3 right side, (pair kernel, PD kernel) expected: the shapes of test_gpu_track.py::PATHS
PATHS = [
    pytest.param(6, 53, True, True, (1, 1), id="pair"),
    pytest.param(6, 53, True, False, (1, 1), id="pair_left"),
    pytest.param(5, 53, True, True, (0, 1), id="odd_batch_pd"),
    pytest.param(6, 26, True, True, (1, 0), id="dof26"),
    pytest.param(6, 53, False, True, (0, 0), id="general"),
]


@pytest.mark.parametrize("B,dof,pd,right,kernels", PATHS)
def test_fixes_bitwise(eng, B, dof, pd, right, kernels):
    """One run with fixes against run_log cut at the fix epochs with the
    single-call updates at the cuts; the kernel pair of the start still holds
    at the end (a fix does not couple the parameter block)."""
    from uwvk import synth
    log = synth.make_pose_log(B, 120, "C3", dof=dof)
    fx = make_fixes(log, PLAN)
    ga, gb, gn = (_handle(eng, log, dof, pd, right) for _ in range(3))
    assert (ga.pair_active(), ga.param_block()) == kernels
    got = _with_fixes(eng, ga, log, fx)
    ref = _by_cuts(eng, gb, log, fx)
    _same(got, ref)
    assert (got["pair"], got["pd"]) == kernels
    assert not got["status"].any()
    # the fixes were applied: XY and Z accept everything, GEO is gated
    np.testing.assert_array_equal(got["facc"][:, :2], [[3, 2]] * B)
    assert got["facc"][:, 2].max() > 0 and got["facc"][:, 2].max() <= 2
    gn.run_log(gn.upload_log(log))
    assert np.abs(gn.get_state()[0][:, :3] - got["x"][:, :3]).max() > 1e-3


def test_fixes_bitwise_literal(eng):
    """The literal path: the fused launch of each epoch, then k_pose_update per kind."""
    from uwvk import synth
    log = synth.make_pose_log(6, 12, "C3")
    fx = make_fixes(log, [(0, XY), (5, XY | Z | GEO), (6, Z), (11, GEO)])
    ga, gb = (_handle(eng, log, literal=True) for _ in range(2))
    got = _with_fixes(eng, ga, log, fx)
    ref = _by_cuts(eng, gb, log, fx)
    _same(got, ref)
    assert got["pd"] == 0 and not got["status"].any()
    np.testing.assert_array_equal(got["facc"][:, :2], [[2, 2]] * 6)


def test_fixes_with_track(eng):
    """every = 30 on the same log: the record of epoch 59 holds the state after
    that epoch's fixes; calls over adjacent ranges split at epoch 60 concatenate."""
    from uwvk import synth
    log = synth.make_pose_log(6, 120, "C3")
    fx = make_fixes(log, PLAN)
    ga, gb, gc = (_handle(eng, log) for _ in range(3))
    rec = (29, 59, 89, 119)
    ref = _by_cuts(eng, gb, log, fx, records=rec)
    names = ("mean", "variance", "x", "P", "acc", "facc", "status", "pd", "pair")
    one = _with_fixes(eng, ga, log, fx, every=30)
    np.testing.assert_array_equal(one["epochs"], rec)
    _same(one, ref, names)
    two = _with_fixes(eng, gc, log, fx, ranges=[(0, 60), (60, 60)], every=30)
    np.testing.assert_array_equal(two["epochs"], rec)
    _same(two, ref, names)
    # post-fix: the record differs from the state before epoch 59's fixes
    pre = _handle(eng, log)
    dl = pre.upload_log(log)
    for a, b in ((0, 1), (1, 31), (31, 60)):
        pre.run_log(dl, a, b - a)
        if b - 1 in (0, 30):
            _update_at(pre, fx, b - 1)
    x_pre = pre.get_state()[0]
    assert np.abs(one["mean"][1][:, :3] - x_pre[:, :3]).max() > 1e-3


@pytest.mark.parametrize("dof", [53, 26])
def test_fixes_match_oracle(eng, dof):
    """The compressed C4 log of test_track_all_events_match_oracle with ten fix
    epochs (one on the BodyEfforts epoch 399, one on a record epoch): every
    record and the final state against the oracle advanced piecewise, to that
    test's tolerance; one GEO row a kilometre off is rejected by both."""
    from helpers import init_both, state_err
    import oracle_ctypes as orc
    from uwvk import abi, synth
    B, E, every = 6, 900, 100
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    log = synth.make_pose_log(B, E, "C4", dof=dof, dropout_on=0.4, dropout_off=0.1, adcp_every=150)
    fx, want_geo = oracle_case_fixes(log)
    assert log["flags"][399] & abi.EV_EFFORTS
    o, on = orc.OraclePoseBatch(B, dof), orc.OraclePoseBatch(B, dof)
    g = eng.PoseUKFBatch(B, dof)
    init_both(o, g, cfg, uwv, log)
    on.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    on.set_process_noise_from_config(cfg, 1e-3)
    got = _with_fixes(eng, g, log, fx, every=every)
    rec = np.arange(every - 1, E, every)
    np.testing.assert_array_equal(got["epochs"], rec)
    ref = oracle_by_cuts(o, log, fx, rec)
    for r, e in enumerate(rec):
        xo, Po = ref["states"][r]
        do = np.diagonal(Po, axis1=1, axis2=2)
        es = state_err(got["mean"][r], xo, Po, dof).max()
        ev = (np.abs(got["variance"][r] - do) / do).max()
        print("dof %d record %d (epoch %d): state %.3e variance %.3e" % (dof, r, e, es, ev))
        assert es < 1e-7 and ev < 1e-7, (r, es, ev)
    np.testing.assert_array_equal(got["acc"], ref["acc"])
    np.testing.assert_array_equal(got["facc"], ref["facc"])
    np.testing.assert_array_equal(ref["geo_acc"], want_geo)  # every row but the outlier
    assert not got["status"].any()
    # teeth: the fixes move the oracle's final position by far more than the tolerance
    on.run_log(log, nthreads=B)
    xn = on.get_state()[0]
    xo, Po = ref["states"][-1]
    sd = np.sqrt(np.diagonal(Po, axis1=1, axis2=2)[:, :3])
    moved = (np.abs(xo[:, :3] - xn[:, :3]) / sd).max()
    print("dof %d: fixes move the oracle's final position by %.3g sd" % (dof, moved))
    assert moved > 1e-7


ORACLE_PLAN = [(49, XY), (120, Z), (199, GEO), (399, XY | Z), (450, GEO), (520, GEO), (650, XY), (700, Z),
               (780, GEO), (860, XY | GEO)]
OUTLIER = (520, 3)  # (epoch, instance) of the GEO row a kilometre off


def oracle_case_fixes(log):
    """The fixes of test_fixes_match_oracle and the GEO accept pattern expected
    of the oracle ([GEO rows][batch]): XY and Z with a small R (5 cm), GEO with
    0.5 m; one GEO row 1 km north."""
    from numpy_twin import radii
    from uwvk import synth
    fx = make_fixes(log, ORACLE_PLAN)
    row = fx["geo_index"][OUTLIER[0]]
    fx["geo"][row, OUTLIER[1], 0] += 1000.0 / radii(synth.LAT0)[0]
    want = np.ones((len(fx["geo"]), log["gyro"].shape[1]), np.uint8)
    want[row, OUTLIER[1]] = 0
    return fx, want


def oracle_by_cuts(o, log, fx, records):
    """The oracle advanced piecewise: run_log to each fix epoch, the fixes as
    single updates, the state after each record epoch."""
    B, E = log["gyro"].shape[1], log["epochs"]
    acc = np.zeros((B, 4), np.uint32)
    facc = np.zeros((B, 3), np.uint32)
    geo_acc = []
    cuts = sorted({0, E} | {e + 1 for e in np.flatnonzero(fx["flags"])} | {e + 1 for e in records})
    states = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        acc += o.run_log(log, a, b - a, nthreads=B)  # (the instances are independent)
        before = facc[:, 2].copy()
        if fx["flags"][b - 1]:
            _update_at(o, fx, b - 1, None, facc)
            if fx["flags"][b - 1] & GEO:
                geo_acc.append((facc[:, 2] - before).astype(np.uint8))
        if b - 1 in records:
            states.append(o.get_state())
    return dict(states=states, acc=acc, facc=facc, geo_acc=np.array(geo_acc))


def test_fix_nan_row_is_skipped_per_instance(eng):
    """Instance 2's XY row of epoch 59 is NaN: it skips that kind (and still
    takes the epoch's Z and GEO fixes), carries UWVK_ST_NAN, and equals the cut
    reference with its XY update masked out; the others are unaffected."""
    from uwvk import synth
    B = 6
    log = synth.make_pose_log(B, 120, "C3")
    fx = make_fixes(log, PLAN)
    clean = _with_fixes(eng, _handle(eng, log), log, fx)
    fx["xy"][fx["xy_index"][59], 2, 1] = np.nan
    mask = np.ones(B, np.uint8)
    mask[2] = 0
    got = _with_fixes(eng, _handle(eng, log), log, fx)
    ref = _by_cuts(eng, _handle(eng, log), log, fx, masks={(59, XY): mask})
    _same(got, ref, ("x", "P", "acc", "facc", "pd", "pair"))
    want = np.zeros(B, np.uint32)
    want[2] = 0x2  # UWVK_ST_NAN
    np.testing.assert_array_equal(got["status"], want)
    assert not ref["status"].any()
    np.testing.assert_array_equal(got["facc"][2], clean["facc"][2] - [1, 0, 0])
    others = [i for i in range(B) if i != 2]
    np.testing.assert_array_equal(got["x"][others], clean["x"][others])
    np.testing.assert_array_equal(got["P"][others], clean["P"][others])
    assert np.abs(got["x"][2] - clean["x"][2]).max() > 0


def test_fix_arguments(eng):
    from uwvk import abi, synth
    B, E = 6, 60
    log = synth.make_pose_log(B, E, "C3")
    fx = make_fixes(log, [(10, XY), (20, Z), (30, GEO), (59, XY | Z | GEO)])
    g = _handle(eng, log)
    dlog, dfx = g.upload_log(log), g.upload_fixes(fx)
    x0, P0 = g.get_state()

    def call(s, first=0, count=E, track=None):
        return g.L.uwvk_pose_run_log_fixes(g.h, C.byref(dlog.s), C.byref(s) if s is not None else None,
                                           C.c_int64(first), C.c_int64(count), None, track)

    def variant(**kw):
        s = abi.PoseFixes.from_buffer_copy(dfx.s)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    keep = []

    def arr(a, dtype):
        keep.append(np.ascontiguousarray(a, dtype=dtype))
        return keep[-1].ctypes.data

    def with_flag(e, v):
        f = fx["flags"].copy()
        f[e] = v
        return arr(f, np.uint32)

    def with_index(k, e, v):
        i = fx[k + "_index"].copy()
        i[e] = v
        return arr(i, np.int32)

    bad = dict(
        flags_null=variant(host_flags=None),
        flag_bit=variant(host_flags=with_flag(5, 0x8)),
        flag_ev_bit=variant(host_flags=with_flag(5, XY | 0x10)),
        xy_index_null=variant(xy_index=None), xy_null=variant(xy=None),
        z_index_null=variant(z_index=None), z_null=variant(z=None),
        geo_index_null=variant(geo_index=None), geo_null=variant(geo=None),
        xy_index_neg=variant(xy_index=with_index("xy", 10, -1)),
        xy_index_past=variant(xy_index=with_index("xy", 10, 2)),
        z_index_past=variant(z_index=with_index("z", 59, 2)),
        geo_index_neg=variant(geo_index=with_index("geo", 30, -7)),
        geo_index_past=variant(geo_index=with_index("geo", 59, 1 << 20)),
        xy_unflagged_kind=variant(host_flags=with_flag(40, XY)),  # flagged, its index there is -1
    )
    for name, s in bad.items():
        assert call(s) == 1, name  # UWVK_EINVAL
        x, P = g.get_state()
        np.testing.assert_array_equal(x, x0, err_msg=name)
        np.testing.assert_array_equal(P, P0, err_msg=name)
    assert not g.get_status().any()
    # the check covers [first, first + count) only; the errors of run_log_track stay
    assert call(variant(xy_index=with_index("xy", 59, 99)), 0, 0) == 0
    assert call(dfx.s, 0, E + 1) == 1
    tr = abi.PoseTrack()
    tr.every = 0
    assert call(dfx.s, 0, E, C.byref(tr)) == 1
    np.testing.assert_array_equal(g.get_state()[1], P0)


def test_null_fixes_and_zero_flags(eng):
    """fixes = NULL is run_log_track (track = NULL too: run_log); fix flags all
    zero is run_log, bitwise."""
    from uwvk import abi, synth
    B, E = 6, 60
    log = synth.make_pose_log(B, E, "C3")
    ga, gb, gc, gd, ge = (_handle(eng, log) for _ in range(5))
    ref_acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    tref = gb.run_log_track(gb.upload_log(log), 20, accept_counts=ref_acc)
    ref = dict(x=gb.get_state()[0], P=gb.get_state()[1], acc=ref_acc.read(np.uint32, (B, 4)), mean=tref.mean())
    # NULL fixes, a track
    dlog = ga.upload_log(log)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    mean = eng.DeviceBuffer.empty(3 * B * 54 * 8)
    tr = abi.PoseTrack()
    tr.every, tr.capacity, tr.mean = 20, 3, mean.ptr
    eng._chk(ga.L.uwvk_pose_run_log_fixes(ga.h, C.byref(dlog.s), None, C.c_int64(0), C.c_int64(E), acc.ptr,
                                          C.byref(tr)))
    ga.synchronize()
    np.testing.assert_array_equal(mean.read(np.float64, (3, B, 54)), ref["mean"])
    np.testing.assert_array_equal(ga.get_state()[1], ref["P"])
    np.testing.assert_array_equal(acc.read(np.uint32, (B, 4)), ref["acc"])
    # NULL fixes, NULL track
    dlog = gc.upload_log(log)
    eng._chk(gc.L.uwvk_pose_run_log_fixes(gc.h, C.byref(dlog.s), None, C.c_int64(0), C.c_int64(E), None, None))
    gc.synchronize()
    plain_acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    gd.run_log(gd.upload_log(log), accept_counts=plain_acc)
    plain = gd.get_state()
    for a, b in zip(gc.get_state(), plain):
        np.testing.assert_array_equal(a, b)
    # flags all zero, payloads present
    fx = make_fixes(log, [(10, XY), (20, Z | GEO)])
    fx["flags"][:] = 0
    got = _with_fixes(eng, ge, log, fx)
    np.testing.assert_array_equal(got["x"], plain[0])
    np.testing.assert_array_equal(got["P"], plain[1])
    np.testing.assert_array_equal(got["acc"], plain_acc.read(np.uint32, (B, 4)))
    assert not got["facc"].any() and (got["pair"], got["pd"]) == (gd.pair_active(), gd.param_block())


def test_mission_replay_with_fixes(eng):
    """mission.replay passes the log's fixes on."""
    from uwvk import mission, synth
    log = synth.make_pose_log(6, 60, "C3")
    log["fixes"] = make_fixes(log, [(10, XY), (29, Z | GEO)])
    g, r = _handle(eng, log), _handle(eng, log)
    out = mission.replay(g, log, 30)
    ref = _by_cuts(eng, r, log, log["fixes"], records=(29, 59))
    np.testing.assert_array_equal(out["mean"], ref["mean"])
    np.testing.assert_array_equal(out["variance"], ref["variance"])
