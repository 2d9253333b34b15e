"""The pair epoch kernel's fused half-wide broadcasts (csrc/uwvk_psp_dev.hpp
rep16 / fmac_bc, r10): the predict's Delta loop and the update's P / Dz loop
read their broadcast operand from the source lane's registers inside the fp64
FMA (v_fmac_f64 with a DPP row_newbcast source) instead of through an LDS
round trip.  Every FMA is the one the kernel ran before, in the same order
(the first P step with the product rounded on its own, as the compiler had
it), so the results are bitwise what they were: the fixtures
tests/golden/pair_bcast_*.npz were recorded on an MI355X from the library of
the commit before the change (tests/golden/record_pair_bcast.py names it) for
exactly these inputs.

The shapes are the smallest that run every fused site: one wave (batch 2, two
unlike instances, each started through init_from_state with its own parameter
means, density and orientation) for three epochs, the second of which carries
the DVL sample (M = 3: P in lanes 0..17, the upper row's copy for lanes 16 and
17) or, in the ADCP scenes, four ADCP cells (M = 2, the EVS = 0 kernels); 53 DOF
(PD = 1) and 26 DOF (PD = 0) on both SO3 sides.  A wave whose other instance
skips an update runs the fused sites with that half of the wave off: batch 6
with a NaN acceleration sample in a lower-half instance and a NaN DVL sample in
an upper-half instance."""
import hashlib
import os

import numpy as np
import pytest

from test_gpu_pair_units import ST_NAN, _check_pair_against_single

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = [(kind, dof, side) for kind in ("dvl", "adcp") for dof in (53, 26) for side in ("right", "left")]
NAN_ACC = (0, 2)   # (epoch, instance): instance 2 is the lower half of wave 1
NAN_DVL_INST = 5   # the upper half of wave 2, at the DVL epoch


@pytest.fixture(scope="module")
def eng():
    from uwvk import engine
    if not engine.device_available(0):
        pytest.fail("no gfx950 device / libuwvk.so not loadable: the HIP path is mandatory")
    return engine


def make_log(kind, B, dof):
    """Three epochs with the event in the second: `dvl` is epochs 198..200 of the
    C3 mission (the 5 Hz DVL sample falls on epoch 199), `adcp` a C4 log with
    the ADCP period set to two epochs (four cells, d2p95 gate; no pressure,
    DVL or BodyEfforts sample within three epochs)."""
    from uwvk import abi, synth
    if kind == "dvl":
        log = synth.make_pose_log(B, 3, "C3", dof=dof, epoch0=198)
        want = abi.EV_ACC | abi.EV_DVL
    else:
        log = synth.make_pose_log(B, 3, "C4", dof=dof, adcp_every=2)
        want = abi.EV_ACC | abi.EV_ADCP
    assert [int(f) for f in log["flags"]] == [abi.EV_ACC, want, abi.EV_ACC]
    return log


_STARTS = {}


def start(eng, kind, B, dof):
    """(log, x, P): every instance's start distinct (as test_gpu_pair_boundary);
    made once per shape, shared and left unchanged."""
    key = (kind, B, dof)
    if key not in _STARTS:
        from uwvk import synth
        cfg, uwv = synth.default_pose_config(), synth.default_uwv()
        log = make_log(kind, B, dof)
        g = eng.PoseUKFBatch(B, dof)
        g.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
        x, P = g.get_state()
        i = np.arange(B, dtype=np.float64)
        if dof == 53:
            x[:, 20:47] += 1e-3 * (1.0 + i[:, None] / B + np.arange(27)[None, :] / 64.0)
        x[:, -1] *= 1.0 + 1e-3 * (i + 1.0) / B
        assert len(np.unique(np.round(x[:, 3:7], 12), axis=0)) == B
        _STARTS[key] = (log, x, P)
    return _STARTS[key]


def run(eng, st, pair, dof, side, log=None):
    """(state, covariance, accept counts, status) after the three epochs."""
    from uwvk import abi, synth
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    log0, x, P = st
    log = log or log0
    B = len(x)
    g = eng.PoseUKFBatch(B, dof)
    g.set_so3_right(side == "right")
    g.set_pair(pair)
    loc = abi.Location(cfg.location.latitude, cfg.location.longitude, cfg.location.altitude)
    g.init_from_state(x, P, loc, uwv, synth.pose_parameter(cfg))
    g.set_process_noise_from_config(cfg, 1e-3)
    assert g.pair_active() == (1 if pair else 0)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    g.run_log(g.upload_log(log), accept_counts=acc)
    xo, Po = g.get_state()
    return xo, Po, acc.read(np.uint32, (B, 4)), g.get_status()


def inputs_digest(st, log=None):
    """sha256 over the start and the measurement rows a run reads."""
    log0, x, P = st
    log = log or log0
    h = hashlib.sha256()
    for a in (x, P, log["flags"], log["gyro"], log["acc"], log["dvl"], log["dvl_index"], log["adcp"],
              log["adcp_index"]):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def nan_logs(clean):
    """clean with a NaN acceleration sample (NAN_ACC) and a NaN DVL sample
    (instance NAN_DVL_INST); and the two logs in which no instance has that
    acceleration / DVL update at all (the event's flag cleared)."""
    from uwvk import abi
    dv = int(np.flatnonzero((clean["flags"] & abi.EV_DVL) != 0)[0])
    bad = dict(clean)
    bad["acc"] = clean["acc"].copy()
    bad["dvl"] = clean["dvl"].copy()
    bad["acc"][NAN_ACC[0], NAN_ACC[1], 1] = np.nan
    bad["dvl"][clean["dvl_index"][dv], NAN_DVL_INST, 2] = np.nan
    no_acc, no_dvl = dict(clean), dict(clean)
    no_acc["flags"] = clean["flags"].copy()
    no_acc["flags"][NAN_ACC[0]] &= ~np.uint32(abi.EV_ACC)
    no_dvl["flags"] = clean["flags"].copy()
    no_dvl["flags"][dv] &= ~np.uint32(abi.EV_DVL)
    return bad, no_acc, no_dvl


def scene_key(kind, dof, side):
    return "%s_%d_%s" % (kind, dof, side)


def golden(name):
    return np.load(os.path.join(GOLDEN, "pair_bcast_%s.npz" % name))


def assert_golden(z, key, got, digest):
    assert str(z[key + "_inputs"]) == digest, "the scene's inputs are not the recorded ones: " + key
    for part, a in zip(("x", "P", "status"), (got[0], got[1], got[3])):
        ref = z["%s_%s" % (key, part)]
        print("%s %s: %d of %d entries differ from the fixture" % (key, part, (a != ref).sum(), a.size))
        np.testing.assert_array_equal(a, ref, err_msg="%s %s" % (key, part))


@pytest.mark.parametrize("kind,dof,side", SCENES)
def test_one_wave(eng, kind, dof, side):
    """Batch 2, three epochs, the DVL sample or the four ADCP cells in the
    second: the pair kernel within 1e-9 (sigma units) of the one-instance
    kernel, and bitwise the fixture."""
    st = start(eng, kind, 2, dof)
    got = run(eng, st, True, dof, side)
    one = run(eng, st, False, dof, side)
    if kind == "adcp":
        assert got[2][:, 2].sum() > 0  # cells were accepted: the M = 2 update ran
    _check_pair_against_single((*got, None), (*one, None), dof)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert not np.array_equal(got[0][0], got[0][1])  # two unlike instances
    assert_golden(golden(kind), scene_key(kind, dof, side), got, inputs_digest(st))


def test_half_masked(eng):
    """Batch 6 (three waves).  Instance 2 (a lower half) skips its acceleration
    update at epoch 0, instance 5 (an upper half) its DVL update: the fused sites
    of instances 3 and 4 run with the other half of their wave off.  Every
    other instance is bitwise the clean run; instance 2 is bitwise its run
    without that epoch's acceleration update, instance 5 bitwise its run
    without the DVL update; both carry UWVK_ST_NAN, the others no status bit.
    The clean and the NaN run are bitwise the fixture, and the NaN run is
    within 1e-9 of the one-instance kernel on the same log."""
    from helpers import cov_err, state_err
    st = start(eng, "dvl", 6, 53)
    bad, no_acc, no_dvl = nan_logs(st[0])
    clean = run(eng, st, True, 53, "right")
    got = run(eng, st, True, 53, "right", log=bad)
    one = run(eng, st, False, 53, "right", log=bad)
    pa = run(eng, st, True, 53, "right", log=no_acc)
    pd = run(eng, st, True, 53, "right", log=no_dvl)
    assert not clean[3].any()
    want_status = [0, 0, ST_NAN, 0, 0, ST_NAN]
    assert list(got[3]) == want_status and list(one[3]) == want_status
    others = [0, 1, 3, 4]
    for name, a, b in zip(("state", "covariance", "accept counts"), got, clean):
        np.testing.assert_array_equal(a[others], b[others], err_msg=name)
    for name, a, b, c in zip(("state", "covariance"), got, pa, pd):
        np.testing.assert_array_equal(a[NAN_ACC[1]], b[NAN_ACC[1]], err_msg="%s: skipped acceleration update" % name)
        np.testing.assert_array_equal(a[NAN_DVL_INST], c[NAN_DVL_INST], err_msg="%s: skipped DVL update" % name)
    # the skipped updates changed those instances (the NaNs reached the kernel)
    assert not np.array_equal(got[0][NAN_ACC[1]], clean[0][NAN_ACC[1]])
    assert not np.array_equal(got[0][NAN_DVL_INST], clean[0][NAN_DVL_INST])
    assert got[2][NAN_DVL_INST, 0] == 0 and (got[2][:NAN_DVL_INST, 0] == 1).all()
    np.testing.assert_array_equal(got[2], one[2])
    es, ec = state_err(got[0], one[0], one[1], 53), cov_err(got[1], one[1])
    print("half-masked pair vs single: state %s, cov %s" % (es, ec))
    assert es.max() < 1e-9 and ec.max() < 1e-9
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    z = golden("nan")
    assert_golden(z, "clean", clean, inputs_digest(st))
    assert_golden(z, "nan", got, inputs_digest(st, bad))
