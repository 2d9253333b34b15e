"""The pair epoch kernel's tiled rank-M update (csrc/uwvk_psp_dev.hpp
rankm_tiles, csrc/uwvk_tiles.hpp) at the smallest shapes where it can go wrong.

Sigma~ -= C~ K~^T runs on 4x4 register tiles, one tile of the block triangle
per local lane of a 32-lane half.  The pair kernel is compared against the
one-instance kernel (set_pair(0): the MFMA rank-M update) and against the CPU
oracle, with the tolerances of test_gpu_pd.py::test_pair_*: 1e-9 in sigma
units against the one-instance kernel, 1e-7 against the oracle, accept counts
and status words bitwise.

* one pair unit (batch 2) over a few epochs with a DVL epoch among plain
  acceleration epochs: rank 3, for a 53-DOF decoupled handle (PD = 1) and a
  26-DOF handle (PD = 0);
* the same with a C4-style log holding an ADCP epoch: rank 2 (4 cells) in the
  kernel that has the ADCP update compiled in (EVS = 0);
* batch 6 with a NaN measurement in one instance of two pair units (a lower and
  an upper half): that half skips its update while the other half of the wave
  runs it -- the other instances are bitwise the clean run's, and the skipping
  instance's state and Sigma are bitwise the prediction's (a run whose last
  epoch carries no measurement at all);
* a run across epoch 1,023 at batch 2: the time-scale fold, after which the
  Cholesky panels and the update work on re-scaled DOFs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ST_NAN = 0x2  # UWVK_ST_NAN
NAMES = ("state", "covariance", "accept counts", "status", "rotation rate")


@pytest.fixture(scope="module")
def eng():
    from uwvk import engine
    if not engine.device_available(0):
        pytest.fail("no gfx950 device / libuwvk.so not loadable: the HIP path is mandatory")
    return engine


def _run(eng, log, pair, dof=53):
    from uwvk import synth
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    B = log["gyro"].shape[1]
    g = eng.PoseUKFBatch(B, dof)
    g.set_pair(pair)
    g.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    g.set_process_noise_from_config(cfg, 1e-3)
    assert g.pair_active() == (1 if pair else 0)
    acc = eng.DeviceBuffer(np.zeros((B, 4), np.uint32))
    g.run_log(g.upload_log(log), accept_counts=acc)
    x, P = g.get_state()
    return x, P, acc.read(np.uint32, (B, 4)), g.get_status(), g.get_rotation_rate()


def _oracle(log, dof):
    from uwvk import synth
    import oracle_ctypes as orc
    cfg, uwv = synth.default_pose_config(), synth.default_uwv()
    o = orc.OraclePoseBatch(log["gyro"].shape[1], dof)
    o.init_from_config(log["pos0"], log["pos_cov"], log["rot0"], log["rot_cov"], cfg, uwv)
    o.set_process_noise_from_config(cfg, 1e-3)
    counts = o.run_log(log)
    x, P = o.get_state()
    return x, P, counts


def _check(eng, log, dof):
    """pair against one-instance (1e-9, gates and status bitwise) and against
    the oracle (1e-7, accept counts bitwise)."""
    from helpers import cov_err, state_err
    got, one = _run(eng, log, True, dof), _run(eng, log, False, dof)
    xo, Po, co = _oracle(log, dof)
    np.testing.assert_array_equal(got[2], one[2])
    np.testing.assert_array_equal(got[3], one[3])
    assert not got[3].any()
    np.testing.assert_array_equal(got[2], co)
    es, ec = state_err(got[0], one[0], one[1], dof), cov_err(got[1], one[1])
    eso, eco = state_err(got[0], xo, Po, dof), cov_err(got[1], Po)
    print("pair vs single: state %.3g, cov %.3g; vs oracle: state %.3g, cov %.3g (sigma units)"
          % (es.max(), ec.max(), eso.max(), eco.max()))
    assert es.max() < 1e-9 and ec.max() < 1e-9
    assert eso.max() < 1e-7 and eco.max() < 1e-7
    # the lower triangle the kernel keeps comes back as a symmetric matrix
    np.testing.assert_array_equal(got[1], np.swapaxes(got[1], 1, 2))
    return got


@pytest.mark.parametrize("dof", [53, 26])
def test_one_pair_unit_rank3(eng, dof):
    """Batch 2, epochs 197..201 of the mission: the DVL epoch 199 among plain
    acceleration epochs (two rank-3 updates in one epoch, one in the others)."""
    from uwvk import abi, synth
    log = synth.make_pose_log(2, 5, "C3", dof=dof, epoch0=197)
    assert list(np.flatnonzero(log["flags"] & abi.EV_DVL)) == [2]
    assert (log["flags"] & abi.EV_ACC).all()
    got = _check(eng, log, dof)
    assert (got[2][:, 0] == 1).all()  # the DVL update ran and was accepted


@pytest.mark.parametrize("dof", [53, 26])
def test_one_pair_unit_rank2_adcp(eng, dof):
    """Batch 2, 10 epochs of a C4-style log with an ADCP sample every 7th
    (epoch 6: four cells, rank 2 each, gated) and no pressure epoch: the
    launch runs k_psp_epoch_pair<SR, 0, PD>."""
    from uwvk import abi, synth
    log = synth.make_pose_log(2, 10, "C4", dof=dof, adcp_every=7)
    fl = log["flags"]
    assert list(np.flatnonzero(fl & abi.EV_ADCP)) == [6]
    assert not (fl & (abi.EV_PRESSURE | abi.EV_EFFORTS)).any()
    got = _check(eng, log, dof)
    assert (got[2][:, 2] > 0).all()  # ADCP cells accepted


def test_half_skips_its_update(eng):
    """Batch 6 (three pair units), 4 epochs; in the last epoch instance 2 (the
    lower half of unit 1) and instance 5 (the upper half of unit 2) have a NaN
    acceleration sample."""
    from uwvk import abi, synth
    B, E = 6, 4
    clean = synth.make_pose_log(B, E, "C3")
    assert (clean["flags"] == abi.EV_ACC).all()
    bad = dict(clean)
    bad["acc"] = clean["acc"].copy()
    bad["acc"][E - 1, 2, 1] = np.nan
    bad["acc"][E - 1, 5, 0] = np.nan
    nomeas = dict(clean)  # the last epoch predicts only
    nomeas["flags"] = clean["flags"].copy()
    nomeas["flags"][E - 1] = 0
    ref, got, pred = _run(eng, clean, True), _run(eng, bad, True), _run(eng, nomeas, True)
    keep = [0, 1, 3, 4]
    for name, a, b in zip(NAMES, got, ref):
        np.testing.assert_array_equal(a[keep], b[keep], err_msg=name)
    assert list(got[3]) == [0, 0, ST_NAN, 0, 0, ST_NAN]
    for i in (2, 5):
        np.testing.assert_array_equal(got[0][i], pred[0][i])
        np.testing.assert_array_equal(got[1][i], pred[1][i])
        assert not np.array_equal(got[1][i], ref[1][i])  # the skipped update would have changed Sigma
    assert not pred[3].any() and not ref[3].any()
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()


def test_across_the_fold(eng):
    """Batch 2, 1,030 epochs in one launch (five DVL epochs, 199 .. 999): the
    fold at the launch's epoch 1,023, then six more epochs of predicts and
    updates on the re-scaled Sigma~."""
    from uwvk import abi, synth
    log = synth.make_pose_log(2, 1030, "C3")
    assert ((log["flags"] & abi.EV_DVL) != 0).sum() == 5
    _check(eng, log, 53)
